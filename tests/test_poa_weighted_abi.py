"""The C-ABI and header side of base weights and coverage, without a GPU: the ctypes mirrors of hx_poa_weighted_params and hx_wcns_out
have the C sizes and offsets, the two entry points are exported and the option is listed, the header's three add_alignment overloads
throw on what they refuse, and a caller compiled against include/spoa_hx.hpp that uses weights or asks for the coverage fails loudly
without a device while a graph without sequences needs none."""
import ctypes as C
import os
import subprocess

import pytest

from haslr_amd import ctypes_defs as T
from haslr_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAM_FIELDS = ["match", "mismatch", "gap_open", "gap_extend", "type", "want_coverage", "want_profile"]
OUT_FIELDS = ["n_set", "cns_off", "cns", "coverage", "profile", "dp_cells", "seq_bases", "n_aligned", "cov_kernel_ms", "cov_kernel_bytes"]


@pytest.fixture(scope="module")
def weighted_caller(built, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("spoa_weighted") / "spoa_weighted_caller")
    lib = os.path.join(ROOT, "haslr_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "spoa_weighted_caller.cpp"), "-o", exe,
                           "-L", lib, "-lhaslr_hip", "-pthread", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_struct_sizes_and_offsets_match_c(built, tmp_path):
    src = tmp_path / "sz.c"
    items = ["sizeof(hx_poa_weighted_params)"] + [f"offsetof(hx_poa_weighted_params,{f})" for f in PARAM_FIELDS] + \
            ["sizeof(hx_wcns_out)"] + [f"offsetof(hx_wcns_out,{f})" for f in OUT_FIELDS] + ["sizeof(hx_cns_out)", "sizeof(hx_msa_out)"]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "haslr_types.h"\nint main(){' +
                   "".join(f'printf("%zu\\n",(size_t){it});' for it in items) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    want = [C.sizeof(T.PoaWeightedParams)] + [getattr(T.PoaWeightedParams, f).offset for f in PARAM_FIELDS] + \
           [C.sizeof(T.WcnsOut)] + [getattr(T.WcnsOut, f).offset for f in OUT_FIELDS] + [C.sizeof(T.CnsOut), C.sizeof(T.MsaOut)]
    assert got == want
    assert got[0] == 28 and [n for n, _ in T.PoaWeightedParams._fields_] == PARAM_FIELDS and [n for n, _ in T.WcnsOut._fields_] == OUT_FIELDS
    assert got[-2:] == [48, 96]   # hx_cns_out and hx_msa_out are as they were: the weighted entry has a struct of its own


def test_entry_points_and_option_are_exported(built):
    assert hasattr(hip.lib(), "hx_poa_weighted") and hasattr(hip.lib(), "hx_free_wcns")
    assert "hx_poa_weighted" in hip.SYMBOLS and "hx_free_wcns" in hip.SYMBOLS
    assert "poa_weighted" in hip.option_names()


def test_the_header_throws_on_bad_weights(weighted_caller):
    r = subprocess.run([weighted_caller, "--throws"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "throws ok\n", (r.returncode, r.stdout, r.stderr)


def test_weights_and_coverage_without_a_device_fail_loudly(weighted_caller):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a HIP device is present: covered by tests/test_poa_weighted_gpu.py")
    for args in ([], ["--batch"]):
        for text in ("nw\nACGTACGT w 3\nACGTTCGT w 3\n", "sw +cov\nACGTACGT\nACGTTCGT\n", "ov 5 -4 -8 -2\nACGTACGT q IIIIIIII\nACGTTCGT q 55555555\n",
                     "nw 5 -4 -8 -2 +cov\nACGTACGT v 1,2,3,4,5,6,7,255\nACGTTCGT\n"):
            r = subprocess.run([weighted_caller] + args, input=text, capture_output=True, text=True)
            assert r.returncode == 1 and "no HIP device" in r.stderr and r.stdout == "", (args, text, r.returncode, r.stderr)


def test_a_graph_without_sequences_has_no_coverage_and_needs_no_device(weighted_caller):
    r = subprocess.run([weighted_caller], input="nw +cov\n- w 9\n", capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "\n\n=\n", (r.returncode, r.stdout, r.stderr)
