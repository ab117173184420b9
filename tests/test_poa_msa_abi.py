"""The C-ABI and header side of the MSA output, without a GPU: the ctypes mirrors of hx_poa_msa_params and hx_msa_out have the C sizes and
offsets, the two entry points are exported, and a caller compiled against include/spoa_hx.hpp that asks a graph for
generate_multiple_sequence_alignment fails loudly without a device."""
import ctypes as C
import os
import subprocess

import pytest

from haslr_amd import ctypes_defs as T
from haslr_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAM_FIELDS = ["match", "mismatch", "gap_open", "gap_extend", "type", "include_consensus"]
OUT_FIELDS = ["n_set", "n_rows", "n_cols", "msa_off", "msa", "cns_off", "cns", "dp_cells", "seq_bases", "n_aligned", "rows_kernel_ms", "rows_kernel_bytes"]


@pytest.fixture(scope="module")
def msa_caller(built, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("spoa_msa") / "spoa_msa_caller")
    lib = os.path.join(ROOT, "haslr_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "spoa_msa_caller.cpp"), "-o", exe,
                           "-L", lib, "-lhaslr_hip", "-pthread", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_struct_sizes_and_offsets_match_c(built, tmp_path):
    src = tmp_path / "sz.c"
    items = ["sizeof(hx_poa_msa_params)"] + [f"offsetof(hx_poa_msa_params,{f})" for f in PARAM_FIELDS] + \
            ["sizeof(hx_msa_out)"] + [f"offsetof(hx_msa_out,{f})" for f in OUT_FIELDS] + ["sizeof(hx_cns_out)"]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "haslr_types.h"\nint main(){' +
                   "".join(f'printf("%zu\\n",(size_t){it});' for it in items) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    want = [C.sizeof(T.PoaMsaParams)] + [getattr(T.PoaMsaParams, f).offset for f in PARAM_FIELDS] + \
           [C.sizeof(T.MsaOut)] + [getattr(T.MsaOut, f).offset for f in OUT_FIELDS] + [C.sizeof(T.CnsOut)]
    assert got == want
    assert got[0] == 24 and [n for n, _ in T.PoaMsaParams._fields_] == PARAM_FIELDS and [n for n, _ in T.MsaOut._fields_] == OUT_FIELDS
    assert got[-1] == 48   # hx_cns_out is as it was: the MSA has a struct of its own


def test_entry_points_are_exported(built):
    assert hasattr(hip.lib(), "hx_poa_msa") and hasattr(hip.lib(), "hx_free_msa")
    assert "hx_poa_msa" in hip.SYMBOLS and "hx_free_msa" in hip.SYMBOLS


def test_msa_without_a_device_fails_loudly(msa_caller):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a HIP device is present: covered by tests/test_poa_msa_gpu.py")
    for args in ([], ["--batch"]):
        for head in ("nw", "sw +c", "ov 5 -4 -8 -2", "nw 5 -4 -8 -2 +c"):
            r = subprocess.run([msa_caller] + args, input=f"{head}\nACGTACGT\nACGTTCGT\n", capture_output=True, text=True)
            assert r.returncode == 1 and "no HIP device" in r.stderr and r.stdout == "", (args, head, r.returncode, r.stderr)


def test_a_graph_without_sequences_has_no_rows_and_needs_no_device(msa_caller):
    r = subprocess.run([msa_caller], input="nw +c\n-\n", capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "=\n", (r.returncode, r.stderr)
