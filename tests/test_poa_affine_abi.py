"""The C-ABI and header side of the affine-gap POA, without a GPU: the ctypes mirror of hx_poa_affine_params has the C size, the entry
point and its option are exported, a caller compiled against include/spoa_hx.hpp constructs five-score engines and is refused bad scores,
and without a device its consensus fails loudly."""
import ctypes as C
import os
import subprocess

import pytest

from haslr_amd import ctypes_defs as T
from haslr_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def affine_caller(built, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("spoa_affine") / "spoa_affine_caller")
    lib = os.path.join(ROOT, "haslr_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "spoa_affine_caller.cpp"), "-o", exe,
                           "-L", lib, "-lhaslr_hip", "-pthread", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_affine_params_size_matches_c(built, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "haslr_types.h"\nint main(){printf("%zu %zu %zu %zu\\n",sizeof(hx_poa_affine_params),'
                   'offsetof(hx_poa_affine_params,gap_open),offsetof(hx_poa_affine_params,gap_extend),offsetof(hx_poa_affine_params,type));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [C.sizeof(T.PoaAffineParams), T.PoaAffineParams.gap_open.offset, T.PoaAffineParams.gap_extend.offset, T.PoaAffineParams.type.offset]
    assert got[0] == 20


def test_entry_point_and_option_are_exported(built):
    assert hasattr(hip.lib(), "hx_poa_sequences_affine")
    assert "poa_affine" in hip.option_names()


def test_five_score_engines_can_be_constructed_and_bad_scores_throw(affine_caller):
    r = subprocess.run([affine_caller, "--construct"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "ok\n", (r.returncode, r.stderr)


def test_affine_consensus_without_a_device_fails_loudly(affine_caller):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a HIP device is present: covered by tests/test_poa_affine_gpu.py")
    for t in ("sw", "nw", "ov"):
        r = subprocess.run([affine_caller], input=f"{t} 5 -4 -8 -2\nACGTACGT\nACGTTCGT\n", capture_output=True, text=True)
        assert r.returncode == 1 and "no HIP device" in r.stderr and r.stdout == "", (t, r.returncode, r.stderr)
