"""The C-ABI and header side of the convex-gap POA, without a GPU: the ctypes mirror of hx_poa_convex_params has the C layout, the three
entry points and the option are exported, every refusal carries the offending score and its value, a caller compiled against
include/spoa_hx.hpp constructs seven-score engines and is refused bad scores, and without a device a consensus fails loudly."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from haslr_amd import ctypes_defs as T
from haslr_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("hx_poa_sequences_convex", "hx_poa_msa_convex", "hx_poa_weighted_convex")
FIELDS = ("match", "mismatch", "gap_open", "gap_extend", "gap_open2", "gap_extend2", "type")
# (g, e, q, c, type) and the text the refusal ends its entry's name with
REFUSALS = [
    ((0, 0, -10, -4, 1), "the gap open score must be negative, not 0"),
    ((-8, 1, -10, -4, 1), "the gap extend score must not be positive, not 1"),
    ((-2, -8, -10, -4, 1), "the gap extend score -8 is below the gap open score -2 (extending a gap must not cost more than opening one)"),
    ((-8, -6, 0, 0, 1), "the second gap open score must be negative, not 0"),
    ((-8, -6, -10, 2, 1), "the second gap extend score must not be positive, not 2"),
    ((-8, -6, -10, -12, 1), "the second gap extend score -12 is below the second gap open score -10 (extending a gap must not cost more than opening one)"),
    ((-8, -6, -7, -4, 1), "the second gap open score -7 is above the first gap open score -8 (the first piece is the one that opens no dearer)"),
    ((-8, -6, -10, -4, 3), "unknown alignment type 3 (HX_POA_SW 0, HX_POA_NW 1, HX_POA_OV 2)"),
    ((-8, -6, -10, -4, -1), "unknown alignment type -1 (HX_POA_SW 0, HX_POA_NW 1, HX_POA_OV 2)"),
]


@pytest.fixture(scope="module")
def convex_caller(built, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("spoa_convex") / "spoa_convex_caller")
    lib = os.path.join(ROOT, "haslr_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "spoa_convex_caller.cpp"), "-o", exe,
                           "-L", lib, "-lhaslr_hip", "-pthread", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_convex_params_layout_matches_c(built, tmp_path):
    items = ["sizeof(hx_poa_convex_params)"] + [f"offsetof(hx_poa_convex_params,{f})" for f in FIELDS]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "haslr_types.h"\nint main(){printf("' + " ".join(["%zu"] * len(items)) + '\\n",' + ",".join(items) + ");return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [C.sizeof(T.PoaConvexParams)] + [getattr(T.PoaConvexParams, f).offset for f in FIELDS]
    assert got[0] == 28


def test_entry_points_and_option_are_exported(built):
    for name in ENTRIES:
        assert hasattr(hip.lib(), name) and name in hip.SYMBOLS
    assert "poa_convex" in hip.option_names()


def call_entry(name, params, handle=None):
    """the entry on one set of one sequence; (return code, last error). Validation comes before the context is touched."""
    off, soff = np.array([0, 1], dtype=np.uint64), np.array([0, 4], dtype=np.uint64)
    args = [handle, 1, off.ctypes.data_as(T.u64p), soff.ctypes.data_as(T.u64p), b"ACGT"]
    fn = getattr(hip.lib(), name)
    if name == "hx_poa_sequences_convex":
        rc = fn(*args, params, C.byref(T.CnsOut()))
    elif name == "hx_poa_msa_convex":
        rc = fn(*args, params, 1, C.byref(T.MsaOut()))
    else:
        rc = fn(*args, None, params, 1, 1, C.byref(T.WcnsOut()))
    return rc, hip.lib().hx_last_error().decode()


@pytest.mark.parametrize("name", ENTRIES)
def test_every_refusal_names_the_score_and_its_value(built, name):
    for (g, e, q, c, ty), text in REFUSALS:
        rc, err = call_entry(name, C.byref(T.PoaConvexParams(5, -4, g, e, q, c, ty)))
        assert rc != 0 and err == f"{name}: {text}", (name, g, e, q, c, ty, err)
    rc, err = call_entry(name, None)
    assert rc != 0 and err == f"{name}: no parameters"


def test_the_python_methods_want_both_scores_of_the_second_piece():
    class NoDevice:
        _h = None
    for method in (hip.HipContext.poa_msa, hip.HipContext.poa_weighted):
        with pytest.raises(ValueError, match="give gap_open2 and gap_extend2, or neither"):
            method(NoDevice(), [["ACGT"]], gap_open2=-10)
        with pytest.raises(ValueError, match="give gap_open2 and gap_extend2, or neither"):
            method(NoDevice(), [["ACGT"]], gap_extend2=-4)


def test_seven_score_engines_can_be_constructed_and_bad_scores_throw(convex_caller):
    r = subprocess.run([convex_caller, "--construct"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "ok\n", (r.returncode, r.stderr)


def test_convex_consensus_without_a_device_fails_loudly(convex_caller):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a HIP device is present: covered by tests/test_poa_convex_gpu.py")
    for t in ("sw", "nw", "ov"):
        for flag in ([], ["--outputs"], ["--batch"]):
            r = subprocess.run([convex_caller] + flag, input=f"{t} 5 -4 -8 -6 -10 -4\nACGTACGT\nACGTTCGT\n", capture_output=True, text=True)
            assert r.returncode == 1 and "no HIP device" in r.stderr and r.stdout == "", (t, flag, r.returncode, r.stderr)
