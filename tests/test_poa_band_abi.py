"""The C-ABI, Python and header side of banded alignment, without a GPU: the ctypes mirrors of hx_poa_band_params and hx_band_out have the C
sizes and offsets, the two entry points are exported and listed, hx_poa_banded refuses bad parameters with its own name in front before it
touches a context, HipContext.poa_banded checks its weights before it needs a device, and a caller compiled against spoa_hx.hpp
(spoa::hx::banded_batch) fails loudly without one."""
import ctypes as C
import os
import subprocess

import pytest

from haslr_amd import ctypes_defs as T
from haslr_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAM_FIELDS = ["band", "want_msa", "include_consensus", "want_coverage", "want_profile"]
OUT_FIELDS = ["n_set", "cns_off", "cns", "band_used", "n_rows", "n_cols", "msa_off", "msa", "coverage", "profile", "dp_cells", "seq_bases", "n_aligned", "workspace_bytes",
              "slot_reruns", "band_reruns"]


def test_struct_sizes_and_offsets_match_c(built, tmp_path):
    src = tmp_path / "sz.c"
    items = (["sizeof(hx_band_out)"] + [f"offsetof(hx_band_out,{f})" for f in OUT_FIELDS] + ["sizeof(hx_poa_band_params)"] + [f"offsetof(hx_poa_band_params,{f})" for f in PARAM_FIELDS] +
             ["sizeof(hx_poa_convex_params)", "sizeof(hx_msa_out)", "sizeof(hx_wcns_out)", "sizeof(hx_graph_out)", "sizeof(hx_strand_out)"])
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "haslr_types.h"\nint main(){' +
                   "".join(f'printf("%zu\\n",(size_t){it});' for it in items) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    want = ([C.sizeof(T.BandOut)] + [getattr(T.BandOut, f).offset for f in OUT_FIELDS] + [C.sizeof(T.PoaBandParams)] + [getattr(T.PoaBandParams, f).offset for f in PARAM_FIELDS] +
            [C.sizeof(T.PoaConvexParams), C.sizeof(T.MsaOut), C.sizeof(T.WcnsOut), C.sizeof(T.GraphOut), C.sizeof(T.StrandOut)])
    assert got == want
    assert [n for n, _ in T.BandOut._fields_] == OUT_FIELDS and [n for n, _ in T.PoaBandParams._fields_] == PARAM_FIELDS
    assert got[0] == 120 and got[len(OUT_FIELDS) + 1] == 20
    assert got[-5:] == [28, 96, 80, 192, 144]   # the structs beside them are as they were


def test_entry_points_are_there(built):
    assert hasattr(hip.lib(), "hx_poa_banded") and hasattr(hip.lib(), "hx_free_band")
    assert "hx_poa_banded" in hip.SYMBOLS and "hx_free_band" in hip.SYMBOLS
    assert "poa_modes_slot_kb" in hip.option_names() and "poa_workspace_gb" in hip.option_names()
    assert hip.BandRecord._fields == ("consensus", "band_used", "rows", "coverage", "profile")


def test_the_header_declares_the_entry_as_the_issue_states_it():
    txt = " ".join(open(os.path.join(ROOT, "include", "haslr_hip.h")).read().split())
    assert ("int hx_poa_banded(hx_ctx*, uint32_t n_sets, const uint64_t* set_off, const uint64_t* seq_off, const char* bases, const uint8_t* weights, "
            "const hx_poa_convex_params*, const hx_poa_band_params*, hx_band_out* out);") in txt
    assert "void hx_free_band(hx_ctx*, hx_band_out*);" in txt


def refusal(cp, bp, seqs=("ACGT",), weights=None):
    """the text hx_poa_banded refuses one set with, before it touches its context (none is given)"""
    L = hip.lib()
    bases = "".join(seqs).encode()
    set_off = (C.c_uint64 * 2)(0, len(seqs))
    offs = [0]
    for q in seqs:
        offs.append(offs[-1] + len(q))
    seq_off = (C.c_uint64 * len(offs))(*offs)
    o = T.BandOut()
    rc = L.hx_poa_banded(None, 1, set_off, seq_off, bases, weights, C.byref(cp) if cp else None, C.byref(bp) if bp else None, C.byref(o))
    assert rc == -1 and not o.cns and not o.band_used
    return L.hx_last_error().decode()


def test_every_refusal_names_the_entry_and_the_value(built):
    ok_c, ok_b = T.PoaConvexParams(5, -4, -8, -6, -10, -4, 1), T.PoaBandParams(8, 0, 0, 0, 0)
    assert refusal(None, ok_b) == "hx_poa_banded: no parameters" == refusal(ok_c, None)
    for band in (0, 512, 100000):
        assert refusal(ok_c, T.PoaBandParams(band, 0, 0, 0, 0)) == f"hx_poa_banded: the band half-width must be 1..511, not {band}"
    assert refusal(T.PoaConvexParams(5, -4, 0, 0, -10, -4, 1), ok_b) == "hx_poa_banded: the gap open score must be negative, not 0"
    assert refusal(T.PoaConvexParams(5, -4, -8, 1, -10, -4, 1), ok_b) == "hx_poa_banded: the gap extend score must not be positive, not 1"
    assert refusal(T.PoaConvexParams(5, -4, -8, -9, -10, -4, 1), ok_b).startswith("hx_poa_banded: the gap extend score -9 is below the gap open score -8")
    assert refusal(T.PoaConvexParams(5, -4, -8, -6, -10, -4, 3), ok_b).startswith("hx_poa_banded: unknown alignment type 3")
    assert refusal(T.PoaConvexParams(5, -4, -8, -6, 0, 0, 1), ok_b) == "hx_poa_banded: the second gap open score must be negative, not 0"
    assert refusal(T.PoaConvexParams(5, -4, -8, -6, -10, 2, 1), ok_b) == "hx_poa_banded: the second gap extend score must not be positive, not 2"
    assert refusal(T.PoaConvexParams(5, -4, -8, -6, -10, -11, 1), ok_b).startswith("hx_poa_banded: the second gap extend score -11 is below the second gap open score -10")
    assert refusal(T.PoaConvexParams(5, -4, -8, -6, -7, -4, 1), ok_b).startswith("hx_poa_banded: the second gap open score -7 is above the first gap open score -8")
    assert refusal(ok_c, ok_b, ("AC", "GT"), bytes([1, 1, 1, 0])) == "hx_poa_banded: set 0, sequence 1, position 1: a weight of 0 is not accepted (weights are 1..255)"
    # (the 2^28 bound and the length limits are the plan's: tests/test_poa_band_plan.py)


def test_weights_are_checked_as_poa_weighted_checks_them():
    # (the checks come before the context is touched: no device, no library call)
    call = hip.HipContext.poa_banded
    with pytest.raises(ValueError, match="give weights or qualities, not both"):
        call(None, [["AC"]], 8, weights=[[[1, 1]]], qualities=[["II"]])
    with pytest.raises(ValueError, match="set 0, sequence 0: 1 weights for 2 bases"):
        call(None, [["AC"]], 8, weights=[[[1]]])
    with pytest.raises(ValueError, match="set 0, sequence 0, position 0: the quality character '!' gives 0"):
        call(None, [["AC"]], 8, qualities=[["!I"]])
    with pytest.raises(ValueError, match="unknown alignment type"):
        call(None, [["AC"]], 8, type="global")
    with pytest.raises(ValueError, match="give gap_open2 and gap_extend2, or neither"):
        call(None, [["AC"]], 8, gap_open2=-10)
    with pytest.raises(ValueError, match="band is a half-width in columns, 1..511"):
        call(None, [["AC"]], -1)


@pytest.fixture(scope="module")
def band_caller(built, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("spoa_band") / "spoa_band_caller")
    lib = os.path.join(ROOT, "haslr_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "spoa_band_caller.cpp"), "-o", exe,
                           "-L", lib, "-lhaslr_hip", "-pthread", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def text_of(edges):
    return "\n".join(f"{mode} {band} {' '.join(str(v) for v in sc)}{' +c' if c else ''}\n" + "".join((q or "-") + "\n" for q in st) for mode, band, sc, c, st in edges)


def test_banded_batch_without_a_device_fails_loudly(band_caller):
    import torch
    import bandlib
    r = subprocess.run([band_caller], input=text_of([("nw", 8, bandlib.LINEAR, False, bandlib.ESC_SET)]), capture_output=True, text=True)
    if torch.cuda.is_available():   # (a device is present: the same call works; the test below checks what it prints)
        assert r.returncode == 0 and r.stdout.endswith("=\n"), (r.returncode, r.stderr)
    else:
        assert r.returncode == 1 and "no HIP device" in r.stderr and r.stdout == "", (r.returncode, r.stderr)


@pytest.mark.gpu
def test_banded_batch_prints_the_restatements_answers(band_caller, tmp_path):
    import bandlib
    ref = bandlib.BandRef(str(tmp_path))
    sets = [bandlib.copies(970 + k, 200, 4, 0.06) for k in range(4)] + [bandlib.ESC_SET, ["", "ACGT", "ACGA"], []]
    kinds = [("nw", 8, bandlib.LINEAR, False), ("sw", 8, bandlib.AFFINE, True), ("ov", 20, bandlib.CONVEX, True), ("nw", 8, bandlib.CONVEX, False)]
    edges = [kinds[k % 4] + (st,) for k, st in enumerate(sets)]
    r = subprocess.run([band_caller], input=text_of(edges), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [blk.split("\n")[:-1] for blk in r.stdout.split("=\n")[:-1]]
    want = []
    for mode, band, sc, c, st in edges:
        rec = ref.banded(st, band, mode, sc, include_consensus=c)
        want.append([rec.consensus, str(rec.band_used)] + rec.rows)
    assert got == want and want[4][1] == "32"
