"""The C-ABI, Python and header side of per-label consensus, without a GPU: the ctypes mirrors of hx_poa_label_params and hx_label_out have
the C sizes and offsets, the out-structs beside them are as they were, the two entry points are exported and listed, hx_poa_labelled
refuses bad parameters with its own name and the offending value in front before it touches a context, and HipContext.poa_labelled
checks its labels and weights before it needs a device."""
import ctypes as C
import os
import subprocess

import pytest

from haslr_amd import ctypes_defs as T
from haslr_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAM_FIELDS = ["n_labels", "want_msa", "include_consensus", "want_coverage", "want_profile"]
OUT_FIELDS = ["n_set", "n_labels", "cns_off", "cns", "cns_col", "coverage", "profile", "n_rows", "n_cols", "msa_off", "msa", "dp_cells", "seq_bases", "n_aligned", "slot_reruns"]


def test_struct_sizes_and_offsets_match_c(built, tmp_path):
    src = tmp_path / "sz.c"
    items = (["sizeof(hx_label_out)"] + [f"offsetof(hx_label_out,{f})" for f in OUT_FIELDS] + ["sizeof(hx_poa_label_params)"] + [f"offsetof(hx_poa_label_params,{f})" for f in PARAM_FIELDS] +
             ["sizeof(hx_poa_convex_params)", "sizeof(hx_cns_out)", "sizeof(hx_msa_out)", "sizeof(hx_wcns_out)", "sizeof(hx_graph_out)", "sizeof(hx_strand_out)", "sizeof(hx_band_out)"])
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "haslr_types.h"\nint main(){' +
                   "".join(f'printf("%zu\\n",(size_t){it});' for it in items) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    want = ([C.sizeof(T.LabelOut)] + [getattr(T.LabelOut, f).offset for f in OUT_FIELDS] + [C.sizeof(T.PoaLabelParams)] + [getattr(T.PoaLabelParams, f).offset for f in PARAM_FIELDS] +
            [C.sizeof(T.PoaConvexParams), C.sizeof(T.CnsOut), C.sizeof(T.MsaOut), C.sizeof(T.WcnsOut), C.sizeof(T.GraphOut), C.sizeof(T.StrandOut), C.sizeof(T.BandOut)])
    assert got == want
    assert [n for n, _ in T.LabelOut._fields_] == OUT_FIELDS and [n for n, _ in T.PoaLabelParams._fields_] == PARAM_FIELDS
    assert got[0] == 112 and got[len(OUT_FIELDS) + 1] == 20
    assert got[-7:-6] == [28] and got[-5:] == [96, 80, 192, 144, 120]   # the existing out-structs are as they were


def test_entry_points_are_there(built):
    assert hasattr(hip.lib(), "hx_poa_labelled") and hasattr(hip.lib(), "hx_free_label")
    assert "hx_poa_labelled" in hip.SYMBOLS and "hx_free_label" in hip.SYMBOLS
    assert hip.LabelRecord._fields == ("consensus", "columns", "coverage", "profile", "rows") and hip.NO_LABEL == 255


def test_the_header_declares_the_entry_as_the_issue_states_it():
    txt = " ".join(open(os.path.join(ROOT, "include", "haslr_hip.h")).read().split())
    assert ("int hx_poa_labelled(hx_ctx*, uint32_t n_sets, const uint64_t* set_off, const uint64_t* seq_off, const char* bases, const uint8_t* weights, const uint8_t* labels, "
            "const hx_poa_convex_params*, const hx_poa_label_params*, hx_label_out* out);") in txt
    assert "void hx_free_label(hx_ctx*, hx_label_out*);" in txt


def refusal(cp, lp, seqs=("ACGT",), labels=(0,), weights=None):
    """the text hx_poa_labelled refuses one set with, before it touches its context (none is given)"""
    L = hip.lib()
    bases = "".join(seqs).encode()
    set_off = (C.c_uint64 * 2)(0, len(seqs))
    offs = [0]
    for q in seqs:
        offs.append(offs[-1] + len(q))
    seq_off = (C.c_uint64 * len(offs))(*offs)
    o = T.LabelOut()
    rc = L.hx_poa_labelled(None, 1, set_off, seq_off, bases, weights, None if labels is None else bytes(labels) + b"\0", C.byref(cp) if cp else None, C.byref(lp) if lp else None, C.byref(o))
    assert rc == -1 and not o.cns and not o.cns_off and not o.cns_col
    return L.hx_last_error().decode()


def test_every_refusal_names_the_entry_and_the_value(built):
    ok_c, ok_l = T.PoaConvexParams(5, -4, -8, -6, -10, -4, 1), T.PoaLabelParams(2, 0, 0, 0, 0)
    assert refusal(None, ok_l) == "hx_poa_labelled: no parameters" == refusal(ok_c, None)
    for nl in (0, 17, 255, 100000):
        assert refusal(ok_c, T.PoaLabelParams(nl, 0, 0, 0, 0)) == f"hx_poa_labelled: n_labels must be 1..16, not {nl}"
    assert refusal(ok_c, ok_l, labels=None) == "hx_poa_labelled: no labels"
    assert refusal(ok_c, ok_l, ("AC", "GT", "A"), (1, 255, 2)) == "hx_poa_labelled: set 0, sequence 2: label 2 is not below n_labels = 2 and not 255 (no label)"
    assert refusal(ok_c, T.PoaLabelParams(16, 0, 0, 0, 0), ("AC", "GT"), (15, 16)) == "hx_poa_labelled: set 0, sequence 1: label 16 is not below n_labels = 16 and not 255 (no label)"
    assert refusal(ok_c, T.PoaLabelParams(1, 0, 0, 0, 0), ("AC",), (254,)) == "hx_poa_labelled: set 0, sequence 0: label 254 is not below n_labels = 1 and not 255 (no label)"
    # hx_poa_graph's own refusals, with this entry's name in front
    assert refusal(T.PoaConvexParams(5, -4, 0, 0, -10, -4, 1), ok_l) == "hx_poa_labelled: the gap open score must be negative, not 0"
    assert refusal(T.PoaConvexParams(5, -4, -8, 1, -10, -4, 1), ok_l) == "hx_poa_labelled: the gap extend score must not be positive, not 1"
    assert refusal(T.PoaConvexParams(5, -4, -8, -9, -10, -4, 1), ok_l).startswith("hx_poa_labelled: the gap extend score -9 is below the gap open score -8")
    assert refusal(T.PoaConvexParams(5, -4, -8, -6, -10, -4, 3), ok_l).startswith("hx_poa_labelled: unknown alignment type 3")
    assert refusal(T.PoaConvexParams(5, -4, -8, -6, 0, 0, 1), ok_l) == "hx_poa_labelled: the second gap open score must be negative, not 0"
    assert refusal(T.PoaConvexParams(5, -4, -8, -6, -10, 2, 1), ok_l) == "hx_poa_labelled: the second gap extend score must not be positive, not 2"
    assert refusal(T.PoaConvexParams(5, -4, -8, -6, -10, -11, 1), ok_l).startswith("hx_poa_labelled: the second gap extend score -11 is below the second gap open score -10")
    assert refusal(T.PoaConvexParams(5, -4, -8, -6, -7, -4, 1), ok_l).startswith("hx_poa_labelled: the second gap open score -7 is above the first gap open score -8")
    assert refusal(ok_c, ok_l, ("AC", "GT"), (0, 1), bytes([1, 1, 1, 0])) == "hx_poa_labelled: set 0, sequence 1, position 1: a weight of 0 is not accepted (weights are 1..255)"


def test_labels_and_weights_are_checked_before_a_device_is_needed():
    call = hip.HipContext.poa_labelled
    with pytest.raises(ValueError, match="labels must be nested like sets: one per sequence"):
        call(None, [["AC", "GT"]], [[0]], 2)
    with pytest.raises(ValueError, match="labels must be nested like sets: one per sequence"):
        call(None, [["AC"], ["GT"]], [[0]], 2)
    with pytest.raises(ValueError, match=r"a label is 0 .. n_labels - 1 or 255 \(no label\), n_labels 1..16"):
        call(None, [["AC"]], [[256]], 2)
    with pytest.raises(ValueError, match=r"a label is 0 .. n_labels - 1 or 255 \(no label\), n_labels 1..16"):
        call(None, [["AC"]], [[0]], -1)
    with pytest.raises(ValueError, match="give weights or qualities, not both"):
        call(None, [["AC"]], [[0]], 1, weights=[[[1, 1]]], qualities=[["II"]])
    with pytest.raises(ValueError, match="set 0, sequence 0: 1 weights for 2 bases"):
        call(None, [["AC"]], [[0]], 1, weights=[[[1]]])
    with pytest.raises(ValueError, match="unknown alignment type"):
        call(None, [["AC"]], [[0]], 1, type="global")
    with pytest.raises(ValueError, match="give gap_open2 and gap_extend2, or neither"):
        call(None, [["AC"]], [[0]], 1, gap_open2=-10)


@pytest.fixture(scope="module")
def label_caller(built, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("spoa_label") / "spoa_label_caller")
    lib = os.path.join(ROOT, "haslr_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "spoa_label_caller.cpp"), "-o", exe,
                           "-L", lib, "-lhaslr_hip", "-pthread", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def text_of(edges):
    return "\n".join(f"{mode} {nl} {' '.join(str(v) for v in sc)}\n" + "".join(f"{lb} {q or '-'}\n" for q, lb in zip(st, lbs)) for mode, nl, sc, st, lbs in edges)


def test_labelled_batch_without_a_device_fails_loudly(label_caller):
    import torch
    import lbllib
    seqs, labels, nl, mode = lbllib.ONE_MISMATCH
    r = subprocess.run([label_caller], input=text_of([(mode, nl, lbllib.LINEAR, seqs, labels)]), capture_output=True, text=True)
    if torch.cuda.is_available():   # (a device is present: the same call works; the test below checks what it prints)
        assert r.returncode == 0 and r.stdout.endswith("=\n"), (r.returncode, r.stderr)
    else:
        assert r.returncode == 1 and "no HIP device" in r.stderr and r.stdout == "", (r.returncode, r.stderr)


@pytest.mark.gpu
def test_labelled_batch_prints_the_restatements_answers(label_caller, tmp_path):
    import lbllib
    ref = lbllib.LabelRef(str(tmp_path))
    kinds = [lbllib.LINEAR, lbllib.AFFINE, lbllib.CONVEX]
    edges = [(mode, 3, kinds[k % 3], seqs, labels) for k, (seqs, labels, _, mode) in enumerate(lbllib.HAND.values())] + [("nw", 3, lbllib.AFFINE, [], [])]
    r = subprocess.run([label_caller], input=text_of(edges), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [blk.split("\n")[:-1] for blk in r.stdout.split("=\n")[:-1]]
    want = []
    for mode, nl, sc, st, lbs in edges:
        rec = ref.labelled(st, lbs, nl, mode, sc, include_consensus=True)
        want.append([v for g in range(nl) for v in (rec.consensus[g], " ".join(str(c) for c in rec.columns[g]))] + rec.rows)
    assert got == want and want[0][0] == "AAGAA" and want[0][2] == "AATAA"
