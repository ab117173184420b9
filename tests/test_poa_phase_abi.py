"""The C-ABI, Python and header side of two-haplotype consensus, without a GPU: the ctypes mirrors of hx_poa_phase_params and hx_phase_out
have the C sizes and offsets (the first fields hx_label_out's, at its offsets), the out-structs beside them are as they were, the two entry
points are exported and listed, hx_poa_phased refuses bad parameters with its own name and the offending value in front before it touches
a context, HipContext.poa_phased checks its arguments before it needs a device, and spoa::hx::phased_batch goes through a small caller."""
import ctypes as C
import os
import subprocess

import pytest

from haslr_amd import ctypes_defs as T
from haslr_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAM_FIELDS = ["min_count", "min_pct", "want_msa", "include_consensus", "want_coverage", "want_profile"]
LABEL_FIELDS = ["n_set", "n_labels", "cns_off", "cns", "cns_col", "coverage", "profile", "n_rows", "n_cols", "msa_off", "msa", "dp_cells", "seq_bases", "n_aligned", "slot_reruns"]
OUT_FIELDS = LABEL_FIELDS + ["hap", "n_haps", "rounds", "site_off", "site_col", "site_a1", "site_a2", "site_phase"]
OTHERS = ["hx_poa_convex_params", "hx_cns_out", "hx_msa_out", "hx_wcns_out", "hx_graph_out", "hx_strand_out", "hx_band_out", "hx_label_out", "hx_poa_label_params"]


def test_struct_sizes_and_offsets_match_c(built, tmp_path):
    src = tmp_path / "sz.c"
    items = (["sizeof(hx_phase_out)"] + [f"offsetof(hx_phase_out,{f})" for f in OUT_FIELDS] + ["sizeof(hx_poa_phase_params)"] + [f"offsetof(hx_poa_phase_params,{f})" for f in PARAM_FIELDS] +
             [f"offsetof(hx_label_out,{f})" for f in LABEL_FIELDS] + [f"sizeof({s})" for s in OTHERS])
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "haslr_types.h"\nint main(){' +
                   "".join(f'printf("%zu\\n",(size_t){it});' for it in items) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    want = ([C.sizeof(T.PhaseOut)] + [getattr(T.PhaseOut, f).offset for f in OUT_FIELDS] + [C.sizeof(T.PoaPhaseParams)] + [getattr(T.PoaPhaseParams, f).offset for f in PARAM_FIELDS] +
            [getattr(T.LabelOut, f).offset for f in LABEL_FIELDS] +
            [C.sizeof(s) for s in (T.PoaConvexParams, T.CnsOut, T.MsaOut, T.WcnsOut, T.GraphOut, T.StrandOut, T.BandOut, T.LabelOut, T.PoaLabelParams)])
    assert got == want
    assert [n for n, _ in T.PhaseOut._fields_] == OUT_FIELDS and [n for n, _ in T.PoaPhaseParams._fields_] == PARAM_FIELDS
    assert got[0] == 176 and got[len(OUT_FIELDS) + 1] == 24
    nl = len(LABEL_FIELDS)
    assert got[1:1 + nl] == got[-len(OTHERS) - nl:-len(OTHERS)]               # hx_label_out's fields stand at hx_label_out's offsets
    assert got[-len(OTHERS):] == [28, 48, 96, 80, 192, 144, 120, 112, 20]     # the existing structs are as they were


def test_entry_points_are_there(built):
    assert hasattr(hip.lib(), "hx_poa_phased") and hasattr(hip.lib(), "hx_free_phase")
    assert "hx_poa_phased" in hip.SYMBOLS and "hx_free_phase" in hip.SYMBOLS
    assert hip.PhaseRecord._fields == ("hap", "n_haps", "rounds", "sites") + hip.LabelRecord._fields


def test_the_header_declares_the_entry_as_the_issue_states_it():
    txt = " ".join(open(os.path.join(ROOT, "include", "haslr_hip.h")).read().split())
    assert ("int hx_poa_phased(hx_ctx*, uint32_t n_sets, const uint64_t* set_off, const uint64_t* seq_off, const char* bases, const uint8_t* weights, "
            "const hx_poa_convex_params*, const hx_poa_phase_params*, hx_phase_out* out);") in txt
    assert "void hx_free_phase(hx_ctx*, hx_phase_out*);" in txt


def refusal(cp, pp, seqs=("ACGT",), weights=None):
    """the text hx_poa_phased refuses one set with, before it touches its context (none is given)"""
    L = hip.lib()
    bases = "".join(seqs).encode()
    set_off = (C.c_uint64 * 2)(0, len(seqs))
    offs = [0]
    for q in seqs:
        offs.append(offs[-1] + len(q))
    seq_off = (C.c_uint64 * len(offs))(*offs)
    o = T.PhaseOut()
    rc = L.hx_poa_phased(None, 1, set_off, seq_off, bases, weights, C.byref(cp) if cp else None, C.byref(pp) if pp else None, C.byref(o))
    assert rc == -1 and not o.cns and not o.cns_off and not o.hap and not o.site_off
    return L.hx_last_error().decode()


def test_every_refusal_names_the_entry_and_the_value(built):
    ok_c, ok_p = T.PoaConvexParams(5, -4, -8, -6, -10, -4, 1), T.PoaPhaseParams(2, 25, 0, 0, 0, 0)
    assert refusal(None, ok_p) == "hx_poa_phased: no parameters" == refusal(ok_c, None)
    for mc in (0, 256, 100000):
        assert refusal(ok_c, T.PoaPhaseParams(mc, 25, 0, 0, 0, 0)) == f"hx_poa_phased: min_count must be 1..255, not {mc}"
    for mp in (0, 51, 100, 4000000000):
        assert refusal(ok_c, T.PoaPhaseParams(2, mp, 0, 0, 0, 0)) == f"hx_poa_phased: min_pct must be 1..50, not {mp}"
    # hx_poa_graph's own refusals, with this entry's name in front
    assert refusal(T.PoaConvexParams(5, -4, 0, 0, -10, -4, 1), ok_p) == "hx_poa_phased: the gap open score must be negative, not 0"
    assert refusal(T.PoaConvexParams(5, -4, -8, 1, -10, -4, 1), ok_p) == "hx_poa_phased: the gap extend score must not be positive, not 1"
    assert refusal(T.PoaConvexParams(5, -4, -8, -9, -10, -4, 1), ok_p).startswith("hx_poa_phased: the gap extend score -9 is below the gap open score -8")
    assert refusal(T.PoaConvexParams(5, -4, -8, -6, -10, -4, 3), ok_p).startswith("hx_poa_phased: unknown alignment type 3")
    assert refusal(T.PoaConvexParams(5, -4, -8, -6, 0, 0, 1), ok_p) == "hx_poa_phased: the second gap open score must be negative, not 0"
    assert refusal(T.PoaConvexParams(5, -4, -8, -6, -10, 2, 1), ok_p) == "hx_poa_phased: the second gap extend score must not be positive, not 2"
    assert refusal(T.PoaConvexParams(5, -4, -8, -6, -10, -11, 1), ok_p).startswith("hx_poa_phased: the second gap extend score -11 is below the second gap open score -10")
    assert refusal(T.PoaConvexParams(5, -4, -8, -6, -7, -4, 1), ok_p).startswith("hx_poa_phased: the second gap open score -7 is above the first gap open score -8")
    assert refusal(ok_c, ok_p, ("AC", "GT"), bytes([1, 1, 1, 0])) == "hx_poa_phased: set 0, sequence 1, position 1: a weight of 0 is not accepted (weights are 1..255)"


def test_arguments_are_checked_before_a_device_is_needed():
    call = hip.HipContext.poa_phased
    with pytest.raises(ValueError, match="min_count is 1..255, min_pct 1..50"):
        call(None, [["AC"]], min_count=0)
    with pytest.raises(ValueError, match="min_count is 1..255, min_pct 1..50"):
        call(None, [["AC"]], min_count=256)
    with pytest.raises(ValueError, match="min_count is 1..255, min_pct 1..50"):
        call(None, [["AC"]], min_pct=0)
    with pytest.raises(ValueError, match="min_count is 1..255, min_pct 1..50"):
        call(None, [["AC"]], min_pct=51)
    with pytest.raises(ValueError, match="give weights or qualities, not both"):
        call(None, [["AC"]], weights=[[[1, 1]]], qualities=[["II"]])
    with pytest.raises(ValueError, match="set 0, sequence 0: 1 weights for 2 bases"):
        call(None, [["AC"]], weights=[[[1]]])
    with pytest.raises(ValueError, match="unknown alignment type"):
        call(None, [["AC"]], type="global")
    with pytest.raises(ValueError, match="give gap_open2 and gap_extend2, or neither"):
        call(None, [["AC"]], gap_open2=-10)


@pytest.fixture(scope="module")
def phase_caller(built, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("spoa_phase") / "spoa_phase_caller")
    lib = os.path.join(ROOT, "haslr_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "spoa_phase_caller.cpp"), "-o", exe,
                           "-L", lib, "-lhaslr_hip", "-pthread", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def text_of(edges):
    return "\n".join(f"{mode} {mc} {mp} {' '.join(str(v) for v in sc)}\n" + "".join(f"{q or '-'}\n" for q in st) for mode, mc, mp, sc, st in edges)


def test_phased_batch_without_a_device_fails_loudly(phase_caller):
    import torch
    import phaselib
    seqs, mode, mc, mp = phaselib.HAND["snp"]
    r = subprocess.run([phase_caller], input=text_of([(mode, mc, mp, phaselib.LINEAR, seqs)]), capture_output=True, text=True)
    if torch.cuda.is_available():   # (a device is present: the same call works; the test below checks what it prints)
        assert r.returncode == 0 and r.stdout.endswith("=\n"), (r.returncode, r.stderr)
    else:
        assert r.returncode == 1 and "no HIP device" in r.stderr and r.stdout == "", (r.returncode, r.stderr)


@pytest.mark.gpu
def test_phased_batch_prints_the_restatements_answers(phase_caller, tmp_path):
    import phaselib
    ref = phaselib.PhaseRef(str(tmp_path))
    kinds = [phaselib.LINEAR, phaselib.AFFINE, phaselib.CONVEX]
    edges = [(mode, mc, mp, kinds[k % 3], seqs) for k, (seqs, mode, mc, mp) in enumerate(phaselib.HAND.values())] + [("nw", 2, 25, phaselib.AFFINE, [])]
    r = subprocess.run([phase_caller], input=text_of(edges), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [blk.split("\n")[:-1] for blk in r.stdout.split("=\n")[:-1]]
    want = []
    for mode, mc, mp, sc, st in edges:
        rec = ref.phased(st, mode, sc, include_consensus=True, min_count=mc, min_pct=mp)
        want.append([f"{rec.n_haps} {rec.rounds}", " ".join(str(h) for h in rec.hap), " ".join(str(v) for s in rec.sites for v in s)] +
                    [v for g in range(2) for v in (rec.consensus[g], " ".join(str(c) for c in rec.columns[g]))] + rec.rows)
    assert got == want and want[0][:5] == ["2 1", "0 0 0 1 1 1", "2 2 3 1", "AAGAA", "0 1 2 3 4"]
