"""The C-ABI, Python and header side of strand-ambiguous sets, without a GPU: the ctypes mirrors of hx_poa_strand_want and hx_strand_out
have the C sizes and offsets, the two entry points are exported and listed, the option that names the one-matrix route is registered, and
HipContext.poa_strand checks its weights before it needs a device."""
import ctypes as C
import os
import subprocess

import pytest

from haslr_amd import ctypes_defs as T
from haslr_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANT_FIELDS = ["want_msa", "include_consensus", "want_coverage", "want_profile"]
OUT_FIELDS = ["n_set", "n_seq", "cns_off", "cns", "reversed", "score_fwd", "score_rev", "n_rows", "n_cols", "msa_off", "msa", "coverage", "profile",
              "dp_cells", "seq_bases", "n_aligned", "third_passes", "slot_reruns"]


def test_struct_sizes_and_offsets_match_c(built, tmp_path):
    src = tmp_path / "sz.c"
    items = (["sizeof(hx_strand_out)"] + [f"offsetof(hx_strand_out,{f})" for f in OUT_FIELDS] + ["sizeof(hx_poa_strand_want)"] + [f"offsetof(hx_poa_strand_want,{f})" for f in WANT_FIELDS] +
             ["sizeof(hx_poa_convex_params)", "sizeof(hx_msa_out)", "sizeof(hx_wcns_out)", "sizeof(hx_graph_out)"])
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "haslr_types.h"\nint main(){' +
                   "".join(f'printf("%zu\\n",(size_t){it});' for it in items) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    want = ([C.sizeof(T.StrandOut)] + [getattr(T.StrandOut, f).offset for f in OUT_FIELDS] + [C.sizeof(T.PoaStrandWant)] + [getattr(T.PoaStrandWant, f).offset for f in WANT_FIELDS] +
            [C.sizeof(T.PoaConvexParams), C.sizeof(T.MsaOut), C.sizeof(T.WcnsOut), C.sizeof(T.GraphOut)])
    assert got == want
    assert [n for n, _ in T.StrandOut._fields_] == OUT_FIELDS and [n for n, _ in T.PoaStrandWant._fields_] == WANT_FIELDS
    assert got[0] == 144 and got[len(OUT_FIELDS) + 1] == 16
    assert got[-4:] == [28, 96, 80, 192]   # the structs beside them are as they were


def test_entry_points_and_the_option_are_there(built):
    assert hasattr(hip.lib(), "hx_poa_strand") and hasattr(hip.lib(), "hx_free_strand")
    assert "hx_poa_strand" in hip.SYMBOLS and "hx_free_strand" in hip.SYMBOLS
    assert "poa_strand_one_h" in hip.option_names() and "poa_modes_slot_kb" in hip.option_names()
    assert hip.StrandRecord._fields == ("consensus", "reversed", "scores", "rows", "coverage", "profile")


def test_the_header_declares_the_entry_as_the_issue_states_it():
    txt = " ".join(open(os.path.join(ROOT, "include", "haslr_hip.h")).read().split())
    assert ("int hx_poa_strand(hx_ctx*, uint32_t n_sets, const uint64_t* set_off, const uint64_t* seq_off, const char* bases, const uint8_t* weights, "
            "const hx_poa_convex_params*, const hx_poa_strand_want*, hx_strand_out* out);") in txt
    assert "void hx_free_strand(hx_ctx*, hx_strand_out*);" in txt


def test_weights_are_checked_as_poa_weighted_checks_them():
    # (the checks come before the context is touched: no device, no library call)
    call = hip.HipContext.poa_strand
    with pytest.raises(ValueError, match="give weights or qualities, not both"):
        call(None, [["AC"]], weights=[[[1, 1]]], qualities=[["II"]])
    with pytest.raises(ValueError, match="set 0, sequence 0: 1 weights for 2 bases"):
        call(None, [["AC"]], weights=[[[1]]])
    with pytest.raises(ValueError, match="set 0, sequence 1, position 1: a weight of 0, which is not accepted"):
        call(None, [["AC", "AC"]], weights=[[[1, 1], [1, 0]]])
    with pytest.raises(ValueError, match="set 0, sequence 0, position 0: the quality character '!' gives 0"):
        call(None, [["AC"]], qualities=[["!I"]])
    with pytest.raises(ValueError, match="unknown alignment type"):
        call(None, [["AC"]], type="global")
    with pytest.raises(ValueError, match="give gap_open2 and gap_extend2, or neither"):
        call(None, [["AC"]], gap_open2=-10)
