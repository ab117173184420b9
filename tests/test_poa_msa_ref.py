"""The CPU restatement of the multiple sequence alignment (tests/poa_msa_ref.cpp), without a GPU: on the 320 seeded sets of
test_poa_modes_ref in three modes, linear and affine, the node derivation, the columns and the rows satisfy what an MSA has to satisfy
(conditions, not measurements: no set is skipped), and known answers pin the rows of small cases, the empty-sequence rule and the
two empty-alignment paths."""
from concurrent.futures import ThreadPoolExecutor

import pytest

import msalib
import parlib
import pmrlib
from test_poa_modes_ref import SETS

MODES = ["sw", "nw", "ov"]
LINEAR, AFFINE = (5, -4, -8, -8), (5, -4, -8, -2)


@pytest.fixture(scope="module")
def ref(built, tmp_path_factory):
    return msalib.MsaRef(str(tmp_path_factory.mktemp("pma")))


@pytest.fixture(scope="module")
def lin(built, tmp_path_factory):
    return pmrlib.ModesRef(str(tmp_path_factory.mktemp("pma_pmr")))


@pytest.fixture(scope="module")
def aff(built, tmp_path_factory):
    return parlib.AffineRef(str(tmp_path_factory.mktemp("pma_par")))


def check_rows(seqs, rows, n_cols, consensus=None):
    """what the rows of an MSA have to satisfy, whoever made them; rows = one per sequence (+ the consensus row when consensus is given)"""
    assert len(rows) == len(seqs) + (consensus is not None)
    members = list(seqs) + ([consensus] if consensus is not None else [])
    for row, s in zip(rows, members):
        assert len(row) == n_cols
        assert row.replace("-", "") == s   # (with the row's length this is also "columns rise strictly": the bases stand in order, one per column)
        assert set(row) <= set("ACGT-")
    if any(seqs):
        assert n_cols > 0
        for c in range(n_cols):   # no column is all gaps (the sequences alone fill every column: each node holds a base of one of them)
            assert any(row[c] != "-" for row in rows[:len(seqs)]), c
    else:
        assert n_cols == 0


@pytest.mark.parametrize("scores", [LINEAR, AFFINE])
@pytest.mark.parametrize("mode", MODES)
def test_invariants_on_the_seeded_sets(ref, lin, aff, mode, scores):
    m, x, g, e = scores
    with ThreadPoolExecutor(16) as ex:   # (the restatements release the GIL: ctypes)
        res = list(ex.map(lambda st: ref.msa(st, mode, m, x, g, e, True), SETS))
        want = list(ex.map((lambda st: lin.consensus(st, mode, m, x, g)) if e == g else (lambda st: aff.consensus(st, mode, m, x, g, e)), SETS))
    assert len(res) == len(SETS) == 320
    for k, (st, r) in enumerate(zip(SETS, res)):
        assert r.flags == 0, (k, [t for b, t in msalib.FLAGS.items() if r.flags & b])
        assert r.walked == r.consensus == want[k], k
        check_rows(st, r.rows, r.n_cols, want[k])
        assert ref.rows(st, mode, m, x, g, e) == r.rows[:-1], k   # (without the consensus row: the same rows)


def test_known_answers_nw(ref):
    assert ref.rows(["ACGT", "AGT"]) == ["ACGT", "A-GT"]
    r = ref.msa(["ACGT", "ATGT"])
    assert (r.rows, r.n_cols, r.consensus) == (["ACGT", "ATGT"], 4, "ATGT")   # C and T share a column
    r = ref.msa(["ACGT", "ACAGT"])
    assert (r.rows, r.consensus) == (["AC-GT", "ACAGT"], "ACAGT")
    st = ["ACGT", "ATGT", "AGGT", "ACGT"]
    r = ref.msa(st)
    assert (r.rows, r.n_cols, r.consensus) == (st, 4, "ACGT")
    assert ref.msa(["ACGT", "AGT"]).consensus == "ACGT"
    assert ref.rows(["ACGTACGGTCA", "CGGTCATTGAC"]) == ["ACGT-ACGGTCA", "CGGTCATTGAC-"]


def test_an_empty_member_is_a_row_of_gaps_and_an_empty_set_has_no_column(ref):
    assert ref.rows(["ACGT", "", "ACT"]) == ["ACGT", "----", "AC-T"]
    for st in ([], [""], ["", ""]):
        r = ref.msa(st, include_consensus=True)
        assert (r.n_cols, r.rows, r.consensus) == (0, [""] * (len(st) + 1), "")


def test_the_two_empty_alignment_paths(ref):
    r = ref.msa(["A", "C"], "sw")
    assert (r.rows, r.consensus) == (["A-", "-C"], "A")
    r = ref.msa(["A", "C"], "ov", 5, -20, -1)
    assert (r.rows, r.consensus) == (["A-", "-C"], "A")


def test_known_answers_ov_and_sw(ref):
    st = ["ACGTACGGTCA", "CGGTCATTGAC", "TTGACCA"]
    r = ref.msa(st, "ov", include_consensus=True)
    assert r.rows[:3] == ["ACGTACGGTCA-------", "-----CGGTCATTGAC--", "-----------TTGACCA"]
    assert r.consensus == "ACGTACGGTCATTGACCA" and r.rows[3] == r.consensus   # the consensus row has no gap
    assert ref.rows(["TTTTACGTACGGTCA", "ACGTACGGTCAGGGG"], "sw") == ["TTTTACGTACGGTCA----", "----ACGTACGGTCAGGGG"]
    assert ref.rows(["ACGT", "AGT"], include_consensus=True)[2] == "ACGT"


def test_affine_gaps_move_a_base_across_the_gap(ref):
    st = ["ACGTTTACGGACCA", "ACGTACCA"]
    assert ref.rows(st)[1] == "ACG--T----ACCA"
    assert ref.rows(st, "nw", 5, -4, -8, -2)[1] == "ACGT------ACCA"
