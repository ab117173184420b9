"""The CPU restatement of strand-ambiguous sets (tests/poa_strand_ref.cpp, DESIGN.md "General POA path", "Strand-ambiguous sets"), without
a GPU: the hand-derived cases of the issue come out as stated, and on seeded sets, in three modes under linear, affine and convex gaps,
with and without weights, what it returns is what the plain restatements (MSA, weighted, graph) return on the same sets with the flagged
sequences reverse-complemented beforehand by the test."""
from concurrent.futures import ThreadPoolExecutor

import pytest

import cvxlib
import grflib
import msalib
import strlib
import wgtlib

MODES = ["sw", "nw", "ov"]
MODELS = {"linear": strlib.LINEAR, "affine": strlib.AFFINE, "convex": strlib.CONVEX}


@pytest.fixture(scope="module")
def ref(built, tmp_path_factory):
    return strlib.StrandRef(str(tmp_path_factory.mktemp("str")))


@pytest.fixture(scope="module")
def msa(built, tmp_path_factory):
    return msalib.MsaRef(str(tmp_path_factory.mktemp("str_msa")))


@pytest.fixture(scope="module")
def cvx(built, tmp_path_factory):
    return cvxlib.ConvexRef(str(tmp_path_factory.mktemp("str_cvx")))


@pytest.fixture(scope="module")
def wgt(built, tmp_path_factory):
    return wgtlib.WeightedRef(str(tmp_path_factory.mktemp("str_wgt")))


@pytest.fixture(scope="module")
def grf(built, tmp_path_factory):
    return grflib.GraphRef(str(tmp_path_factory.mktemp("str_grf")))


def pmap(fn, items, threads=16):
    with ThreadPoolExecutor(threads) as ex:   # (the restatements release the GIL: ctypes)
        return list(ex.map(fn, items))


# ---- the known answers of the issue, authored by hand
def test_known_answer_a_sequence_and_its_reverse_complement(ref):
    s = strlib.S1
    for mode in MODES:
        rec = ref.strand([s, strlib.rc(s)], mode)
        assert rec.reversed == [False, True] and rec.consensus == s and rec.rows == [s, s]
        assert rec.scores[0] == (0, 0) and rec.scores[1][1] == 5 * len(s) > rec.scores[1][0]   # (17 matches against the chain of s)
        assert rec.coverage == [2] * len(s)


def test_known_answer_a_palindrome_ties_and_goes_forward(ref):
    p = strlib.PALINDROME
    assert strlib.rc(p) == p
    for model in MODELS.values():
        rec = ref.strand([p, p], "nw", model)
        assert rec.reversed == [False, False] and rec.scores == [(0, 0), (30, 30)] and rec.consensus == p


def test_known_answer_a_local_alignment_without_a_cell_above_zero(ref):
    # neither CCCC nor its reverse complement GGGG shares a letter with the chain AAAA: 0 against 0, forward, an empty alignment (a chain of its own)
    rec, cells, third = ref.strand_cells(["AAAA", "CCCC"], "sw")
    assert rec.reversed == [False, False] and rec.scores == [(0, 0), (0, 0)] and rec.rows == ["AAAA----", "----CCCC"] and third == 0 and cells == 2 * 4 * 4
    # ... while TTTT reverse-complemented is the chain itself
    rec = ref.strand(["AAAA", "TTTT"], "sw")
    assert rec.reversed == [False, True] and rec.scores == [(0, 0), (0, 20)] and rec.rows == ["AAAA", "AAAA"] and rec.profile == [[2, 0, 0, 0]] * 4


def test_known_answer_reversed_weights_change_the_heaviest_bundle(ref):
    # A (weights 3) and rc(V), V = A with a substitution at 4 and one at 15. The weights of rc(V) are 60 on ITS first half: reversed with the
    # sequence they lie on V's second half, so V's letter wins at 15 (edges of 120 against 6) and A's at 4 (6 against 2)
    a, v = strlib.WA, strlib.WV
    rec = ref.strand([a, strlib.rc(v)], weights=strlib.W_WEIGHTS)
    assert rec.reversed == [False, True] and rec.rows == [a, v]
    assert rec.consensus == a[:15] + v[15] + a[16:] == "ACGTTGCAAGGCTATGCAGG"
    # had the weights stayed as given, V's letter would win at 4 and A's at 15
    assert ref.strand([a, v], weights=strlib.W_WEIGHTS).consensus == a[:4] + v[4] + a[5:] == "ACGTAGCAAGGCTATTCAGG"
    assert ref.strand([a, v], weights=[strlib.W_WEIGHTS[0], strlib.W_WEIGHTS[1][::-1]]).consensus == rec.consensus


def test_known_answer_four_members_on_alternating_strands(ref, cvx):
    for model in MODELS.values():
        rec = ref.strand(strlib.FOUR, "nw", model)
        assert rec.reversed == [False, True, False, True] and rec.consensus == strlib.F0   # (each substitution stands alone against three)
        assert rec.rows == strlib.oriented(strlib.FOUR, rec.reversed)
    assert cvx.consensus(strlib.FOUR, "nw", strlib.CONVEX) == "TCATGGCCTGAATATTCAGGTCAACGA" != strlib.F0   # (aligned as given: the reversed members bend it)


def test_a_letter_that_is_not_acgt_reads_as_a_and_its_complement_is_t(ref):
    assert strlib.rc("ACNGn") == "TCTGT"
    rec = ref.strand(["ACAGATT", "ANTCTGT"])   # (the second is the reverse complement of the first as it is read)
    assert rec.reversed == [False, True] and rec.rows == ["ACAGATT", "ACAGATT"]


def test_empty_members_and_sets(ref):
    rec, cells, third = ref.strand_cells(["", "ACGT", "", "ACGT"], include_consensus=True)
    assert rec.reversed == [False] * 4 and rec.scores == [(0, 0), (0, 0), (0, 0), (20, 20)] and rec.rows == ["----", "ACGT", "----", "ACGT", "ACGT"] and cells == 32
    rec = ref.strand([])
    assert rec.consensus == "" and rec.reversed == [] and rec.scores == [] and rec.rows == [] and rec.coverage == []
    assert ref.strand([""]).rows == [""]


# ---- properties on seeded sets
def plain(msa, cvx, wgt, st, mode, scores, weights):
    """(rows, consensus, coverage, profile) of a set aligned as given, by the restatements that know no strands"""
    if grflib.model_of(scores) == 2:
        w = cvx.weighted(st, weights, mode, scores)
        return cvx.msa(st, mode, scores).rows, w.consensus, w.coverage, w.profile
    w = wgt.weighted(st, weights, mode, *scores[:4])
    return msa.rows(st, mode, *scores[:4]), w.consensus, w.coverage, w.profile


def failing(ref, msa, cvx, wgt, grf, sets, mode, scores, weights=None):
    def one(k):
        st, ws = sets[k], None if weights is None else weights[k]
        rec, cells, third = ref.strand_cells(st, mode, scores, ws)
        bad = []
        pre, pre_w = strlib.oriented(st, rec.reversed), None if ws is None else strlib.oriented_weights(ws, rec.reversed)
        rows, cns, cov, prof = plain(msa, cvx, wgt, pre, mode, scores, pre_w)
        if (rows, cns, cov, prof) != (rec.rows, rec.consensus, rec.coverage, rec.profile):
            bad.append("not what the plain restatements give on the set oriented beforehand")
        again, cells2, third2 = ref.strand_cells(pre, mode, scores, pre_w)
        if any(again.reversed) or third2 or again._replace(scores=None) != rec._replace(scores=None, reversed=[False] * len(st)) or cells2 != cells:
            bad.append("the set oriented beforehand does not come out forward and the same")
        if [f for f, _ in again.scores] != [max(f, r) for f, r in rec.scores]:
            bad.append("the forward score of the oriented set is not the winning score")
        g, gcells, _ = grf.graph_cells(pre, mode, scores, pre_w)
        if [sq.score for sq in g.sequences] != [f for f, _ in again.scores] or 2 * gcells != cells:
            bad.append("score_fwd is not the graph restatement's score")
        if third != sum(rec.reversed) or [r > f for f, r in rec.scores] != rec.reversed:
            bad.append("the flags are not the strict comparison of the scores")
        return (k, bad) if bad else None
    return [b for b in pmap(one, range(len(sets))) if b]


@pytest.mark.parametrize("model", list(MODELS))
@pytest.mark.parametrize("mode", MODES)
def test_the_result_is_the_plain_restatements_on_the_oriented_set(ref, msa, cvx, wgt, grf, mode, model):
    sets = strlib.edge_sets(301) + strlib.tie_sets(302, 30) + [["", "AACGT", "", strlib.rc("AACGA"), "G"], [], [""]]
    assert failing(ref, msa, cvx, wgt, grf, sets, mode, MODELS[model]) == []
    few = strlib.edge_sets(303)[:10] + strlib.tie_sets(304, 10)
    assert failing(ref, msa, cvx, wgt, grf, few, mode, MODELS[model], wgtlib.uniform_weights(few, 305)) == []


def test_the_seeded_sets_hold_reversed_members_and_real_ties(ref):
    recs = [ref.strand(st, "nw") for st in strlib.edge_sets(301)]
    assert sum(sum(r.reversed) for r in recs) >= len(recs)   # (every set has at least its second member on the other strand)
    ties = [(f, r) for st in strlib.tie_sets(302) for mode in MODES for f, r in ref.strand(st, mode).scores if f == r != 0]
    assert len(ties) >= 10
