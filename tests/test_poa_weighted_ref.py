"""The CPU restatement of base weights and consensus coverage (tests/poa_weighted_ref.cpp), without a GPU: on the 320 seeded sets of
test_poa_modes_ref in three modes, linear and affine, unit weights and one weight on every base give the existing restatements'
consensus, seeded random weights give a coverage and a profile that satisfy what they have to satisfy and that the MSA restatement's rows
(which do not depend on weights) reproduce, the weights do change consensus sequences, and known answers derived by hand pin small
cases: an outvoted base, a one-base member, an empty member, an end of the consensus that the weights move through branch completion, and
the two empty-alignment paths. The Python mirror refuses weights of 0, qualities that give 0 and lengths that do not match before it
reaches the device."""
from concurrent.futures import ThreadPoolExecutor

import pytest

import msalib
import orclib
import parlib
import pmrlib
import wgtlib
from test_poa_modes_ref import SETS

MODES = ["sw", "nw", "ov"]
LINEAR, AFFINE = (5, -4, -8, -8), (5, -4, -8, -2)
WEIGHTINGS = {"uniform": wgtlib.uniform_weights(SETS, 51), "quality": wgtlib.quality_weights(SETS, 52)}


@pytest.fixture(scope="module")
def ref(built, tmp_path_factory):
    return wgtlib.WeightedRef(str(tmp_path_factory.mktemp("pwr")))


@pytest.fixture(scope="module")
def msa(built, tmp_path_factory):
    return msalib.MsaRef(str(tmp_path_factory.mktemp("pwr_pma")))


@pytest.fixture(scope="module")
def lin(built, tmp_path_factory):
    return pmrlib.ModesRef(str(tmp_path_factory.mktemp("pwr_pmr")))


@pytest.fixture(scope="module")
def aff(built, tmp_path_factory):
    return parlib.AffineRef(str(tmp_path_factory.mktemp("pwr_par")))


def pmap(fn, items):
    with ThreadPoolExecutor(16) as ex:   # (the restatements release the GIL: ctypes)
        return list(ex.map(fn, items))


def unit_consensus(lin, aff, mode, scores):
    m, x, g, e = scores
    return pmap((lambda st: lin.consensus(st, mode, m, x, g)) if e == g else (lambda st: aff.consensus(st, mode, m, x, g, e)), SETS)


@pytest.mark.parametrize("scores", [LINEAR, AFFINE])
@pytest.mark.parametrize("mode", MODES)
def test_unit_weights_give_the_existing_restatements_consensus(ref, lin, aff, mode, scores):
    want = unit_consensus(lin, aff, mode, scores)
    none = pmap(lambda st: ref.weighted(st, None, mode, *scores), SETS)
    ones = pmap(lambda st: ref.weighted(st, [[1] * len(q) for q in st], mode, *scores), SETS)
    assert len(none) == 320
    for k, st in enumerate(SETS):
        assert none[k].flags == 0 and ones[k] == none[k], k
        assert none[k].consensus == none[k].walked == want[k], k
        if mode == "nw" and scores == LINEAR:
            assert none[k].consensus == orclib.poa_consensus(st, 5, -4, -8), k


@pytest.mark.parametrize("scores", [LINEAR, AFFINE])
@pytest.mark.parametrize("mode", MODES)
def test_one_weight_on_every_base_gives_the_unit_weight_consensus(ref, mode, scores):
    # edge weights are k times the unit ones and are compared with each other only; scores are k S - 1 or -1 and keep their order
    unit = pmap(lambda st: ref.weighted(st, None, mode, *scores), SETS)
    for k in (2, 7, 100, 255):
        got = pmap(lambda st: ref.weighted(st, [[k] * len(q) for q in st], mode, *scores), SETS)
        for i in range(len(SETS)):
            assert got[i] == unit[i], (k, i)   # (consensus, coverage, profile and columns alike)


def check_coverage(st, r, rows):
    """what coverage and profile of one set have to satisfy, and their agreement with the rows of the MSA of the same set"""
    counted = [k for k, q in enumerate(st) if len(q) >= 2]
    n = len(r.consensus)
    assert r.flags == 0, [t for b, t in wgtlib.FLAGS.items() if r.flags & b]
    assert r.walked == r.consensus
    assert len(r.coverage) == len(r.profile) == len(r.through) == len(r.cols) == n
    assert all(b > a for a, b in zip(r.cols, r.cols[1:]))   # strictly rising
    for i in range(n):
        assert sum(r.profile[i]) == r.coverage[i] <= len(counted)
        own = "ACGT".index(r.consensus[i])
        assert r.profile[i][own] == r.through[i]
        if r.through[i]:
            assert r.profile[i][own] >= 1
        col = [rows[k][r.cols[i]] for k in counted]
        assert r.coverage[i] == sum(ch != "-" for ch in col)
        assert r.profile[i] == [sum("ACGT".find(ch) == q or (q == 0 and ch not in "ACGT-") for ch in col) for q in range(4)]
        assert any(rows[k][r.cols[i]] == r.consensus[i] for k in range(len(st)))   # the column holds the consensus letter


@pytest.mark.parametrize("weighting", sorted(WEIGHTINGS))
@pytest.mark.parametrize("scores", [LINEAR, AFFINE])
@pytest.mark.parametrize("mode", MODES)
def test_coverage_and_profile_under_random_weights(ref, msa, mode, scores, weighting):
    W = WEIGHTINGS[weighting]
    res = pmap(lambda k: ref.weighted(SETS[k], W[k], mode, *scores), range(len(SETS)))
    rows = pmap(lambda st: msa.rows(st, mode, *scores), SETS)
    assert len(res) == 320
    for k, st in enumerate(SETS):
        check_coverage(st, res[k], rows[k])
        if not any(st):
            assert res[k].consensus == "" and res[k].coverage == []


@pytest.mark.parametrize("mode", MODES)
def test_random_weights_change_consensus_sequences(ref, mode):
    # the numbers are recorded in DESIGN.md ("Base weights and coverage"); what is asserted is that the weights act at all
    unit = pmap(lambda st: ref.weighted(st, None, mode, *LINEAR).consensus, SETS)
    for name, W in sorted(WEIGHTINGS.items()):
        got = pmap(lambda k: ref.weighted(SETS[k], W[k], mode, *LINEAR).consensus, range(len(SETS)))
        changed = sum(a != b for a, b in zip(got, unit))
        print(f"{mode} {name}: the consensus of {changed} of {len(SETS)} sets differs from the unit-weight one")
        assert changed > 0, (mode, name)


def test_a_confident_base_outvotes_two_doubtful_ones(ref):
    st = ["AAGAA", "AAGAA", "AATAA"]
    # unit weights: the edges A->G and G->A weigh 4, A->T and T->A weigh 2; the heaviest bundle runs through G
    r = ref.weighted(st)
    assert (r.consensus, r.coverage, r.profile[2]) == ("AAGAA", [3] * 5, [0, 0, 2, 1])
    # weights 1, 1, 10: A->G = 2 + 2 = 4 against A->T = 10 + 10 = 20; every sequence has a base in every column
    r = ref.weighted(st, [[1] * 5, [1] * 5, [10] * 5])
    assert (r.consensus, r.coverage, r.profile[2], r.through) == ("AATAA", [3] * 5, [0, 0, 2, 1], [3, 3, 1, 3, 3])
    # a weight on ONE base counts on both edges at it: the T of the third sequence alone at 10 gives A->T = 1 + 10 = 11
    assert ref.weighted(st, [[1] * 5, [1] * 5, [1, 1, 10, 1, 1]]).consensus == "AATAA"
    # ... and 2 gives A->T = 3 against A->G = 4
    assert ref.weighted(st, [[1] * 5, [1] * 5, [1, 1, 2, 1, 1]]).consensus == "AAGAA"


def test_a_one_base_member_adds_to_no_coverage(ref):
    # the sequence "A" has no edge, so it carries its label nowhere (spoa counts the labels on a node's edges)
    r = ref.weighted(["ACGT", "A", "ACGT"])
    assert (r.consensus, r.coverage) == ("ACGT", [2, 2, 2, 2])
    for st in (["A"], ["A", "A"], ["A", "A", "A"]):
        r = ref.weighted(st)
        assert (r.consensus, r.coverage, r.profile) == ("A", [0], [[0, 0, 0, 0]])   # a coverage of 0 does occur


def test_an_empty_member_and_empty_sets(ref):
    r = ref.weighted(["ACGT", "", "ACT"], [[3] * 4, [], [2] * 3])
    assert (r.consensus, r.coverage, r.profile) == ("ACGT", [2, 2, 1, 2], [[2, 0, 0, 0], [0, 2, 0, 0], [0, 0, 1, 0], [0, 0, 0, 2]])
    for st in ([], [""], ["", ""]):
        r = ref.weighted(st, [[] for _ in st])
        assert (r.consensus, r.coverage, r.profile, r.flags) == ("", [], [], 0)


def test_weights_move_the_end_of_the_consensus_through_branch_completion(ref):
    # kSW. s1 = T^40 + M is a chain; "G" + M + x aligns its M locally, "G" and x become chains of their own: Q -> M[0] and M[5] -> x.
    M = "ACCAGA"
    st = ["T" * 40 + M, "G" + M + "A", "G" + M + "C", "G" + M + "A"]
    # unit weights: P[39] -> M[0] weighs 2, Q -> M[0] 6, the five edges inside M 8, M[5] -> A 4, M[5] -> C 2. Scores: the chain of
    # T gives -1, 1, .., 77 at P[39]; M[0] takes its heavier in-edge, from Q (score -1): 5, then 13 .. 45 at M[5], A 49, C 47. The
    # heaviest node is P[39], not a sink: branch completion marks Q dead and scores on from P[39]: M[0] 79, M[5] 119, A 123, C 121.
    r = ref.weighted(st, None, "sw")
    assert r.consensus == "T" * 40 + M + "A"
    assert r.coverage == [1] * 40 + [4] * 6 + [2] and r.profile[-1] == [2, 0, 0, 0]   # (A and C are chains of their own, not aligned)
    # weight 3 on every base of the third sequence: Q -> M[0] 2 + 6 + 2 = 10, inside M 12, M[5] -> C 6, M[5] -> A still 4. M[0] 9,
    # M[5] 69, C 75, A 73: all below P[39] = 77, so the completion still runs, and now ends in C: M[0] 79, M[5] 139, C 145, A 143.
    r = ref.weighted(st, [[1] * 46, [1] * 8, [3] * 8, [1] * 8], "sw")
    assert r.consensus == "T" * 40 + M + "C"
    assert r.coverage == [1] * 40 + [4] * 6 + [1] and r.profile[-1] == [0, 1, 0, 0]
    # weight 4 there: Q -> M[0] 12, inside M 14, M[5] -> C 8; M[0] 11, M[5] 81, C 89, above P[39] = 77: no completion, the consensus starts at Q
    assert ref.weighted(st, [[1] * 46, [1] * 8, [4] * 8, [1] * 8], "sw").consensus == "G" + M + "C"


def test_the_two_empty_alignment_paths(ref):
    # "C" becomes a chain of its own beside "A" (tests/test_poa_modes_ref.py has the derivation); one-base sequences: coverage 0
    for w in (None, [[9], [200]]):
        r = ref.weighted(["A", "C"], w, "sw")
        assert (r.consensus, r.coverage) == ("A", [0])
        r = ref.weighted(["A", "C"], w, "ov", 5, -20, -1)
        assert (r.consensus, r.coverage) == ("A", [0])
    # with two bases each the chains carry their labels: "AA" and "CC" share nothing under kSW, the heavier chain wins
    r = ref.weighted(["AA", "CC"], [[1, 1], [2, 2]], "sw")
    assert (r.consensus, r.coverage, r.profile) == ("CC", [1, 1], [[0, 1, 0, 0], [0, 1, 0, 0]])


class NoDevice:
    """stands where a HipContext stands: the checks under test happen before anything reaches the device"""
    _h = None

    def _chk(self, rc):
        raise AssertionError("the call reached the library")


def test_the_python_mirror_refuses_bad_weights_before_the_device(built):
    from haslr_amd import hip
    call = lambda *a, **k: hip.HipContext.poa_weighted(NoDevice(), *a, **k)   # noqa: E731
    with pytest.raises(ValueError, match="set 0, sequence 1, position 2: a weight of 0"):
        call([["ACGT", "ACGT"]], weights=[[[1, 1, 1, 1], [1, 1, 0, 1]]])
    with pytest.raises(ValueError, match="position 0: a weight of 256"):
        call([["ACGT"]], weights=[[[256, 1, 1, 1]]])
    with pytest.raises(ValueError, match=r"set 1, sequence 0, position 3: the quality character '!' gives 0"):
        call([["AC"], ["ACGT"]], qualities=[["II"], ["III!"]])
    with pytest.raises(ValueError, match="set 0, sequence 0: 3 weights for 4 bases"):
        call([["ACGT"]], weights=[[[1, 1, 1]]])
    with pytest.raises(ValueError, match="set 0, sequence 0: 5 weights for 4 bases"):
        call([["ACGT"]], qualities=[["IIIII"]])
    with pytest.raises(ValueError, match="set 0: 1 lists of weights for 2 sequences"):
        call([["ACGT", "AC"]], weights=[[[1, 1, 1, 1]]])
    with pytest.raises(ValueError, match="2 sets of weights for 1 sets"):
        call([["ACGT"]], weights=[[[1, 1, 1, 1]], []])
    with pytest.raises(ValueError, match="weights or qualities, not both"):
        call([["AC"]], weights=[[[1, 1]]], qualities=[["II"]])
    with pytest.raises(ValueError, match="unknown alignment type"):
        call([["AC"]], type="xx")
