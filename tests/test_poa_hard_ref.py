"""The structured POA corpus (tests/poasets.py), judged by the CPU restatements alone, and the restatements held to each other on it.

Conditions on the corpus. The statistics of tests/poa_modes_ref.cpp (pmr_last_stats) under kNW with 5 / -4 / -8 say how far the inputs
reach into what the tuned kernel (kernels/poa.hip) has branches for: end-node ties (its local shortcut takes at most 8 candidates and a
closure U of 32 nodes, the sort fallback the rest), nodes with more than 16 in-edges (the direction bytes' limit: the set comes back and
is redone on the score matrix) and rows with more than 4 predecessors (the wide-row pool). Five one-line tie-break mutants of the
restatement (PMR_MUTANT) say whether the inputs tell the tie rules apart. The floors are the issue's; measured:

                                         the 320 random SETS        the corpus (265 sets, 1 092 592 bases)    floor
    alignments with an end-node tie      9                          619                                       200
    most tie candidates                  2                          6 (SLOW_SETS: 12)                         SLOW_SETS > 8
    ties whose closure U > 32 nodes      0                          23 (SLOW_SETS: 167)                       10
    sets with an in-degree above 16      0 (largest in-degree 5)    7 (largest in-degree 31)                  3
    most wide rows in a set              1                          125                                       100
    most sinks met by an alignment       3                          21 (SLOW_SETS: 46)                        -
    consensus changed by a mutant        nw / sw / ov               nw / sw / ov                              5 % = 14 sets
      last best end cell                 1 / 5 / 1                  23 / 58 / 56
      vertical before diagonal           83 / 74 / 77               133 / 82 / 88
      horizontal first                   63 / 56 / 56               137 / 75 / 80
      last matching predecessor          45 / 45 / 45               121 / 69 / 77
      `<` in the heaviest-bundle tie     77 / 74 / 76               80 / 74 / 76

(The 24 two-member sets of the family walk_edges are in these figures and add nothing to them: no tie, in-degree 1, no mutant changes their consensus.
They are there for the shapes of their alignments: test_walk_edges_alignments_have_the_shapes_the_family_is_for.)

Under kSW and kOV (every cell, or every sink row and the last column, is an end candidate) the corpus has 749 and 1 304 tied
alignments, with up to 56 and 52 tied end cells.

The restatements against each other on the corpus: kNW of the linear one is the oracle (whose int16 row kernels run where the scores
fit, so this holds them to the int32 matrix on tie-heavy input); the affine one with gap_extend == gap_open is the linear one in three
modes, alignment for alignment; the weighted one without weights gives the same consensus; the MSA one's rows are the sequences as
read (a c g t are A C G T, any other letter is an A: the reference's table) and its consensus is the linear one."""
from concurrent.futures import ThreadPoolExecutor

import pytest

import msalib
import orclib
import parlib
import pmrlib
import poasets
import wgtlib
from test_poa_modes_ref import TRIPLES

MODES = ["sw", "nw", "ov"]
CORPUS, SLOW_SETS = poasets.CORPUS, poasets.SLOW_SETS
THIRD = poasets.sub_sample(3)   # what the score sets other than the default run on


def pmap(fn, items):
    with ThreadPoolExecutor(16) as ex:   # (the restatements release the GIL: ctypes)
        return list(ex.map(fn, items))


def failing(corpus, got, want):
    """the (family, index) pairs of the sets whose results differ"""
    return [(f, k) for (f, k, _), a, b in zip(corpus, got, want) if a != b]


@pytest.fixture(scope="module")
def lin(built, tmp_path_factory):
    return pmrlib.ModesRef(str(tmp_path_factory.mktemp("hard_pmr")))


@pytest.fixture(scope="module")
def linear_results(lin):
    """{(mode, triple, whole corpus?): [(consensus, cells, statistics) per set]}, computed once"""
    cache = {}

    def get(mode, triple=TRIPLES[0], whole=True):
        key = (mode, triple, whole)
        if key not in cache:
            cache[key] = pmap(lambda c: lin.consensus_stats(c[2], mode, *triple), CORPUS if whole else THIRD)
        return cache[key]
    return get


def test_the_corpus_is_what_it_says():
    assert sorted(poasets.FAMILIES) == ["fan_in", "fragments", "haplotypes", "homopolymers", "many_members", "other_letters", "prefix_mismatch", "tandem_repeats",
                                        "two_letters", "unrelated", "walk_edges"]
    assert list(poasets.FAMILIES)[-1] == "walk_edges" and CORPUS[-1][0] == "walk_edges"   # appended last: the other families keep their places
    assert 200 <= len(CORPUS) <= 400 and len({f for f, _, _ in THIRD}) == 11
    assert sum(len(q) for _, _, st in CORPUS for q in st) < 1_200_000
    assert all(st and all(1 <= len(q) <= 1200 for q in st) for _, _, st in CORPUS + [("slow", k, s) for k, s in enumerate(SLOW_SETS)])
    assert min(len(q) for _, _, st in CORPUS for q in st) <= 3 and max(len(q) for _, _, st in CORPUS for q in st) >= 700
    assert max(len(st) for st in poasets.FAMILIES["fan_in"]) >= 150 and min(len(st) for st in poasets.FAMILIES["fan_in"]) >= 150
    assert 100 <= min(len(st) for st in poasets.FAMILIES["many_members"]) and max(len(st) for st in poasets.FAMILIES["many_members"]) == 400
    for half in poasets.FAMILIES["haplotypes"]:
        assert len(half) % 2 == 0
    for st in poasets.FAMILIES["fragments"]:
        assert [len(q) for q in st] == sorted(len(q) for q in st)
    t = poasets.FAMILIES["prefix_mismatch"][0]
    assert len(t[0]) == 300 and len(t) == 298 and all(q[:-1] == t[0][:len(q) - 1] and q[-1] != t[0][len(q) - 1] for q in t[1:])
    assert len(poasets.FAMILIES["prefix_mismatch"][1]) == 1 + 3 * 297 and len(SLOW_SETS) == 1 and len(SLOW_SETS[0][0]) == 1200
    assert any(c not in "ACGT" for st in poasets.FAMILIES["other_letters"] for q in st for c in q)
    assert poasets._build() == poasets.FAMILIES   # seeded: the same sets every time


def test_the_corpus_reaches_ties_in_degrees_and_wide_rows(linear_results, lin):
    st = [r[2] for r in linear_results("nw")]
    print("corpus, kNW 5/-4/-8:", {k: (sum if k in ("tied", "ties_above_8", "closure_above_32") else max)(s[k] for s in st) for k in pmrlib.STATS},
          "sets with an in-degree above 16:", sum(s["max_in_degree"] > 16 for s in st))
    assert sum(s["tied"] for s in st) >= 200
    assert sum(s["closure_above_32"] for s in st) >= 10
    assert sum(s["max_in_degree"] > 16 for s in st) >= 3
    assert max(s["wide_rows"] for s in st) >= 100
    slow = [lin.consensus_stats(s, "nw")[2] for s in SLOW_SETS]
    print("SLOW_SETS:", slow)
    assert sum(s["ties_above_8"] for s in slow) >= 1 and max(s["max_candidates"] for s in slow) > 8


def test_walk_edges_alignments_have_the_shapes_the_family_is_for(lin):
    """kNW 5 / -4 / -8: the second member of every walk_edges set aligns to the chain of the first (nodes 0 .. n - 1) exactly as the family says -
    n pairs to the origin; two leading insertions; two leading nodes without a base; two trailing insertions - at every n around 64 and 128"""
    sets = poasets.FAMILIES["walk_edges"]
    assert len(sets) == 4 * len(poasets.WALK_EDGE_LENGTHS)
    for k, n in enumerate(poasets.WALK_EDGE_LENGTHS):
        same, lead, cut, trail = sets[4 * k:4 * k + 4]
        t = same[0]
        assert len(t) == n and t[0] == "A" and t[-1] in "AT" and all(st[0] == t and len(st) == 2 for st in (same, lead, cut, trail))
        assert same[1] == t and lead[1] == "CG" + t and cut[1] == t[2:] and trail[1] == t + "CG"
        diag = [(i, i) for i in range(n)]
        for st, want in ((same, diag),
                         (lead, [(-1, 0), (-1, 1)] + [(i, i + 2) for i in range(n)]),
                         (cut, [(0, -1), (1, -1)] + [(i, i - 2) for i in range(2, n)]),
                         (trail, diag + [(-1, n), (-1, n + 1)])):
            lin.consensus(st, "nw")
            assert lin.last_alignment() == want, (n, st[1][:4])


@pytest.mark.parametrize("mutant", sorted(pmrlib.MUTANTS))
def test_every_tie_break_mutant_changes_the_consensus_of_the_corpus(linear_results, mutant, built, tmp_path):
    mut = pmrlib.ModesRef(str(tmp_path), mutant=mutant)
    for mode in MODES:
        want = [r[0] for r in linear_results(mode)]
        got = pmap(lambda c: mut.consensus(c[2], mode), CORPUS)
        changed = len(failing(CORPUS, got, want))
        print(mutant, mode, changed, "of", len(CORPUS))
        assert 20 * changed >= len(CORPUS), (mutant, mode, changed)


def oracle(st, m=5, x=-4, g=-8):
    """the oracle's consensus of a set as read (its string entry, a test helper, knows upper-case ACGT only)"""
    return orclib.poa_consensus([poasets.as_read(q) for q in st], m, x, g)


def test_lower_case_is_upper_case_and_other_letters_are_a(lin):
    # the reference's table (Compressed_sequence.cpp:10-19, "& 3"): a c g t are A C G T, everything else is an A
    assert poasets.as_read("acgtNxACGT-*") == "ACGTAAACGTAA"
    sets = [["ACGT", "NCGT", "acgt"], ["acgtn", "RYKMS"], ["GGNGG", "GGAGG", "GGcGG"], ["ttTTgG"] * 2]
    for st in sets:
        read = [poasets.as_read(q) for q in st]
        for mode in MODES:
            assert lin.consensus(st, mode) == lin.consensus(read, mode)
    for mode in MODES:
        assert lin.consensus(["acgtn"], mode) == "ACGTA" and lin.consensus(["RYKMS-*"], mode) == "AAAAAAA"
        assert lin.consensus(sets[0], mode) == "ACGT" and lin.consensus(sets[2], mode) == "GGAGG" and lin.consensus(sets[3], mode) == "TTTTGG"


@pytest.mark.parametrize("triple", TRIPLES)
def test_nw_is_the_oracle_on_the_corpus(linear_results, lin, triple):
    whole = triple == TRIPLES[0]
    corpus = CORPUS if whole else THIRD
    got = [r[0] for r in linear_results("nw", triple, whole)]
    want = pmap(lambda c: oracle(c[2], *triple), corpus)
    assert failing(corpus, got, want) == [], triple
    if whole:
        for k, st in enumerate(SLOW_SETS):
            assert lin.consensus(st, "nw") == oracle(st), ("slow", k)


@pytest.mark.parametrize("mode", MODES)
def test_affine_with_equal_scores_is_the_linear_restatement_on_the_corpus(linear_results, mode, built, tmp_path):
    aff = parlib.AffineRef(str(tmp_path))
    for triple in TRIPLES:
        whole = triple == TRIPLES[0]
        corpus = CORPUS if whole else THIRD
        want = [r[:2] for r in linear_results(mode, triple, whole)]
        got = pmap(lambda c: aff.consensus_cells(c[2], mode, *triple, triple[2]), corpus)
        assert failing(corpus, got, want) == [], (mode, triple)


@pytest.mark.parametrize("mode", MODES)
def test_weighted_without_weights_is_the_linear_consensus_on_the_corpus(linear_results, mode, built, tmp_path):
    ref = wgtlib.WeightedRef(str(tmp_path))
    for triple in TRIPLES[:2]:
        whole = triple == TRIPLES[0]
        corpus = CORPUS if whole else THIRD
        want = [r[0] for r in linear_results(mode, triple, whole)]
        got = pmap(lambda c: ref.weighted(c[2], None, mode, *triple, triple[2]), corpus)
        assert [(f, k) for (f, k, _), r in zip(corpus, got) if r.flags] == []
        assert failing(corpus, [r.consensus for r in got], want) == [], (mode, triple)
        assert failing(corpus, [r.walked for r in got], want) == [], (mode, triple)


@pytest.mark.parametrize("mode", MODES)
def test_msa_rows_are_the_sequences_as_read_on_the_corpus(linear_results, mode, built, tmp_path):
    ref = msalib.MsaRef(str(tmp_path))
    for triple in TRIPLES[:2]:
        whole = triple == TRIPLES[0]
        corpus = CORPUS if whole else THIRD
        want = [r[0] for r in linear_results(mode, triple, whole)]
        got = pmap(lambda c: ref.msa(c[2], mode, *triple, triple[2], True), corpus)
        assert [(f, k) for (f, k, _), r in zip(corpus, got) if r.flags] == []
        assert failing(corpus, [r.consensus for r in got], want) == [], (mode, triple)
        assert failing(corpus, [r.walked for r in got], want) == [], (mode, triple)
        for (f, k, st), r in zip(corpus, got):
            assert len(r.rows) == len(st) + 1 and all(len(row) == r.n_cols for row in r.rows), (f, k)
            assert [row.replace("-", "") for row in r.rows] == [poasets.as_read(q) for q in st] + [r.consensus], (f, k)
