"""The CPU restatement of per-label consensus over one shared graph (tests/poa_label_ref.cpp) against what is known without it: with every
sequence on label 0 of one it is, field for field, the weighted restatement of the gap model (tests/poa_weighted_ref.cpp for linear and
affine gaps, pcr_weighted of tests/poa_convex_ref.cpp for convex ones); the hand-derived answers of small sets; and the properties a
per-label consensus has by itself on seeded two-haplotype sets."""
import random

import pytest

import cvxlib
import lbllib
import wgtlib
from lbllib import NO_LABEL

MODES = ["sw", "nw", "ov"]
MODEL_NAMES = ["linear", "affine", "convex"]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return lbllib.LabelRef(str(tmp_path_factory.mktemp("label_ref")))


@pytest.fixture(scope="module")
def weighted(tmp_path_factory):
    return wgtlib.WeightedRef(str(tmp_path_factory.mktemp("label_wgt")))


@pytest.fixture(scope="module")
def convex(tmp_path_factory):
    return cvxlib.ConvexRef(str(tmp_path_factory.mktemp("label_cvx")))


def seeded_sets(seed, n=8):
    rnd = random.Random(seed)
    sets = []
    for _ in range(n):
        t = lbllib.template(rnd, rnd.randrange(20, 80))
        sets.append([t] + [lbllib.noisy(rnd, t, rnd.uniform(0.05, 0.3)) or "A" for _ in range(rnd.randrange(1, 6))])
    return sets + [["ACGT", "", "A", "TTTT"], ["A"], [""], []]


def columns_of(row):
    return [c for c, ch in enumerate(row) if ch != "-"]


@pytest.mark.parametrize("model", MODEL_NAMES)
@pytest.mark.parametrize("mode", MODES)
def test_one_label_for_all_is_the_weighted_restatement(ref, weighted, convex, mode, model):
    sc = lbllib.MODELS[model]
    for st in seeded_sets(11):
        for wts in (None, wgtlib.uniform_weights([st], 5)[0]):
            rec = ref.labelled(st, [0] * len(st), 1, mode, sc, weights=wts, include_consensus=True)
            got = (rec.consensus[0], rec.coverage[0], rec.profile[0])
            if model == "convex":
                want = convex.weighted(st, wts, mode, sc)
                assert got == (want.consensus, want.coverage, want.profile)
                if wts is None:   # (the rows do not depend on the weights; the consensus row does)
                    msa = convex.msa(st, mode, sc, include_consensus=True)
                    assert rec.rows == msa.rows and rec.columns[0] == columns_of(msa.rows[-1])
            else:
                want = weighted.weighted(st, wts, mode, sc[0], sc[1], sc[2], sc[3])
                assert want.flags == 0 and want.walked == want.consensus
                assert got == (want.consensus, want.coverage, want.profile) and rec.columns[0] == want.cols
            assert columns_of(rec.rows[-1]) == rec.columns[0] and rec.rows[-1].replace("-", "") == rec.consensus[0]


@pytest.mark.parametrize("model", MODEL_NAMES)
def test_one_mismatch_column(ref, model):
    seqs, labels, nl, mode = lbllib.ONE_MISMATCH
    rec = ref.labelled(seqs, labels, nl, mode, lbllib.MODELS[model], include_consensus=True)
    assert rec.consensus == ["AAGAA", "AATAA"] and rec.columns == [[0, 1, 2, 3, 4]] * 2 and rec.coverage == [[2] * 5] * 2
    assert rec.profile[0][2] == [0, 0, 2, 0] and rec.profile[1][2] == [0, 0, 0, 2]   # (G 2 / T 2, each within its own label)
    assert rec.profile[0][0] == [2, 0, 0, 0] == rec.profile[1][4]
    assert rec.rows == seqs + ["AAGAA", "AATAA"]


@pytest.mark.parametrize("model", MODEL_NAMES)
def test_a_minority_label_keeps_its_own_base(ref, model):
    seqs, labels, nl, mode = lbllib.MINORITY
    rec = ref.labelled(seqs, labels, nl, mode, lbllib.MODELS[model])
    assert rec.consensus == ["AAGAA", "AATAA"] and rec.coverage == [[3] * 5, [1] * 5]
    assert ref.labelled(seqs, [0] * 4, 1, mode, lbllib.MODELS[model]).consensus == ["AAGAA"]   # (the unlabelled consensus)


@pytest.mark.parametrize("model", MODEL_NAMES)
def test_an_insertion_on_one_label(ref, model):
    seqs, labels, nl, mode = lbllib.INSERTION
    rec = ref.labelled(seqs, labels, nl, mode, lbllib.MODELS[model], include_consensus=True)
    assert rec.consensus == ["AACCGGTT", "AACCAGGTT"]
    assert rec.columns == [[0, 1, 2, 3, 5, 6, 7, 8], list(range(9))]   # (label 0 skips the inserted column)
    assert rec.rows == ["AACC-GGTT", "AACCAGGTT"] * 3


@pytest.mark.parametrize("model", MODEL_NAMES)
def test_branch_completion_runs_inside_the_view(ref, model):
    seqs, labels, nl, mode = lbllib.BRANCH
    rec = ref.labelled(seqs, labels, nl, mode, lbllib.MODELS[model], include_consensus=True)
    # the rows show the graph the answer is derived on: Z is a chain of its own into M's first node
    U, Z, M, W = lbllib.BC_U, lbllib.BC_Z, lbllib.BC_M, lbllib.BC_W
    assert rec.rows[:4] == [U + "---" + M + "-" * 6, "-" * 30 + Z + M + "-" * 6, "-" * 30 + Z + M + "-" * 6, U + "---" + M + W]
    # label 0: the edge scores run 1, 3, .. 57 along U (weight 2 each, the first node scores -1), 3, 7 along Z (weight 4), and M's first
    # node takes the heavier edge, from Z: 4 + 7 = 11, then 6 per edge of M: 41 at its end. 57 is the largest and U's last node has an
    # out-edge in the view, so branch completion runs; it kills Z's last node, M's first node then scores 2 + 57, and the walk back from
    # M's last node, a sink of the view though W hangs on it in the whole graph, gives U + M. Stopping at the heaviest node would give U,
    # the heaviest sink without the completion Z + M, and the whole graph's sink U + M + W.
    assert rec.consensus == [U + M, U + M + W]
    assert rec.coverage[0] == [1] * 30 + [3] * 6


@pytest.mark.parametrize("model", MODEL_NAMES)
def test_fallbacks(ref, model):
    seqs, labels, nl, mode = lbllib.ONE_BASE
    rec = ref.labelled(seqs, labels, nl, mode, lbllib.MODELS[model], include_consensus=True)
    # label 1: "G" went to node 2 and "C" to node 1; its view has no edge, so the consensus is its node of smallest id, and a sequence of
    # one base counts in no coverage. Label 2 has no member
    assert rec.consensus == ["ACGT", "C", ""] and rec.columns == [[0, 1, 2, 3], [1], []] and rec.coverage == [[2] * 4, [0], []]
    assert rec.profile[1] == [[0, 0, 0, 0]] and rec.rows == ["ACGT", "ACGT", "--G-", "-C--", "ACGT", "-C--", "----"]
    seqs, labels, nl, mode = lbllib.UNLABELLED
    rec = ref.labelled(seqs, labels, nl, mode, lbllib.MODELS[model], include_consensus=True)
    assert rec.consensus == ["", ""] and rec.columns == [[], []] and rec.coverage == [[], []] and rec.profile == [[], []]
    assert rec.rows == seqs + ["----"] * 2


# ---- properties on seeded two-haplotype sets
def haplotype_sets():
    return [lbllib.two_haplotypes(500 + k, 60 + 13 * k, 3 + k % 3, 0.06) for k in range(6)]


@pytest.mark.parametrize("mode", MODES)
def test_properties_of_a_label_s_consensus(ref, mode):
    for k, (seqs, labels) in enumerate(haplotype_sets()):
        sc = lbllib.MODELS[MODEL_NAMES[k % 3]]
        wts = wgtlib.quality_weights([seqs], 40 + k)[0]
        rec = ref.labelled(seqs, labels, 2, mode, sc, weights=wts, include_consensus=True)
        for g in (0, 1):
            cns, cols = rec.consensus[g], rec.columns[g]
            members = [rec.rows[i] for i, lb in enumerate(labels) if lb == g]
            assert len(cns) == len(cols) > 0 and all(a < b for a, b in zip(cols, cols[1:]))   # the columns rise strictly
            # every consecutive pair of bases is an edge one of the label's members walks
            for i in range(1, len(cns)):
                a, b = cols[i - 1], cols[i]
                assert any(r[a] == cns[i - 1] and r[b] == cns[i] and set(r[a + 1:b]) <= {"-"} for r in members), (k, g, i)
            # coverage and profile are the counts read from the rows of the label's members (all have two or more bases)
            assert rec.profile[g] == [[sum(r[c] == ch for r in members) for ch in "ACGT"] for c in cols]
            assert rec.coverage[g] == [sum(r[c] != "-" for r in members) for c in cols]
            assert columns_of(rec.rows[len(seqs) + g]) == cols and rec.rows[len(seqs) + g].replace("-", "") == cns
        # swapping the labels swaps the outputs
        swapped = ref.labelled(seqs, [1 - lb for lb in labels], 2, mode, sc, weights=wts, include_consensus=True)
        assert swapped.rows[:len(seqs)] == rec.rows[:len(seqs)] and swapped.rows[len(seqs):] == rec.rows[len(seqs):][::-1]
        assert [f[::-1] for f in swapped[:4]] == [list(f) for f in rec[:4]]
        # label 0 does not see the weights of label 1's sequences
        heavy = [[min(255, 5 * v) for v in w] if lb == 1 else w for w, lb in zip(wts, labels)]
        other = ref.labelled(seqs, labels, 2, mode, sc, weights=heavy)
        assert (other.consensus[0], other.columns[0], other.coverage[0]) == (rec.consensus[0], rec.columns[0], rec.coverage[0])
        # a sequence without a label builds the graph like any other
        moved = ref.labelled(seqs, labels[:-1] + [NO_LABEL], 2, mode, sc, weights=wts)
        assert moved.rows == rec.rows[:len(seqs)]


def test_sixteen_labels_and_a_mix(ref):
    seqs, labels = lbllib.two_haplotypes(900, 70, 9, 0.05)
    labels = [(3 * k) % 16 if k % 5 else NO_LABEL for k in range(len(seqs))]
    rec = ref.labelled(seqs, labels, 16, "nw", lbllib.AFFINE, include_consensus=True)
    for g in range(16):
        members = [q for q, lb in zip(seqs, labels) if lb == g]
        assert bool(rec.consensus[g]) == bool(members)
        if len(members) == 1:   # a label of one sequence walks that sequence alone
            assert rec.consensus[g] == members[0] and rec.coverage[g] == [1] * len(members[0])
