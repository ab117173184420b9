"""What makes the graph restatement (tests/poa_graph_ref.cpp through grflib) a reference for the general POA path under the score sets of
tests/gscorelib.py, without a GPU: its end scores on chains are those of a plain pairwise DP in Python integers, which cannot wrap; the
premises the GPU tests rest on hold (under the sets without a positive score every kSW alignment is empty, every score set moves the
kNW alignments of a quarter of the corpus away from those under 5 / -4 / -8; the counts are printed); and k x a score set gives the same
graph, paths and pairs with k x the end scores."""
import pytest

import grflib
import gscorelib as gs
from test_poa_convex_ref import gotoh2, short_pairs

PAIRS = short_pairs(137, 300)[::15]   # (every score set, model and type runs them all through the Python DP)
SCALES = (1, 7, 1000)
# the scale test's sets: a tenth of the corpus, as far as 1 000 x the int8 ends stays inside the restatement's own int32
SCALE_CORPUS = [c for c in gs.CORPUS[::10] if (sum(len(q) for q in c[2]) + max(len(q) for q in c[2])) * 128_000 < 1 << 29]


@pytest.fixture(scope="module")
def refs(built, tmp_path_factory):
    return gs.References(grflib.GraphRef(str(tmp_path_factory.mktemp("gscores_ref"))))


def pairwise(a, b, mode, scores):
    """the end score of b against the chain a under the model of the scores: the two-piece recurrences of test_poa_convex_ref.gotoh2, whose
    second piece is the first again under the affine model and whose four gap scores are one under the linear model"""
    m, x, g, e, q, c = scores
    model = grflib.model_of(scores)
    if model == 0:
        return gotoh2(a, b, mode, m, x, g, g, g, g)
    if model == 1:
        return gotoh2(a, b, mode, m, x, g, e, g, e)
    return gotoh2(a, b, mode, m, x, g, e, q, c)


@pytest.mark.parametrize("model", gs.MODELS)
@pytest.mark.parametrize("mode", gs.MODES)
def test_end_scores_on_chains_are_a_plain_pairwise_dp(refs, mode, model):
    assert len(PAIRS) == 20
    for name in gs.NAMES:
        scores = gs.scores_of(name, model)
        got = gs.pmap(lambda p: refs.ref.graph([p[0], p[1]], mode, scores).sequences[1].score, PAIRS)
        assert [k for k, (p, s) in enumerate(zip(PAIRS, got)) if s != pairwise(p[0], p[1], mode, scores)] == [], (name, scores)


@pytest.mark.parametrize("model", gs.MODELS)
def test_without_a_positive_score_every_local_alignment_is_empty(refs, model):
    for name in gs.NOTHING_POSITIVE:
        scores = gs.scores_of(name, model)
        assert max(scores) <= 0
        corpus = gs.corpus_of(name, "sw")
        recs = refs.records(scores, "sw", corpus)
        assert [(f, k) for (f, k, _), r in zip(corpus, recs) if any(sq.alignment or sq.score for sq in r.sequences)] == []
        # ... so nothing is ever joined: a node per base
        assert all(len(r.node_base) == sum(len(q) for q in st) for (_, _, st), r in zip(corpus, recs))
        print(f"{name} {model}: every kSW alignment of {len(corpus)} sets is empty")
    assert len(gs.DISJOINT_CORPUS) >= len(gs.CORPUS) * 3 // 4 and all(c in gs.DISJOINT_CORPUS for c in gs.LONG)


@pytest.mark.parametrize("model", gs.MODELS)
def test_every_score_set_moves_the_global_alignments_of_a_quarter_of_the_corpus(refs, model):
    base = refs.records(gs.DEFAULT[model], "nw")
    for name in gs.NAMES:
        scores = gs.scores_of(name, model)
        recs = refs.records(scores, "nw")
        moved = sum(1 for a, b in zip(recs, base) if [sq.alignment for sq in a.sequences] != [sq.alignment for sq in b.sequences])
        print(f"{name} {model} {scores}: the kNW alignment pairs differ from those under {gs.DEFAULT[model]} on {moved} of {len(gs.CORPUS)} sets")
        assert 4 * moved >= len(gs.CORPUS), (name, model, moved)


@pytest.mark.parametrize("model", gs.MODELS)
@pytest.mark.parametrize("mode", gs.MODES)
def test_k_times_the_scores_give_the_same_graph_with_k_times_the_end_scores(refs, mode, model):
    assert len(SCALE_CORPUS) >= 8
    for name in gs.NAMES:
        scores = gs.scores_of(name, model)
        one = refs.records(scores, mode, SCALE_CORPUS)
        for k in SCALES:
            many = refs.records(gs.scaled(scores, k), mode, SCALE_CORPUS)
            assert grflib.model_of(gs.scaled(scores, k)) == grflib.model_of(scores)
            assert gs.failing(SCALE_CORPUS, many, one, lambda a, b: gs.same_but_scores(a, b, k)) == [], (name, k)

