"""The tuned kNW path (kernels/poa.hip behind hx_poa_sequences) under score triples other than 5 / -4 / -8 (tests/scorelib.py), bit for bit
against the oracle, with the failing (family, set index) pairs reported and the cell count the restatement's. What in that kernel depends on
the scores: the de-ramped keys (X = H - gap x column; the sink scores and the score-matrix flavour's rows put the ramp back), the planner's
gate that switches pruning and column passes off for scores of unusual signs, the pruning threshold with its branch for negative scores,
and the host's check that the keys fit 32 bits.

Every triple runs under the default plan, the pruned row loop and a cluster shape (5 / -4 / 3, the slowest, without the last); the first
triple of every group and (0, -1, -1) under every block size, the score-matrix traceback and the launch shapes of test_poa_hard_gpu.py that
route through score-dependent code. hx_poa_sequences_mode (kNW: the same tuned call) gives the same strings and cells where it takes the
triple, and refuses a gap score that is not negative. Witnesses, from hx_poa_prune_stats: under the pruned row loop a triple of usual signs aligned with a threshold - (0, -1, -1),
whose scores are never positive, among them - and one of unusual signs counted nothing.

The limits of the keys: under 127 / -128 / -128 two copies of the longest sequence whose keys fit come back as they are, a base more is
refused with the rule's name, and two unrelated sequences of 3 000 bases (scores near -400 000) equal the oracle."""
import contextlib
import ctypes as C
import random

import pytest

import orclib
import pmrlib
import scorelib
from scorelib import EXTREME, LEADING, NEGATIVE, TRIPLES, UNUSUAL, corpus_of, failing, sets_of
from test_poa_hard_gpu import SHAPES

pytestmark = pytest.mark.gpu

BLOCKS = [64, 128, 256, 512, 1024]
OPTION_SHAPES = ["cluster_64x8", "cluster_256x2_wide", "cluster_128x4_pruned", "pruned_95", "pruned_108", "passes", "ring_zero", "pruned_ring_1kb", "slots2"]
ALL_SHAPES = ["default"] + ["block_%d" % b for b in BLOCKS] + ["score_matrix"] + OPTION_SHAPES
FEW_SHAPES = ["default", "pruned_95", "cluster_64x8"]
# (5 / -4 / 3: a positive gap score makes every base a node of its own - a call on these sets takes 8 s, so the gate's two shapes only)
SLOW = {(5, -4, 3): ["default", "pruned_95"]}
CASES = [(t, s) for t in TRIPLES for s in (ALL_SHAPES if t in LEADING or t == NEGATIVE else SLOW.get(t, FEW_SHAPES))]


@pytest.fixture(scope="module")
def ctx(built):
    from haslr_amd import hip
    c = hip.HipContext(0)   # raises without a device: these tests never run on a fallback
    yield c
    c.close()


@pytest.fixture(scope="module")
def refs(built, tmp_path_factory):
    """the CPU side, computed once per triple (scorelib.References keeps what it has computed)"""
    return scorelib.References(pmrlib.ModesRef(str(tmp_path_factory.mktemp("scores_gpu_pmr"))))


@contextlib.contextmanager
def launch_shape(ctx, shape):
    if shape == "default":
        yield
    elif shape.startswith("block_"):
        ctx.set_poa_block(int(shape[6:]))
        try:
            yield
        finally:
            ctx.set_poa_block(0)
    elif shape == "score_matrix":   # (the flavour whose rows in HBM are plain scores: the ramp put back)
        ctx.set_poa_traceback(0)
        try:
            yield
        finally:
            ctx.set_poa_traceback(1)
    else:
        with ctx.options(**SHAPES[shape]):
            yield


def tuned(ctx, sets, triple):
    """hx_poa_sequences: (consensus list, counters) - HipContext.poa_sequences with the counters of its output struct"""
    from haslr_amd import ctypes_defs as T
    from haslr_amd import hip
    o, pp = T.CnsOut(), T.PoaParams(*triple)
    ctx._chk(hip.lib().hx_poa_sequences(ctx._h, *hip._flatten_sets(sets), C.byref(pp), C.byref(o)))
    r = T.cns_to_list(o), hip._counters(o)
    hip.lib().hx_free_cns(ctx._h, C.byref(o))
    return r


@pytest.mark.parametrize("triple,shape", CASES, ids=lambda v: v if isinstance(v, str) else "%d_%d_%d" % v)
def test_tuned_path_equals_the_oracle(ctx, refs, triple, shape):
    from haslr_amd import hip
    corpus = corpus_of(triple)
    sets = sets_of(corpus)
    cns, cells = refs.want(triple, corpus)
    with launch_shape(ctx, shape):
        # hx_poa_sequences_mode with kNW and without option poa_general IS hx_poa_sequences with the same arguments (hx_poa.hip), and it returns the counters:
        # under the default plan both entries run, under a launch shape the one that takes the triple and reports the cells - one consensus call per case
        if triple[2] < 0:
            if shape == "default":
                assert failing(corpus, ctx.poa_sequences(sets, *triple), cns) == [], (triple, "hx_poa_sequences")
            got, st = ctx.poa_sequences_mode(sets, "nw", *triple, stats=True)
        else:   # (the entry of the alignment modes takes linear gap PENALTIES only, and says so)
            if shape == "default":
                assert failing(corpus, ctx.poa_sequences(sets, *triple), cns) == [], (triple, "HipContext.poa_sequences")
                with pytest.raises(hip.HipError, match="gap score must be negative"):
                    ctx.poa_sequences_mode(sets, "nw", *triple, stats=True)
            got, st = tuned(ctx, sets, triple)
        pruned = ctx.poa_prune_stats()
        assert failing(corpus, got, cns) == [], (triple, shape)
        assert st["dp_cells"] == cells, (triple, shape)
        assert st["seq_bases"] == sum(len(q) for s in sets for q in s) and st["n_aligned"] == sum(len(s) for s in sets)
    print(triple, shape, "pruning:", pruned)   # (attempts_repeated: for the record)
    if shape == "pruned_95":
        if triple in UNUSUAL:
            assert set(pruned.values()) == {0}, (triple, pruned)   # the gate
        else:
            assert pruned["alignments_with_threshold"] > 0 and pruned["wave_rows"] > 0, (triple, pruned)
    elif triple in UNUSUAL:
        assert set(pruned.values()) == {0}, (triple, shape, pruned)


# ---- the limits of the keys. A cell is 64 x score + 6 bits in an int32, and the planner refuses an edge whose (node estimate + columns + 2) x the largest
# |score| reaches 2^24 (hx_poa_plan.hip, PoaPlanner::size_edges: "DP cells are keys ...")
def node_estimate(lmax, n_seq, sum_len):
    """the planner's first node estimate of an edge (hx_poa_plan.hip, PoaPlanner::size_edges: `est` and `vc`, with the default option poa_node_est_pct and before any growth)"""
    est = max(1, lmax * (120 + 9 * n_seq) // 100 + 1024)
    return max(min(sum_len, est), lmax)


def keys_fit(length, score_abs_max):
    """two sequences of `length` bases: the planner's test, `(vc + E.lmax + 2) * score_abs_max >= 2^24` refuses"""
    return (node_estimate(length, 2, 2 * length) + length + 2) * score_abs_max < 1 << 24


def longest_that_fits(score_abs_max):
    lo, hi = 1, 1 << 20   # (keys_fit is monotone in the length)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if keys_fit(mid, score_abs_max) else (lo, mid)
    return lo


def test_two_copies_of_the_longest_sequence_whose_keys_fit(ctx):
    """a known answer (the oracle's matrix would take about 12 GB): identical sequences align on the diagonal, the graph stays a chain, the consensus is the sequence"""
    n = longest_that_fits(128)
    assert 54000 < n < 55000 and keys_fit(n, 128) and not keys_fit(n + 1, 128)
    assert (1 << 24) - 3 * 128 <= (node_estimate(n, 2, 2 * n) + n + 2) * 128 < 1 << 24   # just under 2^24: a base more adds 2 or 3 to the sum
    rnd = random.Random(7401)
    s = "".join(rnd.choice("ACGT") for _ in range(n))
    assert ctx.poa_sequences([[s, s]], 127, -128, -128) == [s]


def test_a_base_more_is_refused_by_name(ctx):
    from haslr_amd import hip
    n = longest_that_fits(128) + 1
    rnd = random.Random(7402)
    s = "".join(rnd.choice("ACGT") for _ in range(n))
    with pytest.raises(hip.HipError, match="score keys would overflow"):
        ctx.poa_sequences([[s, s]], 127, -128, -128)
    assert ctx.poa_sequences([["ACGT", "ACGT"]], 127, -128, -128) == ["ACGT"]   # (the context serves the next call)


@pytest.mark.parametrize("triple", EXTREME, ids=lambda t: "%d_%d_%d" % t)
def test_unrelated_sequences_under_the_largest_scores(ctx, triple):
    """scores near -400 000 pass through the de-ramp and the sinks' re-ramp"""
    pair = scorelib.UNRELATED_PAIR
    assert len(pair) == 2 and min(len(q) for q in pair) == 3000
    want = orclib.poa_consensus(pair, *triple)
    assert ctx.poa_sequences([pair], *triple) == [want]
    ctx.set_poa_traceback(0)
    try:
        assert ctx.poa_sequences([pair], *triple) == [want], "score-matrix traceback"
    finally:
        ctx.set_poa_traceback(1)
