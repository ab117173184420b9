"""The POA kernels on the structured corpus (tests/poasets.py: tie-heavy, high fan-in and many-member sets), bit for bit against the
CPU side, with the failing (family, set index) pairs reported.

The tuned kNW path (hx_poa_sequences) against the oracle on the whole corpus and SLOW_SETS, under the default plan and under the launch
shapes test_gpu_parity.py forces on pipeline data: every block size, the score-matrix traceback, persistent slots, cluster mode on
these short sequences, the pruned row loop, column passes, no LDS ring (where the tie shortcut has no room and every tie takes the sort
fallback) and a ring of 1 KB; the cell count is the restatement's everywhere. Under the default plan the in-degree retry runs UNFORCED:
hx_poa_retry_stats counts exactly the sets whose graph, by the restatement, has a node with more than 16 in-edges. The witness of the
tie fallback is on the reference side (test_poa_hard_ref.py): ties of more than 8 candidates and closures of more than 32 nodes, which
the kernel's static gates send to the sort.

The general path (kernels/poa_modes.hip) on the corpus: kSW / kOV / kNW against the linear restatement, affine gaps against the affine
one, MSA rows with and without the consensus row, weighted consensus, coverage and profile under two weightings - each also with
first-round slots of 1 KB, so that sets stop and are rerun in larger slots."""
from concurrent.futures import ThreadPoolExecutor

import pytest

import msalib
import orclib
import parlib
import pmrlib
import poasets
import wgtlib
from test_poa_modes_ref import TRIPLES

pytestmark = pytest.mark.gpu
MODES = ["sw", "nw", "ov"]
CORPUS, SLOW_SETS = poasets.CORPUS, poasets.SLOW_SETS
ALL = CORPUS + [("slow", k, st) for k, st in enumerate(SLOW_SETS)]
THIRD = poasets.sub_sample(3)
AFFINE = [(5, -4, -8, -2), (3, -5, -4, 0)]


def sets_of(corpus):
    return [st for _, _, st in corpus]


def pmap(fn, items):
    with ThreadPoolExecutor(16) as ex:   # (the restatements and the oracle release the GIL: ctypes)
        return list(ex.map(fn, items))


def failing(corpus, got, want):
    """the (family, index) pairs of the sets whose results differ"""
    assert len(got) == len(want) == len(corpus)
    return [(f, k) for (f, k, _), a, b in zip(corpus, got, want) if a != b]


@pytest.fixture(scope="module")
def ctx(built):
    from haslr_amd import hip
    c = hip.HipContext(0)   # raises without a device: these tests never run on a fallback
    yield c
    c.close()


@pytest.fixture(scope="module")
def lin(built, tmp_path_factory):
    return pmrlib.ModesRef(str(tmp_path_factory.mktemp("hardg_pmr")))


@pytest.fixture(scope="module")
def nw_want(lin):
    """over ALL: the oracle's consensus of every set as read, the restatement's cell count and graph statistics (kNW, 5 / -4 / -8)"""
    cns = pmap(lambda c: orclib.poa_consensus([poasets.as_read(q) for q in c[2]]), ALL)
    res = pmap(lambda c: lin.consensus_stats(c[2], "nw"), ALL)
    assert failing(ALL, [r[0] for r in res], cns) == []
    return cns, sum(r[1] for r in res), [r[2] for r in res]


def check_tuned(ctx, nw_want, tag):
    cns, cells, _ = nw_want
    got, st = ctx.poa_sequences_mode(sets_of(ALL), "nw", stats=True)   # (the tuned path: hx_poa_sequences behind the entry that reports the counters)
    assert failing(ALL, got, cns) == [], tag
    assert st["dp_cells"] == cells, tag
    assert st["seq_bases"] == sum(len(q) for _, _, s in ALL for q in s) and st["n_aligned"] == sum(len(s) for _, _, s in ALL)


def test_tuned_path_under_the_default_plan_and_the_unforced_in_degree_retry(ctx, nw_want):
    cns, cells, stats = nw_want
    deep = [(f, k) for (f, k, _), s in zip(ALL, stats) if s["max_in_degree"] > 16]
    assert len(deep) >= 3 and ctx.get_option("poa_max_indeg") == 16
    got = ctx.poa_sequences(sets_of(ALL))
    assert failing(ALL, got, cns) == []
    retried = ctx.poa_retry_stats()
    print("retry statistics under the default plan:", retried, "sets with an in-degree above 16:", deep)
    assert retried["in_degree"] == len(deep)
    check_tuned(ctx, nw_want, "default")
    assert ctx.poa_retry_stats()["in_degree"] == len(deep)
    ctx.set_poa_traceback(0)
    try:
        check_tuned(ctx, nw_want, "score-matrix traceback")
        assert ctx.poa_retry_stats()["in_degree"] == 0
    finally:
        ctx.set_poa_traceback(1)
    # a call without such a set resets the counts
    assert ctx.poa_sequences([["ACGT", "ACGT"]]) == ["ACGT"] and set(ctx.poa_retry_stats().values()) == {0}


@pytest.mark.parametrize("block", [64, 128, 256, 512, 1024])
def test_tuned_path_block_sizes(ctx, nw_want, block):
    ctx.set_poa_block(block)
    try:
        check_tuned(ctx, nw_want, block)
    finally:
        ctx.set_poa_block(0)


CLUSTER_KEYS = ("poa_cluster_min", "poa_member_lanes", "poa_cluster_cols", "poa_cluster_max", "poa_wide_members", "poa_prune_shared")
SHAPES = {
    "slots1": {"poa_slots": 1}, "slots2": {"poa_slots": 2},
    # cluster mode forced on these short sequences: 64- and 256-lane members, 2 / 4 / 8 columns per lane, wide members none / some / all, pruning inside
    "cluster_64x8": dict(zip(CLUSTER_KEYS, (100, 64, 8, 8, 0))), "cluster_64x4_wide": dict(zip(CLUSTER_KEYS, (100, 64, 4, 3, 100))),
    "cluster_128x4": dict(zip(CLUSTER_KEYS, (200, 128, 4, 4, 2))), "cluster_256x8_wide": dict(zip(CLUSTER_KEYS, (200, 256, 8, 8, 100))),
    "cluster_256x2": dict(zip(CLUSTER_KEYS, (150, 256, 2, 8, 0))), "cluster_256x2_wide": dict(zip(CLUSTER_KEYS, (100, 256, 2, 3, 100))),
    "cluster_64x8_pruned": dict(zip(CLUSTER_KEYS, (100, 64, 8, 8, 0, 95))), "cluster_128x4_pruned": dict(zip(CLUSTER_KEYS, (150, 128, 4, 4, 2, 108))),
    "cluster_256x2_wide_pruned": dict(zip(CLUSTER_KEYS, (150, 256, 2, 8, 100, 95))),
    # the pruned row loop with an honest and an optimistic threshold, column passes, no ring / a small ring
    "pruned_95": {"HX_POA_PRUNE": 95, "HX_POA_WAVE_MAX": 128}, "pruned_108": {"HX_POA_PRUNE": 108, "HX_POA_WAVE_MAX": 64},
    "passes": {"HX_POA_PRUNE": 95, "HX_POA_WAVE_MAX": 64, "HX_POA_PASS_LANES": 64, "HX_POA_CLUSTER_MIN": 100000},
    "ring_zero": {"HX_POA_RING_ZERO": 1}, "ring_1kb": {"HX_POA_RING_KB": 1},
    "pruned_ring_zero": {"HX_POA_PRUNE": 95, "HX_POA_WAVE_MAX": 128, "HX_POA_CLUSTER_MIN": 100000, "HX_POA_RING_ZERO": 1},
    "pruned_ring_1kb": {"HX_POA_PRUNE": 108, "HX_POA_WAVE_MAX": 64, "HX_POA_CLUSTER_MIN": 100000, "HX_POA_RING_KB": 1},
}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_tuned_path_launch_shapes(ctx, nw_want, shape):
    with ctx.options(**SHAPES[shape]):
        check_tuned(ctx, nw_want, shape)


@pytest.fixture(scope="module")
def slots(ctx):
    """runs a call under the default slots and under first-round slots of 1 KB (sets stop and are rerun in larger ones)"""
    def both(call):
        out = [call()]
        with ctx.options(poa_modes_slot_kb=1):
            out.append(call())
        return out
    return both


@pytest.mark.parametrize("mode", MODES)
def test_general_path_modes(ctx, lin, slots, mode):
    for triple in TRIPLES:
        corpus = CORPUS if triple == TRIPLES[0] else THIRD
        res = pmap(lambda c: lin.consensus_cells(c[2], mode, *triple), corpus)
        with ctx.options(poa_general=1):   # (kNW through the general path; kSW and kOV run it anyway)
            for got, st in slots(lambda: ctx.poa_sequences_mode(sets_of(corpus), mode, *triple, stats=True)):
                assert failing(corpus, got, [r[0] for r in res]) == [], (mode, triple)
                assert st["dp_cells"] == sum(r[1] for r in res), (mode, triple)


@pytest.mark.parametrize("mode", MODES)
def test_general_path_affine(ctx, slots, mode, built, tmp_path):
    aff = parlib.AffineRef(str(tmp_path))
    for scores in AFFINE:
        corpus = CORPUS if scores == AFFINE[0] else THIRD
        res = pmap(lambda c: aff.consensus_cells(c[2], mode, *scores), corpus)
        for got, st in slots(lambda: ctx.poa_sequences_affine(sets_of(corpus), mode, *scores, stats=True)):
            assert failing(corpus, got, [r[0] for r in res]) == [], (mode, scores)
            assert st["dp_cells"] == sum(r[1] for r in res), (mode, scores)


@pytest.mark.parametrize("mode", MODES)
def test_general_path_msa_rows(ctx, slots, mode, built, tmp_path):
    ref = msalib.MsaRef(str(tmp_path))
    for scores in ((5, -4, -8, -8), AFFINE[0]):
        corpus = CORPUS if scores[2] == scores[3] else THIRD
        want = pmap(lambda c: ref.msa(c[2], mode, *scores, True), corpus)
        assert all(r.flags == 0 for r in want)
        kw = dict(type=mode, match=scores[0], mismatch=scores[1], gap_open=scores[2], gap_extend=scores[3])
        for rows, cns, _ in slots(lambda: ctx.poa_msa(sets_of(corpus), include_consensus=True, stats=True, **kw)):
            assert failing(corpus, rows, [r.rows for r in want]) == [], (mode, scores)
            assert failing(corpus, cns, [r.consensus for r in want]) == [], (mode, scores)
        for rows in slots(lambda: ctx.poa_msa(sets_of(corpus), **kw)):
            assert failing(corpus, rows, [r.rows[:-1] for r in want]) == [], (mode, scores, "without the consensus row")


@pytest.mark.parametrize("weighting", ["uniform", "quality"])
@pytest.mark.parametrize("mode", MODES)
def test_general_path_weighted(ctx, slots, mode, weighting, built, tmp_path):
    ref = wgtlib.WeightedRef(str(tmp_path))
    for scores in ((5, -4, -8, -8), AFFINE[0]):
        corpus = CORPUS if scores[2] == scores[3] else THIRD
        sets = sets_of(corpus)
        W = (wgtlib.uniform_weights if weighting == "uniform" else wgtlib.quality_weights)(sets, 71)
        want = pmap(lambda k: ref.weighted(sets[k], W[k], mode, *scores), range(len(sets)))
        assert all(r.flags == 0 for r in want)
        kw = dict(type=mode, match=scores[0], mismatch=scores[1], gap_open=scores[2], gap_extend=scores[3])
        for cns, cov, prof in slots(lambda: ctx.poa_weighted(sets, W, coverage=True, profile=True, **kw)):
            assert failing(corpus, list(zip(cns, cov, prof)), [(r.consensus, r.coverage, r.profile) for r in want]) == [], (mode, scores, weighting)
