"""The tile walk of the tuned POA kernel (kernels/poa.hip: a table of next rows per tile of 64 rows x 32 columns, built by all lanes, walked
by one) on the sets of tests/walksets.py - every built set and the corpus picks with later predecessors and wide rows - bit for bit against
the oracle, with the restatement's cell count: under the default plan, under five of test_poa_hard_gpu's launch shapes, and on the
score-matrix traceback, the GPU's independent walk. No set is left out of any shape."""
from concurrent.futures import ThreadPoolExecutor

import pytest

import orclib
import pmrlib
import walksets
from test_poa_hard_gpu import SHAPES

pytestmark = pytest.mark.gpu
WALK_SHAPES = ["block_64", "block_256", "cluster_256x2_wide", "cluster_64x8", "pruned_95"]


@pytest.fixture(scope="module")
def ctx(built):
    from haslr_amd import hip
    c = hip.HipContext(0)   # raises without a device: these tests never run on a fallback
    yield c
    c.close()


@pytest.fixture(scope="module")
def want(built, tmp_path_factory):
    """(keys, sets, the oracle's consensus of every set, the restatement's cell count over all of them), computed once"""
    lin = pmrlib.ModesRef(str(tmp_path_factory.mktemp("walkg_pmr")))
    with ThreadPoolExecutor(16) as ex:
        stats = list(ex.map(lambda c: lin.consensus_stats(c[2], "nw")[2], walksets.CANDIDATES))
    later, wide = walksets.corpus_picks(stats)
    assert later and wide
    keys = [(f, name) for f, name, _, _ in walksets.BUILT] + [(f, k) for f, k, _ in later + wide]
    sets = [st for _, _, st, _ in walksets.BUILT] + [st for _, _, st in later + wide]
    with ThreadPoolExecutor(16) as ex:
        cns = list(ex.map(orclib.poa_consensus, sets))
        res = list(ex.map(lambda st: lin.consensus_cells(st, "nw"), sets))
    assert [r[0] for r in res] == cns
    return keys, sets, cns, sum(r[1] for r in res)


def check(ctx, want, tag):
    keys, sets, cns, cells = want
    got, st = ctx.poa_sequences_mode(sets, "nw", stats=True)
    assert len(got) == len(sets)
    assert [k for k, a, b in zip(keys, got, cns) if a != b] == [], tag
    assert st["dp_cells"] == cells, tag


def test_default_plan(ctx, want):
    check(ctx, want, "default")


@pytest.mark.parametrize("shape", WALK_SHAPES)
def test_launch_shapes(ctx, want, shape):
    if shape.startswith("block_"):
        ctx.set_poa_block(int(shape[6:]))
        try:
            check(ctx, want, shape)
        finally:
            ctx.set_poa_block(0)
    else:
        with ctx.options(**SHAPES[shape]):
            check(ctx, want, shape)


def test_score_matrix_traceback(ctx, want):
    ctx.set_poa_traceback(0)
    try:
        check(ctx, want, "score-matrix traceback")
    finally:
        ctx.set_poa_traceback(1)
