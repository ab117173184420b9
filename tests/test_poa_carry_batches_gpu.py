"""The carry hand-over of the tuned POA kernel's wave pipeline (kernels/poa_dp.inl: batches of carries out of a tagged ring, the right
neighbour's count read only when the last value does not cover a batch, the wave's own count told every 16 rows) on the sets of
tests/carrysets.py, bit for bit against the oracle, with the restatement's cell count: under the default plan, under forced workgroups of
128, 256 and 512 lanes, and under five of test_poa_hard_gpu's cluster shapes - members of one, two and four waves, wide members with their
relay wave, pruning inside the shared edge. No set is left out of any shape."""
from concurrent.futures import ThreadPoolExecutor

import pytest

import carrysets
import orclib
import pmrlib
from test_poa_hard_gpu import SHAPES

pytestmark = pytest.mark.gpu
CARRY_SHAPES = ["block_128", "block_256", "block_512", "cluster_64x8", "cluster_128x4", "cluster_256x2", "cluster_256x2_wide", "cluster_128x4_pruned"]


@pytest.fixture(scope="module")
def ctx(built):
    from haslr_amd import hip
    c = hip.HipContext(0)   # raises without a device: these tests never run on a fallback
    yield c
    c.close()


@pytest.fixture(scope="module")
def want(built, tmp_path_factory):
    """(names, sets, the oracle's consensus of every set, the restatement's cell count over all of them), computed once"""
    lin = pmrlib.ModesRef(str(tmp_path_factory.mktemp("carryg_pmr")))
    names = [n for _, n, _, _ in carrysets.BUILT]
    sets = [st for _, _, st, _ in carrysets.BUILT]
    with ThreadPoolExecutor(16) as ex:
        cns = list(ex.map(orclib.poa_consensus, sets))
        res = list(ex.map(lambda st: lin.consensus_cells(st, "nw"), sets))
    assert [r[0] for r in res] == cns
    return names, sets, cns, sum(r[1] for r in res)


def check(ctx, want, tag):
    names, sets, cns, cells = want
    got, st = ctx.poa_sequences_mode(sets, "nw", stats=True)
    assert len(got) == len(sets)
    assert [n for n, a, b in zip(names, got, cns) if a != b] == [], tag
    assert st["dp_cells"] == cells, tag


def test_default_plan(ctx, want):
    check(ctx, want, "default")


@pytest.mark.parametrize("shape", CARRY_SHAPES)
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
