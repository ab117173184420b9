"""The unrestricted heaviest-bundle pass of the tuned POA kernel (kernels/poa_graph.inl, bundle_pass_free: chosen in-edges by weight, scores by
pointer jumping inside chunks of 64 ranks, tied ranks finished in rank order) on the sets of tests/bundlesets.py, bit for bit against the
oracle: under the default plan, under forced workgroups of 64, 256 and 1 024 lanes, and under the wide two-column cluster members of
test_poa_hard_gpu.SHAPES. tests/test_poa_bundle_ref.py states on the CPU what each set is there for. No set is left out of any shape."""
from concurrent.futures import ThreadPoolExecutor

import pytest

import bundlesets
import orclib
from test_poa_hard_gpu import SHAPES

pytestmark = pytest.mark.gpu
BUNDLE_SHAPES = ["block_64", "block_256", "block_1024", "cluster_256x2_wide"]


@pytest.fixture(scope="module")
def ctx(built):
    from haslr_amd import hip
    c = hip.HipContext(0)   # raises without a device: these tests never run on a fallback
    yield c
    c.close()


@pytest.fixture(scope="module")
def want(built):
    """(names, sets, the oracle's consensus of every set), computed once"""
    names = [n for _, n, _ in bundlesets.BUILT]
    sets = [st for _, _, st in bundlesets.BUILT]
    with ThreadPoolExecutor(16) as ex:
        cns = list(ex.map(orclib.poa_consensus, sets))
    return names, sets, cns


def check(ctx, want, tag):
    names, sets, cns = want
    got = ctx.poa_sequences(sets)
    assert len(got) == len(sets)
    assert [n for n, a, b in zip(names, got, cns) if a != b] == [], tag


def test_default_plan(ctx, want):
    check(ctx, want, "default")


@pytest.mark.parametrize("shape", BUNDLE_SHAPES)
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
