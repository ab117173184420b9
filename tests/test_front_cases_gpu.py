"""The HIP chain, edge and coordinate kernels on the hand-built PAF edge cases of tests/frontcases.py, bit for bit against the CPU
oracle: reads past one wavefront (the chain kernel's one-lane path), trim walks that stop in every CIGAR letter and at every lane
split of trim_walk_wave, filters at exact equality, ties, and edges above and at the coordinate kernel's LDS_SUPP = 384. The
manifests themselves are checked on the CPU (test_front_cases.py)."""
import os
import subprocess

import numpy as np
import pytest

import frontcases as fc
import orclib
import util
from haslr_amd import hip, host

pytestmark = pytest.mark.gpu
FAMILIES = fc.FAMILIES + fc.GPU_ONLY


@pytest.fixture(scope="module")
def ctx(built):
    c = hip.HipContext(0)   # raises without a device: no fallback
    yield c
    c.close()


@pytest.fixture(scope="module")
def cases(built, tmp_path_factory):
    made = {}

    def get(name):
        if name not in made:
            made[name] = fc.build(str(tmp_path_factory.mktemp(name)), fc.FAMILIES if name == "combined" else [name], seed=7 if name == "combined" else 1)
        return made[name]
    return get


def both(ds, ctx, out_o, out_g):
    """the whole stage on the oracle and on the HIP path (test_gpu_parity.py's both())"""
    ob = orclib.OracleBackend(ds, 4)
    ro = host.Run(ds, ds.params(), ob.table, out_o)
    ro.all()
    ctx.upload(ds)
    rg = host.Run(ds, ds.params(), ctx.backend(), out_g)
    rg.all()
    return ro, rg, ob


def assert_same(ro, rg):
    for what, a, b in (("chain", ro.chain_out(), rg.chain_out()), ("edges", ro.edges_out(), rg.edges_out()),
                       ("coords", ro.coords_out(), rg.coords_out())):
        for k in a:
            assert np.array_equal(a[k], b[k]), f"{what}.{k} differs between the HIP path and the oracle"
    assert ro.cns_out() == rg.cns_out()
    assert ro.cns_stats() == rg.cns_stats()


def open_ds(pre, index_dir=None):
    return host.Dataset(pre + ".contigs.fa", pre + ".reads.fa", pre + ".paf", index_dir=index_dir)


@pytest.mark.parametrize("family", FAMILIES)
def test_family_bit_exact(family, cases, ctx, tmp_path):
    pre, case = cases(family)
    ds = open_ds(pre)
    ro, rg, ob = both(ds, ctx, str(tmp_path / "o"), str(tmp_path / "g"))
    assert_same(ro, rg)
    assert util.compare_dirs(str(tmp_path / "o"), str(tmp_path / "g")) == []
    assert len(rg.chain_out()["hit"]) > 0
    rg.close(); ro.close(); ob.close(); ds.close()


@pytest.mark.parametrize("family", ["coords", "combined"])
def test_coords_through_the_global_scratch(family, cases, ctx):
    """option coords_lds_supp=0: every edge, not only the 400-support one, through the coordinate kernel's global scratch"""
    pre, case = cases(family)
    ds = open_ds(pre)
    with ctx.options(coords_lds_supp="0"):
        ro, rg, ob = both(ds, ctx, None, None)
    assert_same(ro, rg)
    assert (np.diff(rg.coords_out()["supp_off"]) > 0).sum() >= 2
    rg.close(); ro.close(); ob.close(); ds.close()


@pytest.mark.parametrize("family", FAMILIES)
def test_prefiltered_route(family, cases, ctx, tmp_path):
    """index.longread written from the oracle's run, loaded back: the chain kernel takes its records as they are"""
    pre, case = cases(family)
    ds = open_ds(pre)
    ob = orclib.OracleBackend(ds, 4)
    run = host.Run(ds, ds.params(), ob.table, None)
    run.chain()
    idx = str(tmp_path / "idx")
    os.makedirs(idx)
    ds.write_contig_index(os.path.join(idx, "index.contig"))
    run.write_longread_index(os.path.join(idx, "index.longread"))
    run.close(); ob.close(); ds.close()
    di = open_ds(pre, idx)
    assert di.used_longread_index
    ro, rg, ob = both(di, ctx, None, None)
    assert_same(ro, rg)
    rg.close(); ro.close(); ob.close(); di.close()


def test_hip_front_half_against_the_reference(cases, ctx, ref_front, tmp_path):
    """every family in one data set: the HIP front half against the compiled reference's files"""
    pre, case = cases("combined")
    rd = str(tmp_path / "ref")
    os.makedirs(rd)
    subprocess.check_call([ref_front, "-c", pre + ".contigs.fa", "-l", pre + ".reads.fa", "-m", pre + ".paf", "-d", rd],
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    ds = open_ds(pre)
    ctx.upload(ds)
    gd = str(tmp_path / "g")
    run = host.Run(ds, ds.params(), ctx.backend(), gd)
    run.chain()
    run.graph()
    assert util.compare_dirs(rd, gd) == []
    chain, edges = run.chain_out(), run.edges_out(sides=False)
    assert fc.fixed_paf_equal(case, ds, chain, open(os.path.join(rd, "alignments.fixed.paf")).read()) > 0
    assert util.edge_supp_text(edges) == open(os.path.join(rd, "edge_supp.01.txt")).read()
    keep = util.gfa_edge_keys(os.path.join(gd, "backbone.06.smallbubble.gfa"))
    assert util.edge_supp_text(edges, keep) == open(os.path.join(rd, "edge_supp.06.txt")).read()
    run.close(); ds.close()
