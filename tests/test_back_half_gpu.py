"""The back half of the HIP path (K5 edge coordinates, the sub-sequence rule in the POA batch, stitching in the host pipeline) against a
live run of the compiled reference's whole program (oracle/_ref/ref_back, which travels with the built tree; tests/backlib.py): on the
hand-built `back` family of tests/backcases.py with the coordinate kernel's supports in LDS (default), in the global scratch
(coords_lds_supp=0) and split between the two at 3 supports, on the `coords` family (400 and 384 supports per edge) and on two
simulated sets. The consensus strings the reference stitches are the CPU oracle's; the HIP consensus must equal them bit for bit, as
everywhere else in the suite. The `back` family is also checked against the stored results of the reference (golden/back_family)."""
import json
import os

import pytest

import backcases as bc
import backlib
import frontcases as fc
import util
from haslr_amd import hip, host

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# the two smallest of the simulated sets of test_back_half_ref.py (by read bases: the reference's run is the longest part of a case)
SIMS = [("--genome-len", "150000", "--seed", "21", "--variant-per-mb", "30"),
        ("--genome-len", "200000", "--seed", "8", "--variant-per-mb", "30", "--cov", "14", "--hairpin-frac", "0.1")]


@pytest.fixture(scope="module")
def ctx(built):
    c = hip.HipContext(0)   # raises without a device: no fallback
    yield c
    c.close()


@pytest.fixture(scope="module")
def back(built, tmp_path_factory):
    """the `back` family, made once: (prefix, Case, directory for the reference's run)"""
    d = tmp_path_factory.mktemp("back")
    pre, case = bc.build(str(d / "in"))
    return pre, case, str(d / "ref")


def hip_run(ctx, pre, out):
    ds = host.Dataset(pre + ".contigs.fa", pre + ".reads.fa", pre + ".paf")
    ctx.upload(ds)
    run = host.Run(ds, ds.params(), ctx.backend(), out)
    run.all()
    return ds, run


@pytest.mark.parametrize("lds_supp", [None, "0", "3"])
def test_back_family_equals_the_reference(lds_supp, back, ctx, tmp_path):
    pre, case, rd = back
    if not os.path.isdir(rd):
        backlib.run_ref(pre, rd)
    out = str(tmp_path / "g")
    if lds_supp is None:
        ds, run = hip_run(ctx, pre, out)
    else:
        with ctx.options(coords_lds_supp=lds_supp):
            ds, run = hip_run(ctx, pre, out)
    c = backlib.check_against_ref(run, ds, rd, out, pre)
    for k, v in case.man["back"]["census"].items():
        if not k.startswith("case"):
            assert c[k] == v, f"{k}: the reference's logs show {c[k]}, planted {v}"
    run.close(); ds.close()


def test_back_family_equals_the_stored_reference_run(back, ctx, tmp_path):
    pre, case, _ = back
    cd = os.path.join(GOLD, "back_family")
    man = json.load(open(os.path.join(cd, "back_manifest.json")))
    for k, h in man["inputs"].items():
        if util.sha256_file(pre + k) != h:
            pytest.skip("tests/backcases.py produced different bytes than when the fixture was made")
    out = str(tmp_path / "g")
    ds, run = hip_run(ctx, pre, out)
    backlib.golden_back_check(man["back"], os.path.join(cd, "expected_back"), run, out)
    run.close(); ds.close()


def test_coords_family_equals_the_reference(ctx, built, tmp_path):
    """the edges of 400 and 384 supports (above and at LDS_SUPP)"""
    pre, case = fc.build(str(tmp_path / "in"), ["coords"])
    rd, out = backlib.run_ref(pre, str(tmp_path / "ref")), str(tmp_path / "g")
    ds, run = hip_run(ctx, pre, out)
    c = backlib.check_against_ref(run, ds, rd, out, pre)
    assert c["edges"] == 2 and c["stitching"] == 2
    run.close(); ds.close()


@pytest.mark.parametrize("args", SIMS, ids=lambda a: "_".join(a[1:4:2]))
def test_simulated_sets_equal_the_reference(args, sim, ctx, tmp_path):
    pre = sim(*args)
    rd, out = backlib.run_ref(pre, str(tmp_path / "ref")), str(tmp_path / "g")
    ds, run = hip_run(ctx, pre, out)
    c = backlib.check_against_ref(run, ds, rd, out, pre)
    assert c["edges"] >= 6 and all(c[f"case{k}"] > 0 for k in range(1, 9))
    run.close(); ds.close()
