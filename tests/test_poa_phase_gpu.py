"""hx_poa_phased on the MI355X: the haplotype of every sequence, the sites, rounds and verdict, and per haplotype the consensus, its columns,
coverage and profile, the MSA rows with two consensus rows and dp_cells equal the CPU restatement (tests/poa_phase_ref.cpp) field by field,
and equal HipContext.poa_labelled fed the returned haplotypes as labels, which pins the new entry to a tested one on the same device:
one set per workgroup width, the lane edges of the 64-lane instance, the hand-built sets of tests/test_poa_phase_ref.py under every type
and gap model with weights, more sequences than a wavefront and than a workgroup, 0, 1 and 65 sites, sites in the first and the last
column, more sets than resident workgroups, the rerun in a larger slot, every combination of the switches, and sets without a base."""
import itertools
import random
from concurrent.futures import ThreadPoolExecutor

import pytest

import phaselib
import wgtlib

pytestmark = pytest.mark.gpu
MODES = ["sw", "nw", "ov"]
MODELS = phaselib.MODELS
_wanted = {}


@pytest.fixture(scope="module")
def ref(built, tmp_path_factory):
    return phaselib.PhaseRef(str(tmp_path_factory.mktemp("phase_gpu")))


@pytest.fixture(scope="module")
def ctx(built):
    from haslr_amd import hip
    c = hip.HipContext(0)   # raises without a device: these tests never run on a fallback
    yield c
    c.close()


def wanted(ref, key, sets, mode, scores, weights=None, min_count=2, min_pct=25):
    """the restatement's (record, cells, n_cols) per set, computed once per key and left unchanged"""
    if key not in _wanted:
        with ThreadPoolExecutor(16) as ex:   # (the restatement releases the GIL: ctypes)
            _wanted[key] = list(ex.map(lambda k: ref.phased_cells(sets[k], mode, scores, None if weights is None else weights[k], True, min_count, min_pct), range(len(sets))))
    return _wanted[key]


def assert_equal(ctx, want, sets, mode, scores, weights=None, min_count=2, min_pct=25, msa=True, include_consensus=True, coverage=True, profile=True, labelled=True):
    """one call, every field it returns against the restatement's, the counters, and poa_labelled given the haplotypes; returns (records, counters)"""
    kw = phaselib.kw_of(scores, mode)
    got, st = ctx.poa_phased(sets, weights=weights, min_count=min_count, min_pct=min_pct, msa=msa, include_consensus=include_consensus, coverage=coverage, profile=profile,
                             stats=True, **kw)
    assert len(got) == len(sets)
    for k, (g, (w, _, _)) in enumerate(zip(got, want)):
        assert (g.hap, g.n_haps, g.rounds, g.sites) == (w.hap, w.n_haps, w.rounds, w.sites), (k, mode, scores)
        assert g.consensus == w.consensus and g.columns == w.columns, (k, mode, scores)
        assert g.coverage == (w.coverage if coverage else None) and g.profile == (w.profile if profile else None), (k, mode, scores)
        assert g.rows == (None if not msa else w.rows if include_consensus else w.rows[:len(sets[k])]), (k, mode, scores)
    assert st["dp_cells"] == sum(w[1] for w in want)
    assert st["seq_bases"] == sum(len(q) for s in sets for q in s) and st["n_aligned"] == sum(1 for s in sets for q in s if q)
    if labelled:
        lab = ctx.poa_labelled(sets, [g.hap for g in got], 2, weights=weights, msa=msa, include_consensus=include_consensus, coverage=coverage, profile=profile, **kw)
        for k, (g, b) in enumerate(zip(got, lab)):
            assert (g.consensus, g.columns, g.coverage, g.profile, g.rows) == (b.consensus, b.columns, b.coverage, b.profile, b.rows), (k, mode, scores)
    return got, st


# the shortest longest sequence that selects each workgroup width (the instance tables of kernels/poa_modes_plan.h)
WIDTHS = [(64, "linear", 150, "nw"), (64, "affine", 151, "sw"), (64, "convex", 149, "ov"), (128, "convex", 1024, "nw"), (256, "linear", 1024, "ov"), (512, "affine", 4096, "nw"),
          (1024, "linear", 8192, "nw")]


@pytest.mark.parametrize("lanes,model,lmax,mode", WIDTHS)
def test_one_set_per_workgroup_width(ctx, ref, lanes, model, lmax, mode):
    seqs, truth, _ = phaselib.snp_set(100 + lanes + lmax, lmax, 2, snps=5)
    assert max(len(q) for q in seqs) == lmax
    weights = wgtlib.quality_weights([seqs], lmax)
    want = wanted(ref, ("width", lanes, model), [seqs], mode, MODELS[model], weights)
    got, _ = assert_equal(ctx, want, [seqs], mode, MODELS[model], weights)
    assert got[0].hap == truth and got[0].n_haps == 2 and len(got[0].sites) == 5


@pytest.mark.parametrize("mode", MODES)
def test_lane_edges_of_the_64_lane_instance(ctx, ref, mode):
    # sequences of 63, 64, 65 and 129 bases of two haplotypes with a site near either end of the short ones
    rnd = random.Random(210)
    t = phaselib.template(rnd, 129)
    u = "".join({"A": "C", "C": "G", "G": "T", "T": "A"}[ch] if i in (3, 60, 126) else ch for i, ch in enumerate(t))
    sets = [[t, u, t[:63], u[:63], t[:65], u[:65], t[:64], u[:64]], [t[:63], u[:64], t[:65], u, t[1:64], u[1:64], t[64:], u[64:], t, u[:63]]]
    for model in MODELS:
        want = wanted(ref, ("lanes", mode, model), sets, mode, MODELS[model])
        got, _ = assert_equal(ctx, want, sets, mode, MODELS[model])
        assert got[0].n_haps == 2 and got[0].hap == [0, 1] * 4


@pytest.mark.parametrize("model", list(MODELS))
@pytest.mark.parametrize("mode", MODES)
def test_the_hand_built_sets(ctx, ref, mode, model):
    names = list(phaselib.HAND)
    for mc, mp in sorted({(h[2], h[3]) for h in phaselib.HAND.values()}):
        pick = [n for n in names if phaselib.HAND[n][2:] == (mc, mp)]
        sets = [phaselib.HAND[n][0] for n in pick]
        weights = [phaselib.hand_weights(s) for s in sets]
        for w in (None, weights):
            want = wanted(ref, ("hand", mode, model, mc, mp, w is not None), sets, mode, MODELS[model], w, mc, mp)
            got, _ = assert_equal(ctx, want, sets, mode, MODELS[model], w, mc, mp)
        by = dict(zip(pick, got))
        if mode == "nw" and "snp" in by:   # (the answers tests/test_poa_phase_ref.py derives by hand, under the sets' own type)
            assert by["snp"].sites == [(2, 2, 3, 1)] and by["snp"].consensus == ["AAGAA", "AATAA"] and by["snp_swapped"].sites == [(2, 2, 3, -1)]
            assert by["deletion"].sites == [(3, 2, 4, 1)] and by["ends"].sites == [(0, 1, 3, 1), (5, 1, 2, -1)]
            assert by["three_alleles"].hap[-1] == 255 and by["short_of_pct"].n_haps == 1 and by["empty_and_one_base"].hap == [0, 255, 1, 255, 0, 1, 255]
        if mode == "ov" and "moves" in by:
            assert by["moves"].rounds == 2 and by["moves"].hap[6] == 0 and by["fragments"].hap[-2:] == [0, 255]
        if mode == "nw" and "loses" in by:
            assert (by["loses"].n_haps, by["loses"].rounds, by["loses"].consensus[1]) == (1, 2, "")


def test_more_sequences_than_a_wavefront_and_than_a_workgroup(ctx, ref):
    rnd = random.Random(220)
    t = phaselib.template(rnd, 20)
    u = t[:6] + {"A": "C", "C": "G", "G": "T", "T": "A"}[t[6]] + t[7:14] + {"A": "C", "C": "G", "G": "T", "T": "A"}[t[14]] + t[15:]
    sets = []
    for n in (65, 1025):
        order = [rnd.randrange(2) for _ in range(n)]
        sets.append([(u if g else t)[:rnd.choice((20, 20, 19, 18))] for g in order])
    want = wanted(ref, ("many_seqs",), sets, "nw", phaselib.LINEAR)
    got, _ = assert_equal(ctx, want, sets, "nw", phaselib.LINEAR)
    assert [g.n_haps for g in got] == [2, 2] and all(set(g.hap) == {0, 1} for g in got)


@pytest.mark.parametrize("n_sites", [0, 1, 65])
def test_the_number_of_sites(ctx, ref, n_sites):
    sets = [phaselib.many_sites(n_sites) if n_sites else ["GGAGG"] * 6]
    for mode in ("nw", "sw"):
        want = wanted(ref, ("sites", n_sites, mode), sets, mode, phaselib.AFFINE)
        got, _ = assert_equal(ctx, want, sets, mode, phaselib.AFFINE)
        assert len(got[0].sites) == n_sites and got[0].n_haps == (2 if n_sites else 1) and got[0].rounds == (1 if n_sites else 0)
    if n_sites == 65:   # (the site compaction crosses a wavefront; every site agrees with the seed)
        assert [s[0] for s in got[0].sites] == list(range(2, 2 + 3 * 65, 3)) and all(s[3] == 1 for s in got[0].sites)


def test_sites_in_the_first_and_the_last_column(ctx, ref):
    sets = [phaselib.ENDS, [q + "ACGTTGCA" * 9 + p for q, p in zip(phaselib.ENDS, reversed(phaselib.ENDS))]]
    for model in MODELS:
        want = wanted(ref, ("ends", model), sets, "nw", MODELS[model])
        got, _ = assert_equal(ctx, want, sets, "nw", MODELS[model])
    assert got[0].sites[0][0] == 0 and got[0].sites[-1][0] == 5 and got[1].sites[0][0] == 0 and got[1].sites[-1][0] == len(sets[1][0]) - 1


def test_more_sets_than_resident_workgroups(ctx, ref):
    # phased and unphased sets mixed: every third set is copies of one template (no site), the others two haplotypes with noise
    sets = []
    for k in range(300):
        if k % 3 == 2:
            sets.append([phaselib.template(random.Random(3000 + k), 25 + k % 17)] * (2 + k % 4))
        else:
            sets.append(phaselib.snp_set(1000 + k, 30 + k % 23, 2 + k % 3, snps=1 + k % 4, err=0.04 * (k % 2))[0])
    want = wanted(ref, ("many",), sets, "nw", phaselib.AFFINE)
    got, _ = assert_equal(ctx, want, sets, "nw", phaselib.AFFINE)
    assert {g.n_haps for g in got} == {1, 2}
    # (a device holds more than 300 workgroups of one wavefront: half a megabyte of workspace has room for a few slots only, so that
    # every workgroup takes set after set off the counter, a set without a site right after one with many)
    with ctx.options(poa_workspace_gb=0.0005):
        assert assert_equal(ctx, want, sets, "nw", phaselib.AFFINE, labelled=False)[0] == got


def test_the_rerun_in_a_larger_slot(ctx, ref):
    sets = [phaselib.snp_set(400 + k, 300, 3, snps=4, err=0.05)[0] for k in range(3)]
    weights = wgtlib.uniform_weights(sets, 401)
    want = wanted(ref, ("slot",), sets, "nw", phaselib.CONVEX, weights)
    got, st = assert_equal(ctx, want, sets, "nw", phaselib.CONVEX, weights)
    with ctx.options(poa_modes_slot_kb=1):
        again, st2 = assert_equal(ctx, want, sets, "nw", phaselib.CONVEX, weights, labelled=False)
    assert again == got and st["slot_reruns"] == 0 and st2["slot_reruns"] > 0


def test_every_combination_of_the_switches(ctx, ref):
    seqs = phaselib.snp_set(450, 80, 4, snps=3, err=0.05)[0] + [""]
    want = wanted(ref, ("switches",), [seqs], "ov", phaselib.AFFINE)
    for msa, cns, cov, prof in itertools.product((False, True), repeat=4):
        assert_equal(ctx, want, [seqs], "ov", phaselib.AFFINE, msa=msa, include_consensus=cns, coverage=cov, profile=prof)


def test_sets_without_a_base(ctx, ref):
    sets = [["", "", ""], phaselib.SNP, [], [""]]
    want = wanted(ref, ("empty",), sets, "nw", phaselib.LINEAR)
    got, _ = assert_equal(ctx, want, sets, "nw", phaselib.LINEAR)
    assert got[0].hap == [255] * 3 and (got[0].n_haps, got[0].rounds, got[0].sites, got[0].consensus) == (1, 0, [], ["", ""]) and got[1].n_haps == 2
    assert ctx.poa_phased([]) == [] and ctx.poa_phased([[""], []])[0].hap == [255]


def test_errors_carry_the_entrys_name(ctx):
    from haslr_amd import hip
    for kw in (dict(min_count=0), dict(min_count=256), dict(min_pct=0), dict(min_pct=51)):   # (the C entry's own refusals: tests/test_poa_phase_abi.py)
        with pytest.raises(ValueError, match="min_count is 1..255, min_pct 1..50"):
            ctx.poa_phased([["ACGT"]], **kw)
    with pytest.raises(hip.HipError, match="hx_poa_phased: set 0 holds a sequence of 8192 bases, longer than 8191"):
        ctx.poa_phased([["A" * 8192]], **phaselib.kw_of(phaselib.CONVEX, "nw"))
    # the score bound of the full matrix: 1 024 bases + the 1 024 columns of their instance, times 2^18, reaches 2^29
    import re
    import gscorelib
    seqs, scores = ["A" * 1023, "A"], (5, -4, -(1 << 18), -(1 << 18), -(1 << 18), -(1 << 18))
    assert gscorelib.bound_product(seqs, scores, "linear") == gscorelib.SCORE_BOUND
    with pytest.raises(hip.HipError, match=re.escape(gscorelib.refusal("hx_poa_phased", 0, seqs, scores, "linear"))):
        ctx.poa_phased([seqs], match=5, mismatch=-4, gap_open=-(1 << 18))
