"""hx_poa_labelled on the MI355X: the consensus of every label, its columns, coverage and profile, the MSA rows with one consensus row per
label and dp_cells equal the CPU restatement (tests/poa_label_ref.cpp) field by field: one set per workgroup width of the instance
tables, the lane edges of the 64-lane instance, the label counts and mixes, the hand-built sets of tests/test_poa_label_ref.py under every
type and gap model with weights, more sets than resident workgroups, the rerun in a larger slot, and every combination of the switches."""
import itertools
from concurrent.futures import ThreadPoolExecutor

import pytest

import lbllib
import wgtlib
from lbllib import NO_LABEL

pytestmark = pytest.mark.gpu
MODES = ["sw", "nw", "ov"]
MODELS = lbllib.MODELS
_wanted = {}


@pytest.fixture(scope="module")
def ref(built, tmp_path_factory):
    return lbllib.LabelRef(str(tmp_path_factory.mktemp("label_gpu")))


@pytest.fixture(scope="module")
def ctx(built):
    from haslr_amd import hip
    c = hip.HipContext(0)   # raises without a device: these tests never run on a fallback
    yield c
    c.close()


def wanted(ref, key, sets, labels, n_labels, mode, scores, weights=None):
    """the restatement's (record, cells, n_cols) per set, computed once per key and left unchanged"""
    if key not in _wanted:
        with ThreadPoolExecutor(16) as ex:   # (the restatement releases the GIL: ctypes)
            _wanted[key] = list(ex.map(lambda k: ref.labelled_cells(sets[k], labels[k], n_labels, mode, scores, None if weights is None else weights[k], True), range(len(sets))))
    return _wanted[key]


def assert_equal(ctx, want, sets, labels, n_labels, mode, scores, weights=None, msa=True, include_consensus=True, coverage=True, profile=True):
    """one call, every field it returns against the restatement's, and the counters; returns (records, counters)"""
    got, st = ctx.poa_labelled(sets, labels, n_labels, weights=weights, msa=msa, include_consensus=include_consensus, coverage=coverage, profile=profile, stats=True,
                               **lbllib.kw_of(scores, mode))
    assert len(got) == len(sets)
    for k, (g, (w, _, _)) in enumerate(zip(got, want)):
        assert g.consensus == w.consensus and g.columns == w.columns, (k, mode, scores)
        assert g.coverage == (w.coverage if coverage else None) and g.profile == (w.profile if profile else None), (k, mode, scores)
        assert g.rows == (None if not msa else w.rows if include_consensus else w.rows[:len(sets[k])]), (k, mode, scores)
    assert st["dp_cells"] == sum(w[1] for w in want)
    assert st["seq_bases"] == sum(len(q) for s in sets for q in s) and st["n_aligned"] == sum(1 for s in sets for q in s if q)
    return got, st


# the shortest longest sequence that selects each workgroup width (the instance tables of kernels/poa_modes_plan.h)
WIDTHS = [(64, "linear", 150, "nw"), (64, "affine", 151, "sw"), (64, "convex", 149, "ov"), (128, "convex", 1024, "nw"), (256, "linear", 1024, "ov"), (512, "affine", 4096, "nw"),
          (1024, "linear", 8192, "nw")]


@pytest.mark.parametrize("lanes,model,lmax,mode", WIDTHS)
def test_one_set_per_workgroup_width(ctx, ref, lanes, model, lmax, mode):
    seqs, labels = lbllib.exact_set(100 + lanes + lmax, lmax, 4 if lmax < 1000 else 3)
    assert max(len(q) for q in seqs) == lmax
    weights = wgtlib.quality_weights([seqs], lmax)
    want = wanted(ref, ("width", lanes, model), [seqs], [labels], 2, mode, MODELS[model], weights)
    got, _ = assert_equal(ctx, want, [seqs], [labels], 2, mode, MODELS[model], weights)
    assert all(len(c) >= lmax // 2 for c in got[0].consensus)


@pytest.mark.parametrize("mode", MODES)
def test_lane_edges_of_the_64_lane_instance(ctx, ref, mode):
    # sequences of 63, 64, 65 and 129 bases: label 0's consensus passes 64 ranks, label 1's 128
    sets, labels = [], []
    for seed in (201, 202):
        t = lbllib.template(__import__("random").Random(seed), 129)
        sets.append([t, t[:63], t[:65], t[:64]] if seed == 201 else [t[:63], t[:64], t[:65], t, t[1:64], t[64:]])
        labels.append([1, 0, 0, 1] if seed == 201 else [0, 1, 0, 1, 0, 1])
    for model in MODELS:
        want = wanted(ref, ("lanes", mode, model), sets, labels, 2, mode, MODELS[model])
        got, _ = assert_equal(ctx, want, sets, labels, 2, mode, MODELS[model])
        assert len(got[0].consensus[1]) > 128 and len(got[0].consensus[0]) > 64   # (the walk back passes the bundle's chunks of 64 ranks)


@pytest.mark.parametrize("n_labels", [1, 2, 16])
def test_label_counts_and_mixes(ctx, ref, n_labels):
    base = [lbllib.two_haplotypes(300 + k, 90 + 20 * k, 4, 0.06) for k in range(3)]
    sets = [s for s, _ in base]
    t = lbllib.template(__import__("random").Random(310), 140)
    sets.append([t] * 4 + [t[:70]])   # the members of a label share every edge: the atomic add
    if n_labels == 1:
        labels = [[0] * len(s) for s in sets]
    elif n_labels == 2:
        labels = [lb for _, lb in base] + [[0, 0, 0, 1, 1]]
        labels[1] = [NO_LABEL if k % 3 == 2 else lb for k, lb in enumerate(labels[1])]   # sequences without a label mixed in
        labels[2] = [0 if k else NO_LABEL for k in range(len(sets[2]))]                  # label 1 is empty, the set's first sequence has none
    else:
        labels = [[(5 * k + i) % 16 if (k + i) % 4 else NO_LABEL for k in range(len(s))] for i, s in enumerate(sets)]
        labels[3] = [15, 15, 15, 15, 0]
    weights = wgtlib.uniform_weights(sets, 320)
    for mode, model in (("nw", "linear"), ("ov", "affine"), ("sw", "convex")):
        want = wanted(ref, ("mix", n_labels, mode, model), sets, labels, n_labels, mode, MODELS[model], weights)
        got, _ = assert_equal(ctx, want, sets, labels, n_labels, mode, MODELS[model], weights)
    if n_labels == 2:
        assert got[2].consensus[1] == "" and got[2].consensus[0] and got[3].coverage[0] == [3] * 140


@pytest.mark.parametrize("model", list(MODELS))
@pytest.mark.parametrize("mode", MODES)
def test_the_hand_built_sets(ctx, ref, mode, model):
    sets = [h[0] for h in lbllib.HAND.values()]
    labels = [h[1] for h in lbllib.HAND.values()]
    weights = [lbllib.hand_weights(s) for s in sets]
    for w in (None, weights):
        want = wanted(ref, ("hand", mode, model, w is not None), sets, labels, 3, mode, MODELS[model], w)
        got, _ = assert_equal(ctx, want, sets, labels, 3, mode, MODELS[model], w)
    if mode == "nw":   # (the answers tests/test_poa_label_ref.py derives by hand, under the sets' own type)
        by = dict(zip(lbllib.HAND, ctx.poa_labelled(sets, labels, 3, **lbllib.kw_of(MODELS[model], mode))))
        assert by["one_mismatch"].consensus == ["AAGAA", "AATAA", ""] and by["minority"].consensus == ["AAGAA", "AATAA", ""]
        assert by["insertion"].columns[:2] == [[0, 1, 2, 3, 5, 6, 7, 8], list(range(9))]
        assert by["one_base"].consensus == ["ACGT", "C", ""] and by["unlabelled"].consensus == ["", "", ""]
    if mode == "sw":
        by = dict(zip(lbllib.HAND, ctx.poa_labelled(sets, labels, 3, **lbllib.kw_of(MODELS[model], mode))))
        assert by["branch"].consensus == [lbllib.BC_U + lbllib.BC_M, lbllib.BC_U + lbllib.BC_M + lbllib.BC_W, ""]


def test_more_sets_than_resident_workgroups(ctx, ref):
    picked = [lbllib.two_haplotypes(1000 + k, 30 + k % 23, 2 + k % 3, 0.08) for k in range(300)]
    sets, labels = [s for s, _ in picked], [lb for _, lb in picked]
    want = wanted(ref, ("many",), sets, labels, 2, "nw", lbllib.AFFINE)
    got, _ = assert_equal(ctx, want, sets, labels, 2, "nw", lbllib.AFFINE)
    # (a device holds more than 300 workgroups of one wavefront: half a megabyte of workspace has room for a few slots only, so that
    # every workgroup takes set after set off the counter)
    with ctx.options(poa_workspace_gb=0.0005):
        assert assert_equal(ctx, want, sets, labels, 2, "nw", lbllib.AFFINE)[0] == got


def test_the_rerun_in_a_larger_slot(ctx, ref):
    picked = [lbllib.two_haplotypes(400 + k, 300, 3, 0.05) for k in range(3)]
    sets, labels = [s for s, _ in picked], [lb for _, lb in picked]
    weights = wgtlib.uniform_weights(sets, 401)
    want = wanted(ref, ("slot",), sets, labels, 2, "nw", lbllib.CONVEX, weights)
    got, st = assert_equal(ctx, want, sets, labels, 2, "nw", lbllib.CONVEX, weights)
    with ctx.options(poa_modes_slot_kb=1):
        again, st2 = assert_equal(ctx, want, sets, labels, 2, "nw", lbllib.CONVEX, weights)
    assert again == got and st["slot_reruns"] == 0 and st2["slot_reruns"] > 0


def test_every_combination_of_the_switches(ctx, ref):
    seqs, labels = lbllib.two_haplotypes(450, 80, 4, 0.06)
    labels[-1] = NO_LABEL
    want = wanted(ref, ("switches",), [seqs], [labels], 3, "ov", lbllib.AFFINE)
    for msa, cns, cov, prof in itertools.product((False, True), repeat=4):
        assert_equal(ctx, want, [seqs], [labels], 3, "ov", lbllib.AFFINE, msa=msa, include_consensus=cns, coverage=cov, profile=prof)


def test_errors_carry_the_entrys_name(ctx):
    from haslr_amd import hip
    for nl in (0, 17):
        with pytest.raises(hip.HipError, match=f"hx_poa_labelled: n_labels must be 1..16, not {nl}"):
            ctx.poa_labelled([["ACGT"]], [[0]], nl)
    with pytest.raises(hip.HipError, match=r"hx_poa_labelled: set 1, sequence 2: label 2 is not below n_labels = 2 and not 255 \(no label\)"):
        ctx.poa_labelled([["ACGT"], ["A", "C", "G"]], [[0], [0, 255, 2]], 2)
    with pytest.raises(hip.HipError, match="hx_poa_labelled: set 0 holds a sequence of 8192 bases, longer than 8191"):
        ctx.poa_labelled([["A" * 8192]], [[0]], 1, **lbllib.kw_of(lbllib.CONVEX, "nw"))
