"""The general POA path on the MI355X under the score sets of tests/gscorelib.py: match <= 0, mismatch >= match or above 0, everything
tying at 0, nothing positive under kSW, the ends of int8, and int32 scores up to the bound describe() now holds (kernels/poa_modes_plan.h,
SCORE_BOUND; DESIGN.md section 11, "Score range of the full matrix"). tests/test_poa_gscores_ref.py shows without a GPU that the
restatements are a reference under these scores and that no case is vacuous.

    hx_poa_graph      every score set x type x gap model: nodes, edges, paths, alignment pairs and end scores equal the graph restatement
                      field by field over the corpus, one call per combination; the failing sets are reported as (family, index)
    hx_poa_banded     the band kernel (other DP code) at half-widths 8 and 64 against tests/poa_band_ref.cpp, on the sets wider than the window
    hx_poa_strand     the leading set of each group, a third of the members reverse-complemented
    hx_poa_labelled   once per group
    scale             k x the scores with the bound's product just under 2^29 gives the graph and the pairs of k = 1 and k x its end scores
                      (no reference needed); the smallest k that reaches the bound is refused with describe()'s text
    cross-entry       hx_poa_sequences_mode / _affine / _convex return hx_poa_graph's consensus

How far the scale case reaches. It would be a stronger case if the most negative end score times k exceeded half the bound. No sound
bound allows that on these sets: the bound counts a score per node and per column, since a path of a graph can pass every node, that
is (bases + columns of the instance) x the largest magnitude, at least 3 x 1 100 + the instance's columns here, while the best global
alignment of 1 100 bases never costs more than its all-diagonal path, 1 100 x the largest magnitude. Under (-3, -3, -3, ...), where every
step costs the largest magnitude, that is 1 100 / (2 200 + 4 096) = 0.17 of the bound for the pair on the linear instance and 0.10 for the
three noisy copies on the convex one (whose largest magnitude, q = -6, is twice a step's cost). The test prints the fraction per gap model
and asserts a sixteenth; what comes nearest to the bound is not a stored cell but the scan term -2^29 - j e of the instance's last columns."""
from concurrent.futures import ThreadPoolExecutor

import pytest

import bandlib
import grflib
import gscorelib as gs
import lbllib
import strlib

pytestmark = pytest.mark.gpu
MODELS, MODES = gs.MODELS, gs.MODES
_wanted = {}


@pytest.fixture(scope="module")
def ctx(built):
    from haslr_amd import hip
    c = hip.HipContext(0)   # raises without a device: these tests never run on a fallback
    yield c
    c.close()


@pytest.fixture(scope="module")
def refs(built, tmp_path_factory):
    return gs.References(grflib.GraphRef(str(tmp_path_factory.mktemp("gscores_grf"))))


@pytest.fixture(scope="module")
def band_ref(built, tmp_path_factory):
    return bandlib.BandRef(str(tmp_path_factory.mktemp("gscores_band")))


@pytest.fixture(scope="module")
def strand_ref(built, tmp_path_factory):
    return strlib.StrandRef(str(tmp_path_factory.mktemp("gscores_str")))


@pytest.fixture(scope="module")
def label_ref(built, tmp_path_factory):
    return lbllib.LabelRef(str(tmp_path_factory.mktemp("gscores_lbl")))


def wanted(key, fn, items):
    """a restatement's results over items, computed once per key and left unchanged"""
    if key not in _wanted:
        with ThreadPoolExecutor(16) as ex:   # (the restatements release the GIL: ctypes)
            _wanted[key] = list(ex.map(fn, items))
    return _wanted[key]


# ---- hx_poa_graph
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", gs.NAMES)
def test_graph_equals_the_restatement(ctx, refs, name, mode, model):
    scores, corpus = gs.scores_of(name, model), gs.corpus_of(name, mode)
    want = refs.records(scores, mode, corpus)
    got, st = ctx.poa_graph(gs.sets_of(corpus), stats=True, **grflib.kw_of(scores, mode))
    for field in ("node_base", "consensus", "n_cols"):
        assert gs.failing(corpus, got, want, lambda a, b: getattr(a, field) == getattr(b, field)) == [], field
    assert gs.failing(corpus, got, want, lambda a, b: [sq.score for sq in a.sequences] == [sq.score for sq in b.sequences]) == [], "end scores"
    assert gs.failing(corpus, got, want, lambda a, b: [sq.alignment for sq in a.sequences] == [sq.alignment for sq in b.sequences]) == [], "alignment pairs"
    assert gs.failing(corpus, got, want, grflib.same) == []
    assert st["dp_cells"] == refs.cells(scores, mode, corpus)


# ---- the band kernel
def band_corpus(band, name, mode):
    """the sets of at most 8 000 bases of a score set's corpus that are wider than the window, so that the window really runs (the two long sets among them)"""
    return [c for c in gs.light(gs.corpus_of(name, mode)) if max(len(q) for q in c[2]) + 1 > 2 * band + 1]


@pytest.mark.parametrize("band", [8, 64])
@pytest.mark.parametrize("name", gs.NAMES)
def test_band_kernel_equals_its_restatement(ctx, band_ref, name, band):
    k = gs.NAMES.index(name) + (band == 64)
    for model, mode in ((MODELS[k % 3], MODES[k % 3]), (MODELS[(k + 1) % 3], MODES[(k + 2) % 3])):   # (over the score sets: every model under every type)
        corpus = band_corpus(band, name, mode)
        sets = gs.sets_of(corpus)
        assert len(corpus) >= 15
        scores = gs.scores_of(name, model)
        want = wanted(("band", name, band, model, mode), lambda st: band_ref.banded_cells(st, band, mode, scores, None, True), sets)
        got, st = ctx.poa_banded(sets, band, msa=True, include_consensus=True, coverage=True, profile=True, stats=True, **bandlib.kw_of(scores, mode))
        for field in ("consensus", "band_used", "rows", "coverage", "profile"):
            assert gs.failing(corpus, got, [w[0] for w in want], lambda a, b: getattr(a, field) == getattr(b, field)) == [], (field, model, mode)
        assert st["dp_cells"] == sum(w[1] for w in want) and st["band_reruns"] == sum(w[2] for w in want), (model, mode)
        # the band kernel gave the result wherever the restatement stays banded, not the full matrix. Where no score is positive the best cell of a
        # row is its first, the centre never leaves column 0, and a global alignment misses every band: by the rules those sets end on the full matrix
        kept = [i for i, w in enumerate(want) if w[0].band_used]
        assert all(got[i].band_used != 0 for i in kept), (model, mode)
        assert len(kept) >= 10 or (mode == "nw" and name in gs.NOTHING_POSITIVE and st["band_reruns"] >= len(corpus)), (model, mode, len(kept))


# ---- hx_poa_strand
def strand_sets():
    """a tenth of the corpus, at most nine members of each, and the noisy long set; every third member, the second first, reverse-complemented"""
    return [[strlib.rc(q) if k % 3 == 1 else q for k, q in enumerate(st[:9])] for _, _, st in gs.CORPUS[::10] + gs.LONG[:1]]


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("name", gs.LEADING)
def test_strand_choice_and_scores_equal_the_restatement(ctx, strand_ref, name, model):
    sets, scores = strand_sets(), gs.scores_of(name, model)
    assert sum(1 for st in sets for k in range(len(st)) if k % 3 == 1) * 4 >= sum(len(st) for st in sets)
    for mode in MODES:
        want = wanted(("strand", name, model, mode), lambda st: strand_ref.strand_cells(st, mode, scores, None, True), sets)
        got, st = ctx.poa_strand(sets, msa=True, include_consensus=True, stats=True, **strlib.kw_of(scores, mode))
        for field in ("reversed", "scores", "consensus", "rows"):
            assert [k for k in range(len(sets)) if getattr(got[k], field) != getattr(want[k][0], field)] == [], (field, mode)
        assert st["dp_cells"] == sum(w[1] for w in want) and st["third_passes"] == sum(w[2] for w in want), mode
        if mode != "sw" or name not in gs.NOTHING_POSITIVE:
            assert st["third_passes"] > 0, mode


# ---- hx_poa_labelled
def label_sets():
    sets = [st[:12] for _, _, st in gs.CORPUS[::10]]
    labels = [[lbllib.NO_LABEL if k == 4 else k % 2 for k in range(len(st))] for st in sets]
    for seed in (31, 32):
        sq, lb = lbllib.two_haplotypes(seed, 300, 4)
        sets.append(sq); labels.append(lb)
    return sets, labels


@pytest.mark.parametrize("name", gs.LEADING)
def test_labelled_consensus_equals_the_restatement(ctx, label_ref, name):
    sets, labels = label_sets()
    for k, model in enumerate(MODELS):
        mode = MODES[(k + gs.LEADING.index(name)) % 3]
        scores = gs.scores_of(name, model)
        want = wanted(("label", name, model, mode), lambda i: label_ref.labelled_cells(sets[i], labels[i], 2, mode, scores, None, True), range(len(sets)))
        got, st = ctx.poa_labelled(sets, labels, 2, msa=True, include_consensus=True, coverage=True, profile=True, stats=True, **lbllib.kw_of(scores, mode))
        for field in ("consensus", "columns", "coverage", "profile", "rows"):
            assert [i for i in range(len(sets)) if getattr(got[i], field) != getattr(want[i][0], field)] == [], (field, model, mode)
        assert st["dp_cells"] == sum(w[1] for w in want), (model, mode)


# ---- scale invariance on the device, up to the bound
SCALE_NAME = "all_equal_negative"   # every step of a path costs: the end scores run furthest below 0


@pytest.mark.parametrize("model", MODELS)
def test_k_times_the_scores_up_to_the_bound_and_the_refusal_at_it(ctx, model):
    from haslr_amd import hip
    scores = gs.scores_of(SCALE_NAME, model)
    reach = 0.0
    for seqs in (gs.UNRELATED_PAIR, gs.NOISY_1100):
        k = (gs.SCORE_BOUND - 1) // gs.bound_product(seqs, scores, model)
        many, over = gs.scaled(scores, k), gs.scaled(scores, k + 1)
        assert gs.bound_product(seqs, many, model) < gs.SCORE_BOUND <= gs.bound_product(seqs, over, model) and k > 1000
        assert gs.columns_of(seqs, model) > 1024   # (past the 64 x 16 instance: the prefix maxima cross wavefronts)
        for mode in MODES:
            one = ctx.poa_graph([seqs], **grflib.kw_of(scores, mode))[0]
            got = ctx.poa_graph([seqs], **grflib.kw_of(many, mode))[0]
            assert gs.same_but_scores(got, one, k), (mode, k)
            assert grflib.checks(one, seqs) + grflib.rescore(one, seqs, scores, mode) == [], mode
            with pytest.raises(hip.HipError) as e:
                ctx.poa_graph([["ACGT", "ACGA"], seqs], **grflib.kw_of(over, mode))
            assert str(e.value) == gs.refusal("hx_poa_graph", 1, seqs, over, model), mode
            reach = max(reach, -min(sq.score for sq in one.sequences) * k / gs.SCORE_BOUND)
    print(f"{model} {scores}: the most negative end score x k reaches {reach:.3f} of the bound")
    assert reach > 1 / 16   # (the module's text: why not a half)


def test_the_refusal_carries_the_name_of_every_entry(ctx):
    from haslr_amd import hip
    seqs = gs.UNRELATED_PAIR
    lin, aff, cvx = (gs.scaled(gs.scores_of(SCALE_NAME, m), (gs.SCORE_BOUND - 1) // gs.bound_product(seqs, gs.scores_of(SCALE_NAME, m), m) + 1) for m in MODELS)
    calls = [("hx_poa_sequences_mode", "linear", lin, lambda: ctx.poa_sequences_mode([seqs], "ov", *lin[:3])),
             ("hx_poa_sequences_affine", "affine", aff, lambda: ctx.poa_sequences_affine([seqs], "ov", *aff[:4])),
             ("hx_poa_sequences_convex", "convex", cvx, lambda: ctx.poa_sequences_convex([seqs], "ov", *cvx)),
             ("hx_poa_msa", "affine", aff, lambda: ctx.poa_msa([seqs], **{k: v for k, v in grflib.kw_of(aff, "nw").items() if k not in ("gap_open2", "gap_extend2")})),
             ("hx_poa_msa_convex", "convex", cvx, lambda: ctx.poa_msa([seqs], **grflib.kw_of(cvx, "nw"))),
             ("hx_poa_weighted", "linear", lin, lambda: ctx.poa_weighted([seqs], **{k: v for k, v in grflib.kw_of(lin, "sw").items() if k not in ("gap_open2", "gap_extend2")})),
             ("hx_poa_weighted_convex", "convex", cvx, lambda: ctx.poa_weighted([seqs], **grflib.kw_of(cvx, "sw"))),
             ("hx_poa_strand", "affine", aff, lambda: ctx.poa_strand([seqs], **grflib.kw_of(aff, "nw"))),
             ("hx_poa_labelled", "convex", cvx, lambda: ctx.poa_labelled([seqs], [[0, 1]], 2, **grflib.kw_of(cvx, "nw"))),
             ]
    for who, model, scores, call in calls:
        with pytest.raises(hip.HipError) as e:
            call()
        assert str(e.value) == gs.refusal(who, 0, seqs, scores, model), who
    # a banded set meets its own, tighter bound first (2^28 on bases + longest sequence) unless its instance is much wider than its sequences
    wide = [seqs[0][:1024], "ACGTACGTAC"]
    scores = gs.scaled(gs.scores_of(SCALE_NAME, "linear"), 34885)
    under = gs.scaled(gs.scores_of(SCALE_NAME, "linear"), 34884)
    assert (1034 + 1024) * 3 * 34885 < 1 << 28 and gs.bound_product(wide, under, "linear") < gs.SCORE_BOUND <= gs.bound_product(wide, scores, "linear")
    with pytest.raises(hip.HipError) as e:
        ctx.poa_banded([wide], 500, **grflib.kw_of(scores, "nw"))
    assert str(e.value) == gs.refusal("hx_poa_banded", 0, wide, scores, "linear")


# ---- the consensus entries
@pytest.mark.parametrize("name", gs.LEADING)
def test_the_consensus_entries_return_the_graphs_consensus(ctx, name):
    corpus = gs.light(gs.CORPUS[:-2:3]) + gs.LONG   # (five calls per type beside the graph's three: the sets of at most 8 000 bases)
    sets = gs.sets_of(corpus)
    lin, aff, cvx = (gs.scores_of(name, m) for m in MODELS)
    for mode in MODES:
        want = {m: [r.consensus for r in ctx.poa_graph(sets, **grflib.kw_of(gs.scores_of(name, m), mode))] for m in MODELS}
        with ctx.options(poa_general=1):   # (kNW with linear gaps is the tuned path's otherwise)
            assert gs.failing(corpus, ctx.poa_sequences_mode(sets, mode, *lin[:3]), want["linear"]) == [], (mode, "mode")
            assert gs.failing(corpus, ctx.poa_sequences_affine(sets, mode, *aff[:4]), want["affine"]) == [], (mode, "affine")
            assert gs.failing(corpus, ctx.poa_sequences_convex(sets, mode, *cvx), want["convex"]) == [], (mode, "convex")
            with ctx.options(poa_affine=1):   # the linear scores on the affine kernel
                assert gs.failing(corpus, ctx.poa_sequences_affine(sets, mode, *lin[:4]), want["linear"]) == [], (mode, "linear on affine")
            with ctx.options(poa_convex=1):   # the affine scores on the convex kernel
                assert gs.failing(corpus, ctx.poa_sequences_convex(sets, mode, *aff), want["affine"]) == [], (mode, "affine on convex")
