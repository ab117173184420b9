"""hx_poa_banded on the MI355X: consensus, band_used, MSA rows, coverage, profile and dp_cells equal the CPU restatement
(tests/poa_band_ref.cpp) field by field, through each of the nine band kernels (three gap models x consensus only, node per base,
weighted): the three types under the three gap models, the lane and window edges, windows that drift far, a fan-in row with a predecessor
whose window is wholly disjoint from its own, the escalation to twice the band and to the full matrix, and both kinds of rerun together.
Only the escalation cases hold sets that miss their band; every other case asserts band_reruns == 0, so that a kernel that always falls
back to the full matrix cannot pass it."""
from concurrent.futures import ThreadPoolExecutor

import pytest

import bandlib
import wgtlib

pytestmark = pytest.mark.gpu
MODES = ["sw", "nw", "ov"]
MODELS = bandlib.MODELS
EDGE_W = [1, 7, 8, 31, 32, 511]
_wanted = {}


@pytest.fixture(scope="module")
def ref(built, tmp_path_factory):
    return bandlib.BandRef(str(tmp_path_factory.mktemp("band_gpu")))


@pytest.fixture(scope="module")
def ctx(built):
    from haslr_amd import hip
    c = hip.HipContext(0)   # raises without a device: these tests never run on a fallback
    yield c
    c.close()


def wanted(ref, key, sets, band, mode, scores, weights=None):
    """the restatement's (record, cells, band reruns) per set, computed once per key and left unchanged"""
    if key not in _wanted:
        with ThreadPoolExecutor(16) as ex:   # (the restatement releases the GIL: ctypes)
            _wanted[key] = list(ex.map(lambda k: ref.banded_cells(sets[k], band, mode, scores, None if weights is None else weights[k], True), range(len(sets))))
    return _wanted[key]


def assert_equal(ctx, want, sets, band, mode, scores, variant, weights=None, qualities=None):
    """one call through the band kernel of the scores' gap model and of `variant` ("consensus": the consensus alone; "nodes": the node of
    every base kept, for the rows, the coverage and the profile; "weighted": the same under weights), every field it returns against the
    restatement's, and the counters; returns (records, counters)"""
    assert (variant == "weighted") == (weights is not None or qualities is not None)
    full = variant != "consensus"
    got, st = ctx.poa_banded(sets, band, weights=weights, qualities=qualities, msa=full, include_consensus=full, coverage=full, profile=full, stats=True, **bandlib.kw_of(scores, mode))
    assert len(got) == len(sets)
    for field in ("consensus", "band_used") + (("rows", "coverage", "profile") if full else ()):
        assert [k for k in range(len(sets)) if getattr(got[k], field) != getattr(want[k][0], field)] == [], (field, mode, scores, variant)
    assert st["dp_cells"] == sum(w[1] for w in want)
    assert st["band_reruns"] == sum(w[2] for w in want)
    assert st["seq_bases"] == sum(len(q) for s in sets for q in s) and st["n_aligned"] == sum(1 for s in sets for q in s if q)
    return got, st


@pytest.mark.parametrize("model", list(MODELS))
@pytest.mark.parametrize("mode", MODES)
def test_the_three_types_under_the_three_gap_models(ctx, ref, mode, model):
    sets = [bandlib.copies(500 + k, 300, 6, 0.06) for k in range(4)]
    weights = wgtlib.uniform_weights(sets, 510)
    for variant, w in (("consensus", None), ("nodes", None), ("weighted", weights)):
        want = wanted(ref, ("types", mode, model, variant == "weighted"), sets, 16, mode, MODELS[model], w)
        got, st = assert_equal(ctx, want, sets, 16, mode, MODELS[model], variant, w)
        assert st["band_reruns"] == 0 and all(r.band_used == 16 for r in got)


def edge_sets(w):
    """around a window of B = 2 w + 1 columns: sets whose longest sequence has L + 1 = B - 1 and B (they fit the window: the full matrix)
    and B + 1 (banded), the banded one with members shorter than the window, a sequence of one base and empty sequences; and sets without
    a base"""
    B = 2 * w + 1
    out = []
    for L in (B - 2, B - 1, B):
        st = bandlib.exact_copies(600 + w + L, L, 4, 0.05)
        if L >= 3:
            st = st[:2] + [st[2][:L - 2], "", st[3][:L - 1], st[0][:1], st[1]]
        out.append(st)
    return out + [[""], [], ["", ""]]


@pytest.mark.parametrize("w", EDGE_W)
def test_lane_and_window_edges(ctx, ref, w):
    sets = edge_sets(w)
    B = 2 * w + 1
    for mode, model, variant in (("nw", "linear", "nodes"), ("ov", "affine", "consensus"), ("sw", "convex", "nodes")):
        want = wanted(ref, ("edges", w, mode, model), sets, w, mode, MODELS[model])
        got, st = assert_equal(ctx, want, sets, w, mode, MODELS[model], variant)
        assert st["band_reruns"] == 0
        assert [r.band_used for r in got] == [0, 0, w, 0, 0, 0]   # (only the set whose longest sequence + 1 is B + 1 does not fit the window)
        assert max(len(q) for q in sets[2]) + 1 == B + 1


@pytest.mark.parametrize("mode,model", [("nw", "linear"), ("ov", "convex")])
def test_windows_that_drift(ctx, ref, mode, model):
    sets = [bandlib.copies(11, 3000, 8, 0.10)]
    want = wanted(ref, ("drift", mode, model), sets, 64, mode, MODELS[model])
    got, st = assert_equal(ctx, want, sets, 64, mode, MODELS[model], "nodes")
    assert st["band_reruns"] == 0 and got[0].band_used == 64
    assert st["dp_cells"] < sum(len(q) for q in sets[0]) * 129 * 2   # (the window's columns, not the sequences')


@pytest.mark.parametrize("model", list(MODELS))
def test_a_predecessor_wholly_outside_the_window(ctx, ref, model):
    sets = [bandlib.two_branch_set(700 + k) for k in range(3)]
    scores = bandlib.TWO_BRANCH[model]
    want = wanted(ref, ("branch", model), sets, 8, "nw", scores)
    got, st = assert_equal(ctx, want, sets, 8, "nw", scores, "nodes")
    assert st["band_reruns"] == 0 and all(r.band_used == 8 for r in got)
    # the band lost nothing: the full matrix gives the same rows (the T branch in columns of its own, rejoined behind it)
    full = wanted(ref, ("branch-full", model), sets, 0, "nw", scores)
    assert [r.rows for r in got] == [w[0].rows for w in full]
    assert all("T" * 150 in r.rows[0] and "-" * 150 in r.rows[1] and "T" * 150 in r.rows[2] and "-" * 150 in r.rows[3] for r in got)


@pytest.mark.parametrize("model", list(MODELS))
def test_escalation_and_the_last_rung(ctx, ref, model):
    sets = [bandlib.ESC_SET, bandlib.LAST_RUNG_SET, bandlib.copies(800, 300, 4, 0.05)]
    want = wanted(ref, ("esc", model), sets, 8, "nw", MODELS[model])
    for variant in ("consensus", "nodes"):
        got, st = assert_equal(ctx, want, sets, 8, "nw", MODELS[model], variant)
        assert [r.band_used for r in got] == [32, 0, 8] and st["band_reruns"] == 2 + 6   # (8 -> 16 -> 32; 8 -> ... -> 256 -> the full matrix)
    want64 = wanted(ref, ("esc64", model), sets[:1], 64, "nw", MODELS[model])
    got, st = assert_equal(ctx, want64, sets[:1], 64, "nw", MODELS[model], "nodes")
    assert got[0].band_used == 64 and st["band_reruns"] == 0


def test_both_reruns_together(ctx, ref):
    sets = [bandlib.ESC_SET, bandlib.copies(801, 300, 4, 0.05)]
    weights = wgtlib.uniform_weights(sets, 802)
    want = wanted(ref, ("both",), sets, 8, "nw", bandlib.AFFINE, weights)
    got, st = assert_equal(ctx, want, sets, 8, "nw", bandlib.AFFINE, "weighted", weights)
    with ctx.options(poa_modes_slot_kb=1):
        again, st2 = assert_equal(ctx, want, sets, 8, "nw", bandlib.AFFINE, "weighted", weights)
    assert again == got and st["slot_reruns"] == 0 and st2["slot_reruns"] > 0 and st2["band_reruns"] == st["band_reruns"] == 2


@pytest.mark.parametrize("model", list(MODELS))
def test_weights_and_qualities(ctx, ref, model):
    sets = [bandlib.copies(900 + k, 200, 5, 0.05) for k in range(3)]
    weights = wgtlib.quality_weights(sets, 903)
    want = wanted(ref, ("weights", model), sets, 12, "ov", MODELS[model], weights)
    got, st = assert_equal(ctx, want, sets, 12, "ov", MODELS[model], "weighted", weights)
    assert st["band_reruns"] == 0
    quals = [wgtlib.quality_strings(ws) for ws in weights]
    assert assert_equal(ctx, want, sets, 12, "ov", MODELS[model], "weighted", qualities=quals)[0] == got


def test_identical_sequences_at_the_narrowest_band(ctx):
    t = bandlib.template(__import__("random").Random(950), 500)
    got, st = ctx.poa_banded([[t] * 5], 1, msa=True, stats=True)
    assert got[0].consensus == t and got[0].band_used == 1 and got[0].rows == [t] * 5
    assert st["band_reruns"] == 0 and st["dp_cells"] == 4 * 500 * 3


def test_the_workspace_is_the_windows(ctx):
    sets = [bandlib.copies(960, 2000, 4, 0.05)]
    _, banded = ctx.poa_banded(sets, 64, stats=True)
    _, wide = ctx.poa_banded(sets, 511, stats=True)
    assert 0 < banded["workspace_bytes"] < wide["workspace_bytes"]


def test_errors_carry_the_entrys_name(ctx):
    from haslr_amd import hip
    for band in (0, 512):
        with pytest.raises(hip.HipError, match=f"hx_poa_banded: the band half-width must be 1..511, not {band}"):
            ctx.poa_banded([["ACGT"]], band)
    with pytest.raises(hip.HipError, match=r"hx_poa_banded: set 1 holds 60000 bases, its longest sequence 30000: with scores of up to 3000 their product 270000000 reaches 2\^28 = 268435456"):
        ctx.poa_banded([["ACGT"], ["A" * 30000] * 2], 8, match=5, mismatch=-4, gap_open=-3000)
    with pytest.raises(hip.HipError, match="hx_poa_banded: set 0 holds a sequence of 8192 bases, longer than 8191"):
        ctx.poa_banded([["A" * 8192]], 8, **bandlib.kw_of(bandlib.CONVEX, "nw"))
    with pytest.raises(hip.HipError, match="hx_poa_banded: the gap open score must be negative, not 0"):
        ctx.poa_banded([["ACGT"]], 8, gap_open=0)
