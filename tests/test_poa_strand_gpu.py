"""hx_poa_strand on the MI355X: consensus, flags, both scores, MSA rows, coverage and profile equal the CPU restatement
(tests/poa_strand_ref.cpp) bit for bit - on the hand-derived cases, on seeded sets with half of the members on the other strand at the
lane and instance edges of reversed indexing (1, 15, 16, 17, 1022, 1023, 1024 bases; 4 100; 2 100 under convex gaps: the restatement's
five full matrices make 8 191 bases take too long), on short two-letter sets whose orientations tie, in three modes under the three gap
models, with and without weights, and with workspace slots capped so that sets are rerun. With the existing GPU path as second witness: a
set without reversed members is poa_msa's and poa_weighted's, one with reversed members is theirs on the set oriented beforehand."""
from concurrent.futures import ThreadPoolExecutor

import pytest

import strlib
import wgtlib

pytestmark = pytest.mark.gpu
MODES = ["sw", "nw", "ov"]
MODELS = {"linear": strlib.LINEAR, "affine": strlib.AFFINE, "convex": strlib.CONVEX}
MAX_LEN = {"linear": 32767, "affine": 16383, "convex": 8191}
HAND = [[strlib.S1, strlib.rc(strlib.S1)], [strlib.PALINDROME] * 2, ["AAAA", "CCCC"], ["AAAA", "TTTT"], strlib.FOUR, ["ACAGATT", "ANTCTGT"], [strlib.WA, strlib.rc(strlib.WV)]]
EMPTY = [["", "AACGT", "", strlib.rc("AACGA"), "G"], [], [""], ["", ""], ["A"], ["A", "T"]]
CORPUS = strlib.edge_sets(301) + strlib.tie_sets(302, 30) + HAND + EMPTY
_wanted = {}


@pytest.fixture(scope="module")
def ref(built, tmp_path_factory):
    return strlib.StrandRef(str(tmp_path_factory.mktemp("str_gpu")))


@pytest.fixture(scope="module")
def ctx(built):
    from haslr_amd import hip
    c = hip.HipContext(0)   # raises without a device: these tests never run on a fallback
    yield c
    c.close()


def wanted(ref, key, sets, mode, scores, weights=None):
    """the restatement's (record, cells, third passes) per set, computed once per key and left unchanged"""
    if key not in _wanted:
        with ThreadPoolExecutor(16) as ex:   # (the restatement releases the GIL: ctypes)
            _wanted[key] = list(ex.map(lambda k: ref.strand_cells(sets[k], mode, scores, None if weights is None else weights[k], True), range(len(sets))))
    return _wanted[key]


def assert_equal(ctx, want, sets, mode, scores, weights=None):
    """every array of the call against the restatement's, set by set, and the counters; returns (records, counters)"""
    got, st = ctx.poa_strand(sets, weights=weights, msa=True, include_consensus=True, coverage=True, profile=True, stats=True, **strlib.kw_of(scores, mode))
    assert len(got) == len(sets)
    for field in ("reversed", "scores", "consensus", "rows", "coverage", "profile"):
        assert [k for k in range(len(sets)) if getattr(got[k], field) != getattr(want[k][0], field)] == [], (field, mode, scores)
    assert st["dp_cells"] == sum(w[1] for w in want)
    assert st["third_passes"] == sum(w[2] for w in want) == sum(sum(r.reversed) for r in got)
    assert st["seq_bases"] == sum(len(q) for s in sets for q in s) and st["n_aligned"] == sum(1 for s in sets for q in s if q)
    return got, st


@pytest.mark.parametrize("model", list(MODELS))
@pytest.mark.parametrize("mode", MODES)
def test_every_array_equals_the_restatement(ctx, ref, mode, model):
    want = wanted(ref, (mode, model), CORPUS, mode, MODELS[model])
    got, st = assert_equal(ctx, want, CORPUS, mode, MODELS[model])
    assert st["third_passes"] >= 14   # (every seeded set has its second member on the other strand: the third pass runs)
    # sets rerun in larger slots rewrite their part of the flags and the scores and reach the same
    with ctx.options(poa_modes_slot_kb=1):
        again, st2 = assert_equal(ctx, want, CORPUS, mode, MODELS[model])
    assert st2["slot_reruns"] > 0 and again == got
    # the option that names the one-matrix route: the route there is, whatever its value
    for v in (1, 0):
        with ctx.options(poa_strand_one_h=v):
            assert ctx.poa_strand(CORPUS[:8], **strlib.kw_of(MODELS[model], mode)) == [r._replace(rows=None, coverage=None, profile=None) for r in got[:8]]


@pytest.mark.parametrize("model", list(MODELS))
@pytest.mark.parametrize("mode", MODES)
def test_every_array_equals_the_restatement_under_weights(ctx, ref, mode, model):
    sets = strlib.edge_sets(303) + strlib.tie_sets(304, 10) + [[strlib.WA, strlib.rc(strlib.WV)]] + EMPTY
    weights = wgtlib.uniform_weights(sets[:-7], 305) + [strlib.W_WEIGHTS] + wgtlib.quality_weights(EMPTY, 306)
    want = wanted(ref, (mode, model, "w"), sets, mode, MODELS[model], weights)
    got, _ = assert_equal(ctx, want, sets, mode, MODELS[model], weights)
    if mode == "nw":
        assert got[-7].consensus == "ACGTTGCAAGGCTATGCAGG" and got[-7].reversed == [False, True]   # (the hand-derived answer: the weights went round with the sequence)
    with ctx.options(poa_modes_slot_kb=1):
        assert assert_equal(ctx, want, sets, mode, MODELS[model], weights)[0] == got
    quals = [wgtlib.quality_strings(ws) for ws in wgtlib.quality_weights(sets[:6], 307)]
    assert ctx.poa_strand(sets[:6], qualities=quals, **strlib.kw_of(MODELS[model], mode)) == ctx.poa_strand(sets[:6], weights=wgtlib.quality_weights(sets[:6], 307), **strlib.kw_of(MODELS[model], mode))


@pytest.mark.parametrize("model,length", [("linear", 4100), ("affine", 4100), ("convex", 2100)])
def test_a_long_set(ctx, ref, model, length):
    sets = [strlib.long_set(308, length)]
    for mode in ("nw", "ov"):
        want = wanted(ref, (mode, model, length), sets, mode, MODELS[model])
        got, _ = assert_equal(ctx, want, sets, mode, MODELS[model])
        assert got[0].reversed[1]


def test_the_corpus_holds_real_ties_between_the_orientations(ref):
    # (on the restatement: the inputs are fixed by what it shows)
    want = wanted(ref, ("nw", "linear"), CORPUS, "nw", strlib.LINEAR)
    ties = [(f, r) for rec, _, _ in want for f, r in rec.scores if f == r != 0]
    assert len(ties) >= 1 and all(not rec.reversed[k] for rec, _, _ in want for k, (f, r) in enumerate(rec.scores) if f == r)


def test_the_known_answers(ctx):
    got = ctx.poa_strand(HAND[:6], msa=True)
    assert [r.reversed for r in got] == [[False, True], [False, False], [False, False], [False, True], [False, True, False, True], [False, True]]
    assert got[0].consensus == strlib.S1 and got[0].rows == [strlib.S1] * 2 and got[0].scores[1][1] == 85
    assert got[1].scores == [(0, 0), (30, 30)]
    assert got[2].rows == ["AAAA", "CCCC"] and got[2].scores == [(0, 0), (-16, -16)]   # (global: four mismatches either way, a tie, forward)
    assert got[3].rows == ["AAAA", "AAAA"] and got[3].scores[1] == (-16, 20)
    sw = ctx.poa_strand(HAND[2:4], type="sw", msa=True)
    assert [r.scores[1] for r in sw] == [(0, 0), (0, 20)] and sw[0].rows == ["AAAA----", "----CCCC"] and not any(sw[0].reversed)
    assert got[5].rows == ["ACAGATT"] * 2


def test_aligned_as_given_the_reversed_members_bend_the_consensus(ctx):
    # the behavioural witness: the same set through the entry that knows no strands
    kw = dict(match=5, mismatch=-4, gap_open=-8, gap_extend=-6, gap_open2=-10, gap_extend2=-4)
    raw = ctx.poa_sequences_convex([strlib.FOUR], type="nw", **kw)[0]
    rec = ctx.poa_strand([strlib.FOUR], type="nw", **kw)[0]
    assert raw == "TCATGGCCTGAATATTCAGGTCAACGA" and rec.consensus == "ACGTTGCAAGGCTATTCAGGTCCATGA" == strlib.F0
    assert rec.reversed == [False, True, False, True]


@pytest.mark.parametrize("model", list(MODELS))
def test_the_existing_entries_are_the_second_witness(ctx, model):
    sets = strlib.edge_sets(309) + strlib.tie_sets(310, 20)
    weights = wgtlib.quality_weights(sets, 311)
    for mode in MODES:
        kw = strlib.kw_of(MODELS[model], mode)
        if model != "convex":
            kw.pop("gap_open2"), kw.pop("gap_extend2")
        got, st = ctx.poa_strand(sets, weights=weights, msa=True, coverage=True, profile=True, stats=True, **kw)
        assert any(any(r.reversed) for r in got) and any(not any(r.reversed) for r in got)
        pre = [strlib.oriented(s, r.reversed) for s, r in zip(sets, got)]
        pre_w = [strlib.oriented_weights(w, r.reversed) for w, r in zip(weights, got)]
        cns, cov, prof, wst = ctx.poa_weighted(pre, weights=pre_w, coverage=True, profile=True, stats=True, **kw)
        assert ctx.poa_msa(pre, **kw) == [r.rows for r in got]
        assert (cns, cov, prof) == ([r.consensus for r in got], [r.coverage for r in got], [r.profile for r in got])
        assert st["dp_cells"] == 2 * wst["dp_cells"]
        # oriented beforehand, nothing is reversed and nothing else changes
        again, st2 = ctx.poa_strand(pre, weights=pre_w, msa=True, coverage=True, profile=True, stats=True, **kw)
        assert st2["third_passes"] == 0 and [r._replace(scores=None) for r in again] == [r._replace(scores=None, reversed=[False] * len(r.reversed)) for r in got]
        assert [[f for f, _ in r.scores] for r in again] == [[max(p) for p in r.scores] for r in got]


def test_empty_sequences_and_sets_are_accepted(ctx):
    assert ctx.poa_strand([]) == []
    got, st = ctx.poa_strand(EMPTY, msa=True, include_consensus=True, coverage=True, stats=True)
    assert [r.consensus for r in got] == ["AACGT", "", "", "", "A", "A"] and got[0].reversed == [False, False, False, True, False]
    assert got[0].rows == ["-----", "AACGT", "-----", "AACGA", "---G-", "AACGT"] and got[0].scores[3] == (-5, 16)
    assert got[1].rows == [""] and got[2].rows == ["", ""] and got[5].rows == ["A", "A", "A"] and got[5].reversed == [False, True]
    assert st["n_aligned"] == 6


def test_errors_carry_the_entrys_name(ctx):
    from haslr_amd import hip
    for model, L in MAX_LEN.items():
        with pytest.raises(hip.HipError, match=rf"hx_poa_strand: set 1 holds a sequence of {L + 1} bases, longer than {L}"):
            ctx.poa_strand([["ACGT"], ["ACGT", "A" * (L + 1)]], **strlib.kw_of(MODELS[model], "nw"))
    with pytest.raises(hip.HipError, match="hx_poa_strand: the second gap open score -7 is above the first gap open score -8"):
        ctx.poa_strand([["ACGT"]], gap_open=-8, gap_extend=-6, gap_open2=-7, gap_extend2=-4)
    with pytest.raises(hip.HipError, match="hx_poa_strand: the gap open score must be negative, not 0"):
        ctx.poa_strand([["ACGT"]], gap_open=0)
    with pytest.raises(hip.HipError, match="hx_poa_strand: the gap extend score -9 is below the gap open score -8"):
        ctx.poa_strand([["ACGT"]], gap_open=-8, gap_extend=-9)
