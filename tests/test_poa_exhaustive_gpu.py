"""hx_poa_graph and hx_poa_strand on the MI355X, their end scores held to an exhaustive optimum: the score of a sequence against the graph
it was aligned to is the maximum, over the graph's source-to-sink paths, of a plain pairwise DP against the path's letters (tests/exhlib.py,
tests/pairwise_ref.cpp), which shares no loop over predecessors and no sink flag with the kernels or their restatements. The optimum is
computed once per (inputs, type, scores) on the CPU from the restatement's record and never from the kernel's output; the kernel's record
must be the restatement's (so that the graphs are the same ones) and its scores the optima. The inputs are tests/exhsets.py's, which
tests/test_poa_exhaustive_ref.py shows to branch and to stay under the path cap: tiny branching sets, a column of fan-in 7 and more, long
gaps across a bubble, the lane edges of the 64-lane instance, the sets of the structured corpus that stay under the cap, and one set per workgroup width.
Every call runs once more with workspace slots capped, so that the rerun in a larger slot is covered."""
import contextlib

import pytest

import exhlib
import exhsets as xs
import grflib
import strlib

pytestmark = pytest.mark.gpu
DEFAULT = {"linear": grflib.LINEAR, "affine": grflib.AFFINE, "convex": grflib.CONVEX}


@pytest.fixture(scope="module")
def refs(built, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("exh_gpu"))
    return exhlib.Reference(grflib.GraphRef(d), strlib.StrandRef(d), exhlib.Pairwise(d))


@pytest.fixture(scope="module")
def ctx(built):
    from haslr_amd import hip
    c = hip.HipContext(0)   # raises without a device: these tests never run on a fallback
    yield c
    c.close()


def capped(ctx, on):
    return ctx.options(poa_modes_slot_kb=1) if on else contextlib.nullcontext()


def graph_differences(ctx, refs, inputs, mode, scores, slots_capped):
    """(the sets whose record is not the restatement's, the (family, index, sequence, score, optimum) that differ, the counters)"""
    want, optima = refs.graph(inputs, mode, scores)
    n, _, _, over = exhlib.tally_graph(optima)
    assert over == [] and n > 0
    with capped(ctx, slots_capped):
        got, st = ctx.poa_graph([c[2] for c in inputs], stats=True, **grflib.kw_of(scores, mode))
    assert len(got) == len(inputs)
    unlike = [(f, i) for (f, i, _), a, b in zip(inputs, got, want) if not grflib.same(a, b)]
    off = [(f, i, k, rec.sequences[k].score, o) for (f, i, _), rec, per in zip(inputs, got, optima) for k, o in enumerate(per)
           if rec.sequences[k].score != (0 if o is None else o[0])]
    return unlike, off, st


@pytest.mark.parametrize("model", xs.MODELS)
@pytest.mark.parametrize("mode", xs.MODES)
def test_every_score_of_poa_graph_is_the_optimum_over_the_paths(ctx, refs, mode, model):
    inputs = xs.INPUTS + xs.EXCLUDED
    for scores in xs.SCORES_OF_MODEL[model]:
        for slots_capped in (False, True):
            unlike, off, st = graph_differences(ctx, refs, inputs, mode, scores, slots_capped)
            assert unlike == [], (mode, scores, slots_capped)
            assert off == [], (mode, scores, slots_capped)
            assert not slots_capped or st["slot_reruns"] > 0


@pytest.mark.parametrize("lanes,model,lmax,mode,st", xs.WIDTHS, ids=[f"{w[0]}-{w[1]}-{w[2]}-{w[3]}" for w in xs.WIDTHS])
def test_one_set_per_workgroup_width(ctx, refs, lanes, model, lmax, mode, st):
    for slots_capped in (False, True):
        unlike, off, _ = graph_differences(ctx, refs, [("width", lanes, st)], mode, DEFAULT[model], slots_capped)
        assert unlike == [] and off == [], (lanes, slots_capped)


@pytest.mark.parametrize("model", xs.MODELS)
@pytest.mark.parametrize("mode", xs.MODES)
def test_both_scores_of_poa_strand_are_optima_over_the_paths_of_the_rows(ctx, refs, mode, model):
    inputs = xs.STRAND_INPUTS
    sets = [c[2] for c in inputs]
    for scores in xs.SCORES_OF_MODEL[model]:
        want, optima = refs.strand(inputs, xs.rc, mode, scores)
        n, _, _, over = exhlib.tally_strand(optima)
        assert over == [] and n > 0
        for slots_capped in (False, True):
            with capped(ctx, slots_capped):
                got, st = ctx.poa_strand(sets, msa=True, include_consensus=False, stats=True, **strlib.kw_of(scores, mode))
            assert len(got) == len(sets)
            # the rows are the restatement's: the optima were computed on the graphs that these rows hold
            assert [(f, i) for (f, i, _), a, b in zip(inputs, got, want) if a.rows != b.rows] == [], (mode, scores, slots_capped)
            off = [(f, i, k, rec.scores[k], o) for (f, i, _), rec, per in zip(inputs, got, optima) for k, o in enumerate(per) if rec.scores[k] != ((0, 0) if o is None else o[0])]
            assert off == [], (mode, scores, slots_capped)
            # reversed exactly where the reverse complement scores strictly higher, and both branches run
            assert all(rec.reversed[k] == (f < r) for rec in got for k, (f, r) in enumerate(rec.scores)), (mode, scores, slots_capped)
            flags = sum(f for rec in got for f in rec.reversed)
            assert st["third_passes"] == flags and (max(scores) <= 0 or 4 * flags >= n)
            assert not slots_capped or st["slot_reruns"] > 0
