"""Gaps across lane, wave and instance boundaries of the general POA path's row loop (kernels/poa_modes_dp.inl) on the MI355X. A set of two
sequences: a seeded template of W + 76 bases over A, C, G, and the template with 48 T inserted after base W - 24. The inserted bases match
nothing, so they must come out as one horizontal gap at sequence positions W-24 ... W+23, across column W: for W = 1024, 2048, 4096 and
8192 that is a wave boundary of every instance that takes these lengths (a wave owns 64 lanes x 16 or 32 columns), and the gap crosses
three lane boundaries as well; the lengths lie just past the longest sequence of one instance, so the next one runs. Linear, affine and
convex gaps (convex stops at 8 191 bases: no W = 8192) in the three modes: consensus and dp_cells equal the CPU restatement's, the
restatement's last alignment holds exactly that one run of 48 pairs without a node, and the rows of the MSA show the same gap."""
import functools
import random

import pytest

import cvxlib
import parlib
import pmrlib

pytestmark = pytest.mark.gpu
MODES = ["sw", "nw", "ov"]
INS = 48
SCORES = {"linear": (5, -12, -3), "affine": (5, -4, -8, -6), "convex": (5, -4, -8, -6, -10, -4)}   # (convex: the second piece prices the gap)
CASES = [(model, W) for model in SCORES for W in (1024, 2048, 4096, 8192) if not (model == "convex" and W == 8192)]


@pytest.fixture(scope="module")
def refs(built, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("row_boundaries"))
    return {"linear": pmrlib.ModesRef(d), "affine": parlib.AffineRef(d), "convex": cvxlib.ConvexRef(d)}


@pytest.fixture(scope="module")
def ctx(built):
    from haslr_amd import hip
    c = hip.HipContext(0)   # raises without a device: these tests never run on a fallback
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def pair(W):
    rnd = random.Random(4000 + W)
    t = "".join(rnd.choice("ACG") for _ in range(W + 76))
    return t, t[:W - 24] + "T" * INS + t[W - 24:]


def gap_runs(aln):
    """the maximal runs of consecutive pairs without a node, each as (pairs, first position, last position)"""
    runs, cur = [], []
    for node, pos in list(aln) + [(0, 0)]:
        if node == -1:
            cur.append(pos)
        elif cur:
            runs.append((len(cur), min(cur), max(cur)))
            assert sorted(cur) == list(range(min(cur), max(cur) + 1))
            cur = []
    return runs


def wanted(refs, model, W, mode):
    """(consensus, dp_cells, gap runs of the last alignment) by the CPU restatements"""
    seqs, sc = list(pair(W)), SCORES[model]
    cns, cells = refs[model].consensus_cells(seqs, mode, sc) if model == "convex" else refs[model].consensus_cells(seqs, mode, *sc)
    if model == "linear":   # (its alignment is asked of the convex restatement, with the gap score given four times)
        assert refs["convex"].consensus_cells(seqs, mode, sc[:2] + (sc[2],) * 4) == (cns, cells)
    return cns, cells, gap_runs(refs["convex" if model == "linear" else model].last_alignment())


def gpu_consensus(ctx, model, seqs, mode):
    sc = SCORES[model]
    if model == "linear":
        with ctx.options(poa_general=1):   # (kNW with linear gaps is the tuned path's otherwise)
            return ctx.poa_sequences_mode([seqs], mode, *sc, stats=True)
    return (ctx.poa_sequences_affine if model == "affine" else ctx.poa_sequences_convex)([seqs], mode, *sc, stats=True)


def gpu_msa(ctx, model, seqs, mode):
    sc = SCORES[model]
    kw = dict(zip(("match", "mismatch", "gap_open", "gap_extend", "gap_open2", "gap_extend2"), sc))
    return ctx.poa_msa([seqs], mode, **kw)[0]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("model,W", CASES)
def test_an_insertion_across_column_w_is_one_horizontal_gap(ctx, refs, model, W, mode):
    seqs = list(pair(W))
    cns, cells, runs = wanted(refs, model, W, mode)
    assert runs == [(INS, W - 24, W + 23)], (model, W, mode)
    got, st = gpu_consensus(ctx, model, seqs, mode)
    assert got == [cns], (model, W, mode)
    assert st["dp_cells"] == cells == (W + 76) * (W + 76 + INS)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("model,W", CASES)
def test_the_msa_rows_show_the_same_gap(ctx, model, W, mode):
    seqs = list(pair(W))
    first, second = gpu_msa(ctx, model, seqs, mode)
    assert len(first) == len(second)
    gaps = [k for k, ch in enumerate(first) if ch == "-"]
    assert gaps == list(range(W - 24, W + 24)), (model, W, mode)
    assert [k for k, ch in enumerate(second) if ch == "-"] == [] and "".join(second[k] for k in gaps) == "T" * INS
    assert first.replace("-", "") == seqs[0] and second == seqs[1]
