"""hx_poa_graph on the MI355X: every array of the graph and alignment output equals the CPU restatement (tests/poa_graph_ref.cpp) element
for element - on the CPU tests' sets and the structured corpus in three modes under the score sets of the MSA and the convex tests, with
and without weights, on calls of 2 000 sets that run every instance and the persistent workgroups, with workspace slots capped so that
sets are rerun in larger ones, with the alignment pool capped so that sets are rerun with the exact room, and on the smallest shapes at
which the code can still go wrong (below). Without the restatement: the record's invariants hold on the GPU output, its rows are
poa_msa's, its consensus and counters the consensus entries', errors carry the entry's name, and header callers write DOT and GFA that
parse back to the graph the Python call returns."""
import os
import random
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import grflib
import poasets
import wgtlib
from test_poa_affine_gpu import many_sets as many_sets_affine
from test_poa_convex_gpu import many_sets as many_sets_convex
from test_poa_modes_gpu import many_sets
from test_poa_modes_ref import SETS, noisy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
MODES = ["sw", "nw", "ov"]
# the score sets of tests/test_poa_msa_gpu.py (linear, affine: one piece) and tests/test_poa_convex_gpu.py, as six scores
SCORES = [(5, -4, -8, -8, -8, -8), (3, -5, -4, -4, -4, -4), (5, -4, -8, -2, -8, -2), (3, -5, -4, 0, -4, 0),
          (5, -4, -8, -6, -10, -4), (5, -4, -8, -6, -24, -1), (2, -7, -2, -2, -9, 0), (1, -1, -3, -2, -5, -1)]
MAX_LEN = {0: 32767, 1: 16383, 2: 8191}   # the longest sequence by gap model (include/haslr_hip.h)


@pytest.fixture(scope="module")
def ref(built, tmp_path_factory):
    return grflib.GraphRef(str(tmp_path_factory.mktemp("grf_gpu")))


@pytest.fixture(scope="module")
def ctx(built):
    from haslr_amd import hip
    c = hip.HipContext(0)   # raises without a device: these tests never run on a fallback
    yield c
    c.close()


def pmap(fn, items, threads=16):
    with ThreadPoolExecutor(threads) as ex:   # (the restatement releases the GIL: ctypes)
        return list(ex.map(fn, items))


def assert_equal(ctx, ref, sets, mode, scores, weights=None, tag=None):
    """the call's records against the restatement's, set by set, and the cell count; returns (records, counters, the restatement's records)"""
    want = pmap(lambda k: ref.graph_cells(sets[k], mode, scores, None if weights is None else weights[k]), range(len(sets)))
    got, st = ctx.poa_graph(sets, weights=weights, stats=True, **grflib.kw_of(scores, mode))
    assert len(got) == len(sets)
    bad = [k for k in range(len(sets)) if not grflib.same(got[k], want[k][0])]
    assert bad == [], (tag or (mode, scores), bad[:10])
    assert st["dp_cells"] == sum(w[1] for w in want)
    assert st["seq_bases"] == sum(len(q) for s in sets for q in s) and st["n_aligned"] == sum(1 for s in sets for q in s if q)
    return got, st, [w[0] for w in want]


@pytest.mark.parametrize("si", range(len(SCORES)))
@pytest.mark.parametrize("mode", MODES)
def test_graph_equals_the_restatement_on_the_cpu_sets(ctx, ref, mode, si):
    sets = SETS if si in (0, 2, 4) else SETS[:120]
    assert_equal(ctx, ref, sets, mode, SCORES[si])
    ws = sets[:100]
    assert_equal(ctx, ref, ws, mode, SCORES[si], wgtlib.quality_weights(ws, 50 + si) if si % 2 else wgtlib.uniform_weights(ws, 50 + si))


@pytest.mark.parametrize("si", range(len(SCORES)))
@pytest.mark.parametrize("mode", MODES)
def test_graph_equals_the_restatement_on_the_structured_corpus(ctx, ref, mode, si):
    part = poasets.sub_sample(4, si % 4)   # (a sample: the whole corpus takes the restatement too long; the eight score sets cover it twice)
    sets = [st for _, _, st in part]
    want = pmap(lambda st: ref.graph(st, mode, SCORES[si]), sets)
    got = ctx.poa_graph(sets, **grflib.kw_of(SCORES[si], mode))
    assert [(f, k) for (f, k, _), a, b in zip(part, got, want) if not grflib.same(a, b)] == []
    few = sets[:12]
    assert_equal(ctx, ref, few, mode, SCORES[si], wgtlib.uniform_weights(few, 60 + si))


@pytest.mark.parametrize("model", ["linear", "affine", "convex"])
@pytest.mark.parametrize("mode", MODES)
def test_two_thousand_sets_in_one_call(ctx, ref, mode, model):
    sets, scores = {"linear": (many_sets(42, 2000), SCORES[0]), "affine": (many_sets_affine(43, 2000), grflib.AFFINE), "convex": (many_sets_convex(44, 2000), SCORES[4])}[model]
    assert grflib.model_of(scores) == ["linear", "affine", "convex"].index(model)
    _, st, _ = assert_equal(ctx, ref, sets, mode, scores)
    assert st["aln_reruns"] <= len(sets) // 100   # (the default estimate holds: noisy copies at a tenth of errors stay inside it)


@pytest.mark.parametrize("mode", MODES)
def test_sets_rerun_in_larger_slots_give_the_same_graph(ctx, ref, mode):
    for sets, scores in ((many_sets(45, 300), SCORES[0]), (many_sets_convex(45, 300), SCORES[4])):
        with ctx.options(poa_modes_slot_kb=1):   # (first-round slots hold little more than the graph pools: sets stop and are rerun)
            _, st, _ = assert_equal(ctx, ref, sets, mode, scores)
        assert st["slot_reruns"] > 0


@pytest.mark.parametrize("model", [0, 1, 2])
@pytest.mark.parametrize("mode", MODES)
def test_sets_whose_alignments_outgrow_their_share_are_rerun_once_with_the_exact_room(ctx, ref, mode, model):
    sets = (many_sets, many_sets_affine, many_sets_convex)[model](46, 300) + [[], [""], ["ACGT"], ["A", "C"]]
    scores = (SCORES[0], SCORES[2], SCORES[4])[model]
    with ctx.options(poa_graph_aln_cap=1):   # (the smallest share: every set whose alignments hold two pairs or more outgrows it)
        _, st, want = assert_equal(ctx, ref, sets, mode, scores)
    assert st["aln_reruns"] == sum(1 for r in want if sum(len(sq.alignment) for sq in r.sequences) > 1) > 100
    with ctx.options(poa_graph_aln_cap=1, poa_modes_slot_kb=1):   # (both reasons: a set can come back for one, then for the other)
        _, st2, _ = assert_equal(ctx, ref, sets, mode, scores)
    assert st2["aln_reruns"] == st["aln_reruns"] and st2["slot_reruns"] > 0
    with ctx.options(poa_graph_aln_cap=40):   # (some sets fit, some do not)
        _, st3, _ = assert_equal(ctx, ref, sets, mode, scores)
    assert 0 < st3["aln_reruns"] < st["aln_reruns"]


# ---- the smallest shapes at which this code can still go wrong
def test_node_edge_and_pair_counts_at_the_gathers_chunk_edge(ctx, ref):
    # k_graph_gather takes 64 elements per wavefront: runs of 63, 64 and 65 nodes, edges and pairs. Two copies of N bases: N nodes, N - 1 edges, one alignment of N pairs
    rnd = random.Random(47)
    sets = [[t, t] for t in ("".join(rnd.choice("ACGT") for _ in range(n)) for n in range(62, 68))]
    got, _, _ = assert_equal(ctx, ref, sets, "nw", SCORES[0])
    for what in (lambda r: len(r.node_base), lambda r: len(r.edge_from), lambda r: len(r.sequences[1].alignment), lambda r: len(r.consensus_nodes)):
        assert {63, 64, 65} <= set(what(r) for r in got)
    for mode in ("sw", "ov"):
        assert_equal(ctx, ref, sets, mode, SCORES[4])
    # ... and 128 +- 1 (two chunks), 1 and 2 (a chunk of one element)
    assert_equal(ctx, ref, [["ACGTTGCA" * 16 + x, "ACGTTGCA" * 16 + x] for x in ("", "A", "AC")] + [["A", "A"], ["AC", "AC"]], "nw", SCORES[2])


@pytest.mark.parametrize("model", [0, 1, 2])
def test_longest_sequences_at_the_instance_boundaries(ctx, ref, model):
    # an instance holds NT x CPL columns = the longest sequence + 1: linear 1 024, 4 096, 8 192; affine 1 024, 4 096, 8 192; convex 1 024, 2 048, 4 096
    # (the last instance of each table ends at the model's limit: test_a_sequence_over_the_limit below)
    bounds = {0: (1024, 4096, 8192), 1: (1024, 4096, 8192), 2: (1024, 2048, 4096)}[model]
    scores = {0: SCORES[0], 1: grflib.AFFINE, 2: SCORES[4]}[model]
    rnd = random.Random(48 + model)
    t = "".join(rnd.choice("ACGT") for _ in range(max(bounds)))
    sets = []
    for b in bounds:
        for L in (b - 1, b):
            sets.append([noisy(rnd, t[:L], 0.06)[:L - 40], t[:L]])   # (the longest comes second: it is aligned, not only added)
            assert max(len(q) for q in sets[-1]) == L
    for mode in MODES:
        assert_equal(ctx, ref, sets, mode, scores)


def test_one_base_sequences_empty_members_empty_sets_and_a_single_sequence(ctx, ref):
    sets = [["A"], ["A", "A"], ["A", "C", "G", "T", "A"], ["", "G", ""], [], [""], ["", ""], ["ACGTTGCA"], ["ACGT", "", "ACGT"], ["C"] * 70]
    for mode in MODES:
        for scores in (SCORES[0], SCORES[2], SCORES[4]):
            got, _, _ = assert_equal(ctx, ref, sets, mode, scores)
            assert len(got[0].edge_from) == 0 and got[0].node_base == "A" and got[0].consensus_nodes.tolist() == [0]
            assert got[4].node_base == "" and got[4].sequences == [] and got[5].n_cols == 0 and [len(sq.path) for sq in got[6].sequences] == [0, 0]
            assert got[7].sequences[0].alignment == [] and got[7].sequences[0].path.tolist() == list(range(8)) and len(got[7].edge_from) == 7
    assert ctx.poa_graph([]) == []
    assert ctx.poa_graph([], stats=True)[1]["dp_cells"] == 0


def test_an_alignment_without_a_position_stays_as_the_walk_left_it(ctx, ref):
    sets = [["A", "C"], ["ACGT", "T", "ACGT"], ["AC", "G", "T"]]
    for scores in ((5, -20, -8, -8, -8, -8), (5, -20, -8, -6, -8, -6), (5, -20, -8, -6, -10, -4)):
        got, _, _ = assert_equal(ctx, ref, sets, "ov", scores)
        assert got[0].sequences[1].alignment == [(0, -1)] and got[0].sequences[1].score == -8 and got[0].node_base == "AC"
        assert_equal(ctx, ref, sets, "sw", scores)
        assert_equal(ctx, ref, sets, "nw", scores)


def test_known_answers(ctx):
    got = ctx.poa_graph([["ACGT", "AGT"], ["ACGT", "ACAGT"], ["ACGT", "ACCT"]])
    a = got[0]
    assert a.sequences[1].alignment == [(0, 0), (1, -1), (2, 1), (3, 2)] and a.sequences[1].score == 7 and a.node_base == "ACGT"
    assert a.edge_from.tolist() == [0, 1, 2, 0] and a.edge_to.tolist() == [1, 2, 3, 2] and a.edge_w.tolist() == [2, 2, 4, 2]
    assert [sq.path.tolist() for sq in a.sequences] == [[0, 1, 2, 3], [0, 2, 3]]
    assert got[1].sequences[1].alignment == [(0, 0), (1, 1), (-1, 2), (2, 3), (3, 4)]
    c = got[2]
    assert c.sequences[1].alignment == [(0, 0), (1, 1), (2, 2), (3, 3)] and c.sequences[1].score == 11 and c.node_base == "ACGTC" and c.node_col[4] == c.node_col[2]
    assert c.sequences[1].path.tolist() == [0, 1, 4, 3] and c.node_rank.tolist() == [0, 1, 2, 4, 3] and c.n_cols == 4
    o = ctx.poa_graph([["ACGTACGGTCA", "CGGTCATTGAC"]], "ov")[0]
    assert o.sequences[1].alignment == [(5 + i, i) for i in range(6)] and len(o.node_base) == 16
    assert ctx.poa_graph([["TTACGTAA", "GGACGTCC"]], "sw")[0].sequences[1].alignment == [(2, 2), (3, 3), (4, 4), (5, 5)]


# ---- without the restatement
@pytest.mark.parametrize("si", [0, 2, 4])
@pytest.mark.parametrize("mode", MODES)
def test_invariants_rows_consensus_and_counters_on_the_gpu_output(ctx, mode, si):
    scores, sets = SCORES[si], SETS[:160]
    kw = grflib.kw_of(scores, mode)
    got, st = ctx.poa_graph(sets, stats=True, **kw)
    bad = [(k, why) for k in range(len(sets)) for why in grflib.checks(got[k], sets[k]) + grflib.rescore(got[k], sets[k], scores, mode)]
    assert bad[:5] == []
    mkw = dict(kw) if grflib.model_of(scores) == 2 else {k: v for k, v in kw.items() if k not in ("gap_open2", "gap_extend2")}
    rows, cns, mst = ctx.poa_msa(sets, stats=True, **mkw)
    assert [k for k in range(len(sets)) if grflib.rows_of(got[k], sets[k]) != rows[k]] == []
    assert [r.consensus for r in got] == cns
    with ctx.options(poa_general=1):
        only, st0 = ctx.poa_sequences_convex(sets, mode, *scores, stats=True) if grflib.model_of(scores) == 2 else ctx.poa_sequences_affine(sets, mode, *scores[:4], stats=True)
    assert only == cns and {k: st[k] for k in ("dp_cells", "seq_bases", "n_aligned")} == st0
    W = wgtlib.quality_weights(sets, 70 + si)
    wgot = ctx.poa_graph(sets, weights=W, **kw)
    assert [(k, why) for k in range(len(sets)) for why in grflib.checks(wgot[k], sets[k], W[k])][:5] == []
    assert [r.consensus for r in wgot] == ctx.poa_weighted(sets, W, **mkw)
    # weights change the edges' weights and the consensus, nothing else
    assert all(a.node_base == b.node_base and all(np.array_equal(x.path, y.path) and x.alignment == y.alignment and x.score == y.score for x, y in zip(a.sequences, b.sequences)) for a, b in zip(got, wgot))


def test_the_kernels_of_a_simpler_model_under_the_options_give_the_same_graph(ctx):
    sets = SETS[:80]
    for mode in MODES:
        want = ctx.poa_graph(sets, mode)
        with ctx.options(poa_affine=1):
            assert all(grflib.same(a, b) for a, b in zip(ctx.poa_graph(sets, mode), want))
        want = ctx.poa_graph(sets, mode, gap_extend=-6)
        with ctx.options(poa_convex=1):
            assert all(grflib.same(a, b) for a, b in zip(ctx.poa_graph(sets, mode, gap_extend=-6, gap_open2=-9, gap_extend2=-7), want))
        assert all(grflib.same(a, b) for a, b in zip(ctx.poa_graph(sets, mode, gap_extend=-6, gap_open2=-9, gap_extend2=-7), want))   # (the second piece never wins: the affine route)


@pytest.mark.parametrize("model", [0, 1, 2])
def test_a_sequence_over_the_limit_is_an_error_that_names_its_set(ctx, ref, model):
    from haslr_amd import hip
    scores = {0: SCORES[0], 1: grflib.AFFINE, 2: SCORES[4]}[model]
    L = MAX_LEN[model]
    rnd = random.Random(49)
    t = "".join(rnd.choice("ACGT") for _ in range(L + 1))
    got = ctx.poa_graph([["ACGT"], [t[:L]]], **grflib.kw_of(scores, "ov"))   # (at the limit: the last instance of the table)
    assert got[1].node_base == t[:L] and got[1].consensus == t[:L] and got[1].edge_w.tolist() == [2] * (L - 1)
    with pytest.raises(hip.HipError, match=rf"hx_poa_graph: set 2 holds a sequence of {L + 1} bases, longer than {L}"):
        ctx.poa_graph([["ACGT"], ["ACGT", "ACGA"], ["ACGT", t]], **grflib.kw_of(scores, "ov"))


def test_bad_parameters_and_a_zero_weight_are_errors_under_the_entrys_name(ctx):
    from haslr_amd import hip
    with pytest.raises(hip.HipError, match="hx_poa_graph: the second gap open score -7 is above the first gap open score -8"):
        ctx.poa_graph([["ACGT"]], "sw", 5, -4, -8, -6, -7, -4)
    with pytest.raises(hip.HipError, match="hx_poa_graph: the second gap extend score must not be positive, not 1"):
        ctx.poa_graph([["ACGT"]], gap_open=-8, gap_extend=-6, gap_open2=-10, gap_extend2=1)
    with pytest.raises(hip.HipError, match="hx_poa_graph: the gap open score must be negative, not 0"):
        ctx.poa_graph([["ACGT"]], gap_open=0, gap_extend=0)
    with pytest.raises(hip.HipError, match="hx_poa_graph: the gap extend score -9 is below the gap open score -8"):
        ctx.poa_graph([["ACGT"]], gap_open=-8, gap_extend=-9)
    with pytest.raises(hip.HipError, match="hx_poa_graph: set 1, sequence 1, position 1: a weight of 0 is not accepted"):
        ctx.poa_graph([["ACGT"], ["ACGT", "ACG"]], weights=[[[1, 1, 1, 1]], [[2, 2, 2, 2], [3, 0, 3]]])
    with pytest.raises(ValueError):
        ctx.poa_graph([["ACGT"]], "xx")


@pytest.fixture(scope="module")
def graph_caller(built, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("spoa_graph_gpu") / "spoa_graph_caller")
    lib = os.path.join(ROOT, "haslr_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "spoa_graph_caller.cpp"), "-o", exe,
                           "-L", lib, "-lhaslr_hip", "-pthread", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def mixed_edges(seed, n):
    """edges of every type under four-, five- and seven-score engines; one seven-score kind has a second piece that never wins"""
    rnd = random.Random(seed)
    kinds = [None, (5, -4, -8, -2), (5, -4, -8, -6, -10, -4), (5, -4, -8, -6, -9, -7)]
    edges = []
    for k in range(n):
        t = "".join(rnd.choice("ACGT") for _ in range(rnd.randrange(20, 300)))
        edges.append((MODES[k % 3], kinds[(k // 3) % len(kinds)], [noisy(rnd, t, 0.08) or "A" for _ in range(rnd.randrange(1, 6))]))
    return edges


def six(sc):
    return (5, -4, -8, -8, -8, -8) if sc is None else sc + sc[2:4] if len(sc) == 4 else sc


@pytest.mark.parametrize("args", [["--threads", "16"], ["--batch"]])
def test_header_callers_write_the_graph_the_python_call_returns(ctx, graph_caller, tmp_path, args):
    from haslr_amd import hip
    edges = mixed_edges(51, 48)
    text = "\n\n".join(ty + ("" if sc is None else " " + " ".join(str(v) for v in sc)) + "\n" + "\n".join(st) for ty, sc, st in edges) + "\n"
    r = subprocess.run([graph_caller, "--out", str(tmp_path)] + args, input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    blocks = r.stdout.split("=\n")[:-1]
    assert len(blocks) == len(edges)
    for k, (ty, sc, st) in enumerate(edges):
        rec = ctx.poa_graph([st], **grflib.kw_of(six(sc), ty))[0]
        gfa, dot = (tmp_path / f"{k}.gfa").read_text(), (tmp_path / f"{k}.dot").read_text()
        assert gfa == hip.graph_to_gfa(rec) and dot == hip.graph_to_dot(rec), k   # (the C++ and the Python writers: the same bytes)
        assert grflib.parse_gfa(gfa) == grflib.gfa_of(rec) and grflib.parse_dot(dot) == grflib.dot_of(rec), k
        alns = [" ".join(f"{a}:{b}" for a, b in sq.alignment) or "." for sq in rec.sequences]
        if args[0] == "--threads":   # (the caller asks alignment(k) for the first and the last added sequence)
            alns = [a for q, a in enumerate(alns) if q == 0 or q + 1 == len(alns)]
        assert blocks[k].split("\n")[:-1] == alns, k
