"""The convex-gap entries (hx_poa_sequences_convex, hx_poa_msa_convex, hx_poa_weighted_convex) on the MI355X: the convex instances of the
general path (kernels/poa_modes.hip) equal the CPU restatement (tests/poa_convex_ref.cpp) bit for bit - on the CPU tests' sets in three
modes and four score sets, on sequences at the limit of 8 191 bases, on a call of 2 000 sets that runs every convex instance and the
persistent workgroups, with slots capped so small that sets are rerun in larger ones, and on the structured corpus of tests/poasets.py; a
second piece that never wins through the new entries is the affine entries, and under option poa_convex the convex kernel gives the same
results; MSA rows, weighted consensus, coverage and profile equal the restatement; header callers mix four-, five- and seven-score engines
of every type in one process."""
import os
import random
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

import cvxlib
import parlib
import pmrlib
import poasets
import wgtlib
from test_poa_modes_ref import SETS, noisy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
MODES = ["sw", "nw", "ov"]
# (match, mismatch, g, e, q, c): spoa's defaults, a dear and almost free second piece, c = 0 with g == e, and small scores
SCORES = [(5, -4, -8, -6, -10, -4), (5, -4, -8, -6, -24, -1), (2, -7, -2, -2, -9, 0), (1, -1, -3, -2, -5, -1)]
MAX_LEN = 8191   # the longest sequence a convex call takes (include/haslr_hip.h)


@pytest.fixture(scope="module")
def ref(built, tmp_path_factory):
    return cvxlib.ConvexRef(str(tmp_path_factory.mktemp("cvx_gpu")))


@pytest.fixture(scope="module")
def aff(built, tmp_path_factory):
    return parlib.AffineRef(str(tmp_path_factory.mktemp("cvx_gpu_par")))


@pytest.fixture(scope="module")
def ctx(built):
    from haslr_amd import hip
    c = hip.HipContext(0)   # raises without a device: these tests never run on a fallback
    yield c
    c.close()


def pmap(fn, items, threads=16):
    with ThreadPoolExecutor(threads) as ex:   # (the restatements release the GIL: ctypes)
        return list(ex.map(fn, items))


def ref_all(ref, sets, mode, scores=cvxlib.DEFAULT, threads=16):
    res = pmap(lambda st: ref.consensus_cells(st, mode, scores), sets, threads)
    return [r[0] for r in res], sum(r[1] for r in res)


def kw_of(scores, mode):
    return dict(type=mode, match=scores[0], mismatch=scores[1], gap_open=scores[2], gap_extend=scores[3], gap_open2=scores[4], gap_extend2=scores[5])


def differing(got, want):
    assert len(got) == len(want)
    return [k for k in range(len(want)) if got[k] != want[k]]


def many_sets(seed, n):
    """n sets whose longest sequences fall in every convex instance of the general path (up to 1023, 2047, 4095 and 8191 bases + 1 columns)"""
    rnd = random.Random(seed)
    out = []
    for k in range(n):
        L = rnd.choice([1, 3, 30, 120, 400, 900]) if k % 50 else (1500, 3000, 5000, 7500)[(k // 50) % 4]
        t = "".join(rnd.choice("ACGT") for _ in range(L))
        out.append([noisy(rnd, t, 0.1) for _ in range(rnd.randrange(1, 5 if L < 1000 else 3))])
    return out


def test_many_sets_reach_every_convex_instance():
    longest = [max(len(q) for q in st) for st in many_sets(22, 2000)]
    for lo, hi in ((0, 1023), (1024, 2047), (2048, 4095), (4096, MAX_LEN)):
        assert any(lo <= v <= hi for v in longest), (lo, hi)


@pytest.mark.parametrize("mode", MODES)
def test_convex_equals_the_restatement_on_the_cpu_sets(ctx, ref, mode):
    for scores in SCORES:
        sets = SETS if scores == SCORES[0] else SETS[:120]
        want, cells = ref_all(ref, sets, mode, scores)
        got, st = ctx.poa_sequences_convex(sets, mode, *scores, stats=True)
        assert differing(got, want) == [], (mode, scores)
        assert st["dp_cells"] == cells
        assert st["seq_bases"] == sum(len(q) for s in sets for q in s) and st["n_aligned"] == sum(1 for s in sets for q in s if q)


@pytest.mark.parametrize("mode", MODES)
def test_sequences_at_the_limit(ctx, ref, mode):
    rnd = random.Random(21)
    t = "".join(rnd.choice("ACGT") for _ in range(MAX_LEN))
    sets = [[t], [t, noisy(rnd, t, 0.08)[:MAX_LEN]], ["ACGTACGT", t[2500:7500], t]]
    assert max(len(q) for st in sets for q in st) == MAX_LEN
    assert ctx.poa_sequences_convex(sets, mode) == ref_all(ref, sets, mode, threads=3)[0]


def test_a_sequence_a_base_over_the_limit_is_an_error_that_names_its_set(ctx):
    from haslr_amd import hip
    rnd = random.Random(26)
    t = "".join(rnd.choice("ACGT") for _ in range(MAX_LEN + 1))
    assert ctx.poa_sequences_convex([["ACGT"], [t[:MAX_LEN]]], "ov") == ["ACGT", t[:MAX_LEN]]
    with pytest.raises(hip.HipError, match=rf"hx_poa_sequences_convex: set 2 holds a sequence of {MAX_LEN + 1} bases, longer than {MAX_LEN}"):
        ctx.poa_sequences_convex([["ACGT"], ["ACGT", "ACGA"], ["ACGT", t]], "ov")
    with pytest.raises(hip.HipError, match=rf"hx_poa_msa_convex: set 1 holds a sequence of {MAX_LEN + 1} bases, longer than {MAX_LEN}"):
        ctx.poa_msa([["ACGT"], ["ACGT", t]], **kw_of(SCORES[0], "nw"))
    with pytest.raises(hip.HipError, match=rf"hx_poa_weighted_convex: set 0 holds a sequence of {MAX_LEN + 1} bases, longer than {MAX_LEN}"):
        ctx.poa_weighted([[t]], coverage=True, **kw_of(SCORES[0], "sw"))


@pytest.mark.parametrize("mode", MODES)
def test_two_thousand_sets_in_one_call(ctx, ref, mode):
    sets = many_sets(22, 2000)
    want, cells = ref_all(ref, sets, mode)
    got, st = ctx.poa_sequences_convex(sets, mode, stats=True)
    assert differing(got, want) == []
    assert st["dp_cells"] == cells


@pytest.mark.parametrize("mode", MODES)
def test_overflowing_slots_are_rerun_in_larger_ones(ctx, ref, mode):
    sets = many_sets(23, 300)
    want = ref_all(ref, sets, mode)[0]
    with ctx.options(poa_modes_slot_kb=1):   # (first-round slots hold little more than the largest graph pools of their instance: sets stop and are rerun)
        got = ctx.poa_sequences_convex(sets, mode)
    assert differing(got, want) == []


def test_a_second_piece_that_never_wins_is_the_affine_entries(ctx):
    sets = SETS[:200]
    W = wgtlib.quality_weights(sets, 31)
    for mode in MODES:
        for q, c in ((-8, -6), (-9, -7), (-30, -6)):
            assert ctx.poa_sequences_convex(sets, mode, 5, -4, -8, -6, q, c, stats=True) == ctx.poa_sequences_affine(sets, mode, 5, -4, -8, -6, stats=True)
        # ... which sends equal gap scores on to the linear paths
        assert ctx.poa_sequences_convex(sets, mode, 5, -4, -8, -8, -8, -8, stats=True) == ctx.poa_sequences_mode(sets, mode, stats=True)
        kw = dict(type=mode, gap_open=-8, gap_extend=-6)
        assert ctx.poa_msa(sets, include_consensus=True, gap_open2=-9, gap_extend2=-7, **kw) == ctx.poa_msa(sets, include_consensus=True, **kw)
        assert ctx.poa_weighted(sets, W, coverage=True, profile=True, gap_open2=-9, gap_extend2=-7, **kw) == ctx.poa_weighted(sets, W, coverage=True, profile=True, **kw)
    # the tuned kNW path prunes, the general path fills the whole matrix: the cell counts tell which one ran
    tuned = ctx.poa_sequences_mode(SETS[:60], "nw", stats=True)[1]["dp_cells"]
    assert ctx.poa_sequences_convex(SETS[:60], "nw", 5, -4, -8, -8, -8, -8, stats=True)[1]["dp_cells"] == tuned


def test_a_second_piece_that_never_wins_through_the_convex_kernel_gives_the_affine_results(ctx, aff, built, tmp_path):
    lin = pmrlib.ModesRef(str(tmp_path))
    sets = SETS
    W = wgtlib.quality_weights(sets, 31)
    with ctx.options(poa_convex=1):
        for mode in MODES:
            res = pmap(lambda st: aff.consensus_cells(st, mode, 5, -4, -8, -6), sets)
            for q, c in ((-8, -6), (-9, -7)):
                got, st = ctx.poa_sequences_convex(sets, mode, 5, -4, -8, -6, q, c, stats=True)
                assert differing(got, [r[0] for r in res]) == [], (mode, q, c)
                assert st["dp_cells"] == sum(r[1] for r in res)
            res = pmap(lambda st: lin.consensus_cells(st, mode, 3, -5, -4), sets[:120])
            got, st = ctx.poa_sequences_convex(sets[:120], mode, 3, -5, -4, -4, -4, -4, stats=True)
            assert differing(got, [r[0] for r in res]) == [], (mode, "linear")
            assert st["dp_cells"] == sum(r[1] for r in res)   # (the option is what sent kNW there: the whole matrix)
    for mode in MODES:
        kw = dict(type=mode, gap_open=-8, gap_extend=-6)
        want_msa, want_w = ctx.poa_msa(sets, include_consensus=True, **kw), ctx.poa_weighted(sets, W, coverage=True, profile=True, **kw)
        with ctx.options(poa_convex=1):
            assert ctx.poa_msa(sets, include_consensus=True, gap_open2=-9, gap_extend2=-7, **kw) == want_msa
            assert ctx.poa_weighted(sets, W, coverage=True, profile=True, gap_open2=-9, gap_extend2=-7, **kw) == want_w


@pytest.mark.parametrize("mode", MODES)
def test_msa_rows_equal_the_restatement(ctx, ref, mode):
    sets = SETS[:200] + many_sets(24, 100)
    for scores in SCORES[:2]:
        want = pmap(lambda st: ref.msa(st, mode, scores, True), sets)
        rows, cns, st = ctx.poa_msa(sets, include_consensus=True, stats=True, **kw_of(scores, mode))
        assert differing(rows, [r.rows for r in want]) == [], (mode, scores)
        assert differing(cns, [r.consensus for r in want]) == [], (mode, scores)
        assert st["seq_bases"] == sum(len(q) for s in sets for q in s)
        assert differing(ctx.poa_msa(sets, **kw_of(scores, mode)), [r.rows[:-1] for r in want]) == [], (mode, scores, "without the consensus row")


@pytest.mark.parametrize("mode", MODES)
def test_weighted_consensus_coverage_and_profile_equal_the_restatement(ctx, ref, mode):
    sets = SETS[:200] + many_sets(25, 100)
    for scores, W in ((SCORES[0], wgtlib.quality_weights(sets, 71)), (SCORES[1], wgtlib.uniform_weights(sets, 72))):
        want = pmap(lambda k: ref.weighted(sets[k], W[k], mode, scores), range(len(sets)))
        cns, cov, prof = ctx.poa_weighted(sets, W, coverage=True, profile=True, **kw_of(scores, mode))
        assert differing(list(zip(cns, cov, prof)), [(r.consensus, r.coverage, r.profile) for r in want]) == [], (mode, scores)
        assert ctx.poa_weighted(sets, W, coverage=True, **kw_of(scores, mode)) == (cns, cov)
        assert ctx.poa_weighted(sets, W, **kw_of(scores, mode)) == cns
    # without weights: the unit-weight consensus of the plain entry, and the restatement's coverage
    want = pmap(lambda st: ref.weighted(st, None, mode, SCORES[0]), sets)
    cns, cov = ctx.poa_weighted(sets, coverage=True, **kw_of(SCORES[0], mode))
    assert cns == ctx.poa_sequences_convex(sets, mode, *SCORES[0])
    assert differing(list(zip(cns, cov)), [(r.consensus, r.coverage) for r in want]) == []
    with ctx.options(poa_weighted=1):   # (no weights, through the weighted instances on weights of 1)
        assert ctx.poa_weighted(sets, coverage=True, **kw_of(SCORES[0], mode)) == (cns, cov)


def test_a_zero_weight_is_refused_under_the_new_name(ctx):
    from haslr_amd import hip
    import ctypes as C

    import numpy as np
    from haslr_amd import ctypes_defs as T
    off, soff = np.array([0, 1, 3], dtype=np.uint64), np.array([0, 4, 8, 11], dtype=np.uint64)
    o, cp = T.WcnsOut(), T.PoaConvexParams(*SCORES[0], 1)
    args = (ctx._h, 2, off.ctypes.data_as(T.u64p), soff.ctypes.data_as(T.u64p), b"ACGTACGTACG")
    assert hip.lib().hx_poa_weighted_convex(*args, bytes([1, 1, 1, 1, 2, 2, 2, 2, 3, 0, 3]), C.byref(cp), 1, 0, C.byref(o)) != 0
    assert "hx_poa_weighted_convex: set 1, sequence 1, position 1: a weight of 0 is not accepted" in hip.lib().hx_last_error().decode()


def failing(corpus, got, want):
    """the (family, index) pairs of the sets whose results differ"""
    assert len(got) == len(want) == len(corpus)
    return [(f, k) for (f, k, _), a, b in zip(corpus, got, want) if a != b]


@pytest.mark.parametrize("mode", MODES)
def test_the_structured_corpus(ctx, ref, mode):
    corpus = poasets.CORPUS   # (tie-heavy, high fan-in and many-member sets)
    sets = [st for _, _, st in corpus]
    res = pmap(lambda st: ref.consensus_cells(st, mode, SCORES[0]), sets)
    got, st = ctx.poa_sequences_convex(sets, mode, *SCORES[0], stats=True)
    assert failing(corpus, got, [r[0] for r in res]) == [], mode
    assert st["dp_cells"] == sum(r[1] for r in res), mode


@pytest.mark.parametrize("mode", MODES)
def test_the_structured_corpus_rerun_in_larger_slots_and_its_rows_and_coverage(ctx, ref, mode):
    scores = SCORES[0]
    third = poasets.sub_sample(3)   # (at least one set of every family)
    sets = [st for _, _, st in third]
    W = wgtlib.uniform_weights(sets, 71)
    want_m = pmap(lambda st: ref.msa(st, mode, scores, True), sets)
    want_w = pmap(lambda k: ref.weighted(sets[k], W[k], mode, scores), range(len(sets)))
    with ctx.options(poa_modes_slot_kb=1):   # (first-round slots of 1 KB: sets stop and are rerun in larger slots)
        assert failing(third, ctx.poa_sequences_convex(sets, mode, *scores), [r.consensus for r in want_m]) == [], mode
    assert failing(third, ctx.poa_msa(sets, include_consensus=True, **kw_of(scores, mode)), [r.rows for r in want_m]) == [], mode
    cns, cov, prof = ctx.poa_weighted(sets, W, coverage=True, profile=True, **kw_of(scores, mode))
    assert failing(third, list(zip(cns, cov, prof)), [(r.consensus, r.coverage, r.profile) for r in want_w]) == [], mode


def test_bad_parameters_are_errors(ctx):
    from haslr_amd import hip
    with pytest.raises(hip.HipError, match="hx_poa_sequences_convex: the second gap open score -7 is above the first gap open score -8"):
        ctx.poa_sequences_convex([["ACGT"]], "sw", 5, -4, -8, -6, -7, -4)
    with pytest.raises(hip.HipError, match="hx_poa_msa_convex: the second gap extend score must not be positive, not 1"):
        ctx.poa_msa([["ACGT"]], gap_open=-8, gap_extend=-6, gap_open2=-10, gap_extend2=1)
    with pytest.raises(hip.HipError, match="hx_poa_weighted_convex: the gap open score must be negative, not 0"):
        ctx.poa_weighted([["ACGT"]], gap_open=0, gap_extend=0, gap_open2=-10, gap_extend2=-4)


@pytest.fixture(scope="module")
def convex_caller(built, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("spoa_convex_gpu") / "spoa_convex_caller")
    lib = os.path.join(ROOT, "haslr_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "spoa_convex_caller.cpp"), "-o", exe,
                           "-L", lib, "-lhaslr_hip", "-pthread", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def mixed_edges(seed, n):
    """edges of every type under four-score (None), five-score and seven-score engines; one seven-score kind has a second piece that never wins"""
    rnd = random.Random(seed)
    kinds = [None, (5, -4, -8, -2), (5, -4, -8, -6, -10, -4), (5, -4, -8, -6, -24, -1), (2, -7, -2, -2, -9, 0), (5, -4, -8, -6, -9, -7)]
    edges = []
    for k in range(n):
        t = "".join(rnd.choice("ACGT") for _ in range(rnd.randrange(40, 600)))
        edges.append((("sw", "nw", "ov")[k % 3], kinds[(k // 3) % len(kinds)], [noisy(rnd, t, 0.08) for _ in range(rnd.randrange(1, 7))]))
    return edges


def edge_text(edges):
    return "\n\n".join(ty + ("" if sc is None else " " + " ".join(str(v) for v in sc)) + "\n" + "\n".join(st) for ty, sc, st in edges) + "\n"


def six(sc):
    return (5, -4, -8, -8, -8, -8) if sc is None else sc + sc[2:4] if len(sc) == 4 else sc


@pytest.mark.parametrize("args", [["--threads", "16"], ["--batch"]])
def test_header_callers_with_four_five_and_seven_score_engines_of_mixed_types(convex_caller, ref, args):
    edges = mixed_edges(27, 108)
    r = subprocess.run([convex_caller] + args, input=edge_text(edges), capture_output=True, text=True, env=dict(os.environ, HASLR_SPOA_BATCH_US="3000"))
    assert r.returncode == 0, r.stderr
    want = pmap(lambda e: ref.consensus(e[2], e[0], six(e[1])), edges)   # (one piece, or a second one that never wins: the restatement is the affine one, tests/test_poa_convex_ref.py)
    assert r.stdout.split("\n")[:-1] == want


def test_graph_outputs_under_seven_score_engines_from_several_threads(convex_caller, ref):
    edges = mixed_edges(28, 54)
    r = subprocess.run([convex_caller, "--threads", "8", "--outputs"], input=edge_text(edges), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def want(e):
        ty, sc, st = e
        w, m = ref.weighted(st, None, ty, six(sc)), ref.msa(st, ty, six(sc), True)
        return "|".join([w.consensus, ",".join(str(v) for v in w.coverage)] + m.rows)

    assert r.stdout.split("\n")[:-1] == pmap(want, edges)
