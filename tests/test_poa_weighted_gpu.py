"""hx_poa_weighted on the MI355X: consensus, coverage and profile equal the CPU restatement (tests/poa_weighted_ref.cpp) value for value,
for every set - on the CPU tests' sets with both seeded weightings in three modes, linear and affine, on long sequences, on a call of
2 000 sets that runs every instance and the persistent workgroups, with slots capped so small that sets are rerun in larger ones, and on
a set whose bundle scores are large; without weights the consensus and the counters are those of the consensus-only entries; header
callers mix weights, qualities, coverage calls and plain unit-weight graphs in one process; bad weights are errors that name their place."""
import ctypes as C
import os
import random
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

import wgtlib
from test_poa_affine_gpu import many_sets as many_sets_affine
from test_poa_modes_gpu import many_sets
from test_poa_modes_ref import SETS, noisy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
MODES = ["sw", "nw", "ov"]
LINEAR = [(5, -4, -8, -8), (3, -5, -4, -4)]
AFFINE = [(5, -4, -8, -2), (3, -5, -4, 0)]
WEIGHTINGS = {"uniform": wgtlib.uniform_weights(SETS, 51), "quality": wgtlib.quality_weights(SETS, 52)}


@pytest.fixture(scope="module")
def ref(built, tmp_path_factory):
    return wgtlib.WeightedRef(str(tmp_path_factory.mktemp("pwr_gpu")))


@pytest.fixture(scope="module")
def ctx(built):
    from haslr_amd import hip
    c = hip.HipContext(0)
    yield c
    c.close()


def ref_all(ref, sets, weights, mode, m=5, x=-4, g=-8, e=None, threads=16):
    with ThreadPoolExecutor(threads) as ex:   # (the restatement releases the GIL: ctypes)
        return list(ex.map(lambda k: ref.weighted(sets[k], None if weights is None else weights[k], mode, m, x, g, e), range(len(sets))))


def assert_equal(got, want, tag):
    cns, cov, prof = got[:3]
    assert len(cns) == len(cov) == len(prof) == len(want)
    bad = [k for k in range(len(want)) if (cns[k], cov[k], prof[k]) != (want[k].consensus, want[k].coverage, want[k].profile)]
    assert bad == [], (tag, bad[:10])
    assert all(w.flags == 0 for w in want)


@pytest.mark.parametrize("weighting", sorted(WEIGHTINGS))
@pytest.mark.parametrize("mode", MODES)
def test_weighted_equals_the_restatement_on_the_cpu_sets(ctx, ref, mode, weighting):
    for scores in LINEAR + AFFINE:
        n = len(SETS) if scores in (LINEAR[0], AFFINE[0]) else 120
        sets, W = SETS[:n], WEIGHTINGS[weighting][:n]
        want = ref_all(ref, sets, W, mode, *scores)
        got = ctx.poa_weighted(sets, W, type=mode, match=scores[0], mismatch=scores[1], gap_open=scores[2], gap_extend=scores[3], coverage=True, profile=True)
        assert_equal(got, want, (mode, scores, weighting))
        # coverage alone (one counter per column instead of four) and the consensus alone are the same values
        cns, cov = ctx.poa_weighted(sets, W, type=mode, match=scores[0], mismatch=scores[1], gap_open=scores[2], gap_extend=scores[3], coverage=True)
        assert (cns, cov) == (got[0], got[1])
        assert ctx.poa_weighted(sets, W, type=mode, match=scores[0], mismatch=scores[1], gap_open=scores[2], gap_extend=scores[3]) == got[0]


def test_qualities_are_weights_of_character_minus_33(ctx, ref):
    sets, W = SETS[:150], WEIGHTINGS["quality"][:150]
    Q = [wgtlib.quality_strings(w) for w in W]
    got = ctx.poa_weighted(sets, qualities=Q, coverage=True, profile=True)
    assert got == ctx.poa_weighted(sets, W, coverage=True, profile=True)
    assert_equal(got, ref_all(ref, sets, W, "nw"), "qualities")


@pytest.mark.parametrize("mode", MODES)
def test_without_weights_it_is_the_consensus_entries(ctx, ref, mode):
    ones = [[[1] * len(q) for q in st] for st in SETS]
    for scores in (LINEAR[0], AFFINE[0]):
        kw = dict(type=mode, match=scores[0], mismatch=scores[1], gap_open=scores[2], gap_extend=scores[3])
        with ctx.options(poa_general=1):
            only, st0 = ctx.poa_sequences_affine(SETS, mode, *scores, stats=True)
        want = ref_all(ref, SETS, None, mode, *scores)
        calls = [ctx.poa_weighted(SETS, None, coverage=True, profile=True, stats=True, **kw), ctx.poa_weighted(SETS, ones, coverage=True, profile=True, stats=True, **kw)]
        with ctx.options(poa_weighted=1):   # (no weights, through the weighted instances on weights of 1)
            calls.append(ctx.poa_weighted(SETS, None, coverage=True, profile=True, stats=True, **kw))
        for got in calls:
            assert got[0] == only
            assert {k: got[3][k] for k in ("dp_cells", "seq_bases", "n_aligned")} == st0
            assert_equal(got, want, (mode, scores))
    if mode == "nw":   # the tuned path
        assert ctx.poa_weighted(SETS) == ctx.poa_sequences(SETS)


@pytest.mark.parametrize("k", [2, 255])
def test_one_weight_on_every_base_changes_nothing(ctx, k):
    W = [[[k] * len(q) for q in st] for st in SETS]
    for mode in MODES:
        assert ctx.poa_weighted(SETS, W, type=mode, coverage=True, profile=True) == ctx.poa_weighted(SETS, type=mode, coverage=True, profile=True)


def test_known_answers(ctx):
    st = ["AAGAA", "AAGAA", "AATAA"]
    sets = [st, st, ["ACGT", "A", "ACGT"], ["A"], ["ACGT", "", "ACT"], [], [""]]
    W = [[[1] * 5] * 3, [[1] * 5, [1] * 5, [10] * 5], [[1] * 4, [7], [1] * 4], [[9]], [[3] * 4, [], [2] * 3], [], [[]]]
    cns, cov, prof = ctx.poa_weighted(sets, W, coverage=True, profile=True)
    assert cns == ["AAGAA", "AATAA", "ACGT", "A", "ACGT", "", ""]
    assert cov == [[3] * 5, [3] * 5, [2] * 4, [0], [2, 2, 1, 2], [], []]
    assert prof[0][2] == prof[1][2] == [0, 0, 2, 1] and prof[3] == [[0, 0, 0, 0]] and prof[5] == prof[6] == []
    # the end of the consensus moved through branch completion (tests/test_poa_weighted_ref.py has the derivation)
    M = "ACCAGA"
    st = ["T" * 40 + M, "G" + M + "A", "G" + M + "C", "G" + M + "A"]
    assert ctx.poa_weighted([st, st, st], [[[1] * 46, [1] * 8, [v] * 8, [1] * 8] for v in (1, 3, 4)], type="sw", coverage=True) == \
        (["T" * 40 + M + "A", "T" * 40 + M + "C", "G" + M + "C"], [[1] * 40 + [4] * 6 + [2], [1] * 40 + [4] * 6 + [1], [3] + [4] * 6 + [1]])
    # the two empty-alignment paths
    assert ctx.poa_weighted([["A", "C"]], [[[9], [200]]], type="sw", coverage=True) == (["A"], [[0]])
    assert ctx.poa_weighted([["A", "C"]], [[[9], [200]]], type="ov", mismatch=-20, gap_open=-1, coverage=True) == (["A"], [[0]])
    assert ctx.poa_weighted([], coverage=True, profile=True) == ([], [], [])


@pytest.mark.parametrize("mode", MODES)
def test_long_sequences_near_both_length_limits(ctx, ref, mode):
    rnd = random.Random(61)
    t = "".join(rnd.choice("ACGT") for _ in range(32767))
    for limit, L, e in ((32767, 20000, None), (16383, 16000, -2)):   # linear, affine
        u = t[:L]
        sets = [[t[:limit]], [u, noisy(rnd, u, 0.08)], ["ACGTACGT", u[5000:15000], u], [t[:limit], "ACGT"]]
        W = wgtlib.uniform_weights(sets, 62)
        want = ref_all(ref, sets, W, mode, e=e, threads=4)
        assert_equal(ctx.poa_weighted(sets, W, type=mode, gap_extend=e, coverage=True, profile=True), want, (mode, limit))


@pytest.mark.parametrize("mode", MODES)
def test_two_thousand_sets_in_one_call(ctx, ref, mode):
    sets = many_sets(63, 2000)
    W = wgtlib.quality_weights(sets, 64)
    assert_equal(ctx.poa_weighted(sets, W, type=mode, coverage=True, profile=True), ref_all(ref, sets, W, mode), mode)
    sets = many_sets_affine(65, 2000)
    W = wgtlib.uniform_weights(sets, 66)
    assert_equal(ctx.poa_weighted(sets, W, type=mode, gap_extend=-6, coverage=True, profile=True), ref_all(ref, sets, W, mode, e=-6), (mode, "affine"))


@pytest.mark.parametrize("mode", MODES)
def test_sets_rerun_in_larger_slots_give_the_same_coverage(ctx, ref, mode):
    sets = many_sets(67, 300)
    W = wgtlib.uniform_weights(sets, 68)
    for e in (None, -6):
        want = ref_all(ref, sets, W, mode, e=e)
        with ctx.options(poa_modes_slot_kb=1):   # (first-round slots hold little more than the graph pools: sets stop and are rerun)
            got = ctx.poa_weighted(sets, W, type=mode, gap_extend=e, coverage=True, profile=True)
        assert_equal(got, want, (mode, e))


def test_large_bundle_scores_stay_exact(ctx, ref):
    # 30 copies of 2 500 bases at weight 255: an edge all copies share weighs 30 x 510, a path over it some 3.8e7; the restatement
    # scores in int64, so equality shows the device's int32 scores hold where they are exercised (the bound itself: include/haslr_hip.h)
    rnd = random.Random(69)
    t = "".join(rnd.choice("ACGT") for _ in range(2500))
    st = [noisy(rnd, t, 0.06) for _ in range(30)]
    W = [[[255] * len(q) for q in st]]
    W[0][7] = [rnd.choice((254, 255)) for _ in st[7]]
    for mode, e in (("nw", None), ("ov", -2)):
        assert_equal(ctx.poa_weighted([st], W, type=mode, gap_extend=e, coverage=True, profile=True), ref_all(ref, [st], W, mode, e=e, threads=1), (mode, e))


def test_bad_parameters_are_errors(ctx):
    import numpy as np
    from haslr_amd import ctypes_defs as T
    from haslr_amd import hip
    with pytest.raises(hip.HipError, match="hx_poa_weighted: the gap open score must be negative"):
        ctx.poa_weighted([["ACGT"]], gap_open=0, gap_extend=0)
    with pytest.raises(hip.HipError, match="hx_poa_weighted: the gap extend score -8 is below the gap open score -2"):
        ctx.poa_weighted([["ACGT"]], gap_open=-2, gap_extend=-8)
    with pytest.raises(ValueError, match="set 0, sequence 0, position 1: a weight of 0"):
        ctx.poa_weighted([["ACGT"]], [[[1, 0, 1, 1]]])
    # the C ABI refuses a weight of 0 itself, and names set, sequence and position
    o, wp = T.WcnsOut(), T.PoaWeightedParams(5, -4, -8, -8, 1, 1, 1)
    off = np.array([0, 1, 3], dtype=np.uint64)
    soff = np.array([0, 4, 8, 11], dtype=np.uint64)
    args = (ctx._h, 2, off.ctypes.data_as(T.u64p), soff.ctypes.data_as(T.u64p), b"ACGTACGTACG")
    assert hip.lib().hx_poa_weighted(*args, bytes([1, 1, 1, 1, 2, 2, 2, 2, 3, 0, 3]), C.byref(wp), C.byref(o)) != 0
    assert "hx_poa_weighted: set 1, sequence 1, position 1: a weight of 0 is not accepted" in hip.lib().hx_last_error().decode()
    assert not o.cns and not o.coverage
    wp.type = 3
    assert hip.lib().hx_poa_weighted(*args, None, C.byref(wp), C.byref(o)) != 0
    assert "hx_poa_weighted: unknown alignment type 3" in hip.lib().hx_last_error().decode()
    rnd = random.Random(70)
    t = "".join(rnd.choice("ACGT") for _ in range(32768))
    for limit, e in ((32767, None), (16383, -2)):
        with pytest.raises(hip.HipError, match=rf"hx_poa_weighted: set 1 holds a sequence of {limit + 1} bases, longer than {limit}"):
            ctx.poa_weighted([["ACGT"], ["ACGT", t[:limit + 1]]], type="ov", gap_extend=e, coverage=True)


def test_struct_sizes_match_the_ctypes_mirror(built, tmp_path):
    from haslr_amd import ctypes_defs as T
    pf = [n for n, _ in T.PoaWeightedParams._fields_]
    of = [n for n, _ in T.WcnsOut._fields_]
    src = tmp_path / "sz.c"
    items = ["sizeof(hx_poa_weighted_params)"] + [f"offsetof(hx_poa_weighted_params,{f})" for f in pf] + ["sizeof(hx_wcns_out)"] + [f"offsetof(hx_wcns_out,{f})" for f in of] + \
            ["sizeof(hx_cns_out)", "sizeof(hx_msa_out)"]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "haslr_types.h"\nint main(){' + "".join(f'printf("%zu\\n",(size_t){it});' for it in items) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    want = [C.sizeof(T.PoaWeightedParams)] + [getattr(T.PoaWeightedParams, f).offset for f in pf] + [C.sizeof(T.WcnsOut)] + [getattr(T.WcnsOut, f).offset for f in of] + \
           [C.sizeof(T.CnsOut), C.sizeof(T.MsaOut)]
    assert got == want
    assert got[0] == 28 and pf == ["match", "mismatch", "gap_open", "gap_extend", "type", "want_coverage", "want_profile"]
    assert of == ["n_set", "cns_off", "cns", "coverage", "profile", "dp_cells", "seq_bases", "n_aligned", "cov_kernel_ms", "cov_kernel_bytes"]
    assert got[-2:] == [48, 96]   # hx_cns_out and hx_msa_out are as they were


@pytest.fixture(scope="module")
def weighted_caller(built, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("spoa_weighted_gpu") / "spoa_weighted_caller")
    lib = os.path.join(ROOT, "haslr_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "spoa_weighted_caller.cpp"), "-o", exe,
                           "-L", lib, "-lhaslr_hip", "-pthread", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


@pytest.mark.parametrize("args", [["--threads", "16"], ["--threads", "1"], ["--batch"]])
def test_header_callers_with_weights_qualities_and_plain_graphs(weighted_caller, ref, args):
    rnd = random.Random(71)
    kinds = [None, (5, -4, -8, -2), (3, -5, -4, 0), (5, -4, -8, -8)]   # None: a four-score engine (5, -4, -8)
    edges, text = [], []
    for k in range(96):
        t = "".join(rnd.choice("ACGT") for _ in range(rnd.randrange(40, 600)))
        st = [noisy(rnd, t, 0.08) for _ in range(rnd.randrange(1, 7))]
        how = "pwqv"[k % 4]   # plain unit-weight graph, one weight per sequence, a quality string, a vector of weights
        if how == "p":
            W = [[1] * len(q) for q in st]
        elif how == "w":
            W = [[rnd.randrange(1, 256)] * len(q) for q in st]
        else:
            W = wgtlib.quality_weights([st], rnd.randrange(10 ** 6))[0] if how == "q" else wgtlib.uniform_weights([st], rnd.randrange(10 ** 6))[0]
        ty, sc, cov = ("sw", "nw", "ov")[k % 3], kinds[(k // 3) % 4], k % 8 < 5
        edges.append((ty, sc, st, W))
        lines = [ty + ("" if sc is None else " " + " ".join(str(v) for v in sc)) + (" +cov" if cov else "")]
        for q, w in zip(st, W):
            lines.append(q if how == "p" else f"{q} w {w[0]}" if how == "w" else f"{q} q {wgtlib.quality_strings([w])[0]}" if how == "q" else f"{q} v {','.join(str(v) for v in w)}")
        if k % 10 == 0:
            lines.insert(2, "- w 5")   # an empty member: ignored by add_alignment as in spoa
        text.append("\n".join(lines))
    r = subprocess.run([weighted_caller] + args, input="\n\n".join(text) + "\n", capture_output=True, text=True, env=dict(os.environ, HASLR_SPOA_BATCH_US="3000"))
    assert r.returncode == 0, r.stderr
    blocks = [blk.split("\n")[:-1] for blk in r.stdout.split("=\n")[:-1]]
    assert len(blocks) == len(edges)
    for k, (ty, sc, st, W) in enumerate(edges):
        want = ref.weighted(st, W, ty, *(sc or (5, -4, -8, -8)))
        assert blocks[k][0] == want.consensus, k
        if k % 8 < 5 or args == ["--batch"]:
            assert [int(v) for v in blocks[k][1].split()] == want.coverage, k
        else:
            assert blocks[k][1] == "-", k


def test_the_header_throws_on_bad_weights(weighted_caller):
    r = subprocess.run([weighted_caller, "--throws"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "throws ok\n", (r.returncode, r.stdout, r.stderr)
