"""hx_poa_sequences_affine on the MI355X: the affine instances of the general path (kernels/poa_modes.hip) equal the CPU restatement
(tests/poa_affine_ref.cpp) bit for bit - on the CPU tests' sets in three modes and five score sets, on sequences of 16 000 bases, on a call
of 2 000 sets that runs every affine instance and the persistent workgroups, and with slots capped so small that sets are rerun in larger
ones; gap_extend == gap_open through the new entry is hx_poa_sequences_mode, and under option poa_affine the affine kernel gives the same
strings (under kNW the oracle's); header callers mix linear and affine engines of every type in one process."""
import os
import random
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

import orclib
import parlib
import pmrlib
from test_poa_modes_ref import SETS, TRIPLES, noisy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
MODES = ["sw", "nw", "ov"]
# (match, mismatch, gap open, gap extend): one with e = 0, two with g = e - 1
SCORES = [(5, -4, -8, -2), (5, -4, -8, -6), (3, -5, -4, 0), (2, -7, -2, -1), (1, -1, -3, -2)]
MAX_LEN = 16383   # the longest sequence an affine call takes (include/haslr_hip.h)


@pytest.fixture(scope="module")
def ref(built, tmp_path_factory):
    return parlib.AffineRef(str(tmp_path_factory.mktemp("par_gpu")))


@pytest.fixture(scope="module")
def lin(built, tmp_path_factory):
    return pmrlib.ModesRef(str(tmp_path_factory.mktemp("par_gpu_pmr")))


@pytest.fixture(scope="module")
def ctx(built):
    from haslr_amd import hip
    c = hip.HipContext(0)
    yield c
    c.close()


def ref_all(ref, sets, mode, m=5, x=-4, g=-8, e=-6, threads=16):
    with ThreadPoolExecutor(threads) as ex:   # (the restatement releases the GIL: ctypes)
        res = list(ex.map(lambda st: ref.consensus_cells(st, mode, m, x, g, e), sets))
    return [r[0] for r in res], sum(r[1] for r in res)


def many_sets(seed, n):
    """n sets whose longest sequences fall in every affine instance of the general path (up to 1023, 4095, 8191 and 16383 bases + 1 columns)"""
    rnd = random.Random(seed)
    out = []
    for k in range(n):
        L = rnd.choice([1, 3, 30, 120, 400, 900]) if k % 50 else rnd.choice([1500, 3000, 5000, 9500])
        t = "".join(rnd.choice("ACGT") for _ in range(L))
        out.append([noisy(rnd, t, 0.1) for _ in range(rnd.randrange(1, 5 if L < 1000 else 3))])
    return out


@pytest.mark.parametrize("mode", MODES)
def test_affine_equals_the_restatement_on_the_cpu_sets(ctx, ref, mode):
    for scores in SCORES:
        sets = SETS if scores == SCORES[0] else SETS[:120]
        want, cells = ref_all(ref, sets, mode, *scores)
        got, st = ctx.poa_sequences_affine(sets, mode, *scores, stats=True)
        for k in range(len(sets)):
            assert got[k] == want[k], (mode, scores, k)
        assert st["dp_cells"] == cells
        assert st["seq_bases"] == sum(len(q) for s in sets for q in s) and st["n_aligned"] == sum(1 for s in sets for q in s if q)


@pytest.mark.parametrize("mode", MODES)
def test_sequences_of_16000_bases(ctx, ref, mode):
    rnd = random.Random(21)
    t = "".join(rnd.choice("ACGT") for _ in range(20000))[:16000]
    sets = [[t], [t, noisy(rnd, t, 0.08)], ["ACGTACGT", t[5000:15000], t]]
    assert max(len(q) for st in sets for q in st) <= MAX_LEN
    assert ctx.poa_sequences_affine(sets, mode) == ref_all(ref, sets, mode, threads=3)[0]


def test_a_sequence_a_base_over_the_limit_is_an_error_that_names_its_set(ctx):
    from haslr_amd import hip
    rnd = random.Random(26)
    t = "".join(rnd.choice("ACGT") for _ in range(MAX_LEN + 1))
    assert ctx.poa_sequences_affine([["ACGT"], [t[:MAX_LEN]]], "ov") == ["ACGT", t[:MAX_LEN]]
    with pytest.raises(hip.HipError, match=rf"set 2 holds a sequence of {MAX_LEN + 1} bases, longer than {MAX_LEN}"):
        ctx.poa_sequences_affine([["ACGT"], ["ACGT", "ACGA"], ["ACGT", t]], "ov")


@pytest.mark.parametrize("mode", MODES)
def test_two_thousand_sets_in_one_call(ctx, ref, mode):
    sets = many_sets(22, 2000)
    want, cells = ref_all(ref, sets, mode)
    got, st = ctx.poa_sequences_affine(sets, mode, stats=True)
    assert [k for k in range(len(sets)) if got[k] != want[k]] == []
    assert st["dp_cells"] == cells


@pytest.mark.parametrize("mode", MODES)
def test_overflowing_slots_are_rerun_in_larger_ones(ctx, ref, mode):
    sets = many_sets(23, 300)
    want = ref_all(ref, sets, mode, 5, -4, -8, -6)[0]
    with ctx.options(poa_modes_slot_kb=1):   # (first-round slots hold little more than the largest graph pools of their instance: sets stop and are rerun)
        got = ctx.poa_sequences_affine(sets, mode, 5, -4, -8, -6)
    assert [k for k in range(len(sets)) if got[k] != want[k]] == []


def test_equal_scores_through_the_new_entry_are_the_mode_entry(ctx):
    sets = SETS[:200]
    for mode in MODES:
        assert ctx.poa_sequences_affine(sets, mode, 5, -4, -8, -8) == ctx.poa_sequences_mode(sets, mode)
        assert ctx.poa_sequences_affine(sets, mode, 3, -5, -4, -4) == ctx.poa_sequences_mode(sets, mode, 3, -5, -4)


def test_equal_scores_through_the_affine_kernel_are_the_linear_results(ctx, lin):
    with ctx.options(poa_affine=1):
        for triple in TRIPLES:
            m, x, g = triple
            sets = SETS if triple == (5, -4, -8) else SETS[:120]
            for mode in MODES:
                got, st = ctx.poa_sequences_affine(sets, mode, m, x, g, g, stats=True)
                if mode == "nw":
                    want = [orclib.poa_consensus(s, *triple) for s in sets]
                else:
                    with ThreadPoolExecutor(16) as ex:
                        res = list(ex.map(lambda s: lin.consensus_cells(s, mode, *triple), sets))
                    want = [r[0] for r in res]
                    assert st["dp_cells"] == sum(r[1] for r in res)
                assert [k for k in range(len(sets)) if got[k] != want[k]] == [], (triple, mode)
    # the option is what sent them there: the affine kernel fills the whole matrix, the tuned kNW path prunes
    sets = SETS[:60]
    full = sum(c for _, c in (lin.consensus_cells(s, "nw") for s in sets))
    with ctx.options(poa_affine=1):
        assert ctx.poa_sequences_affine(sets, "nw", 5, -4, -8, -8, stats=True)[1]["dp_cells"] == full


def test_bad_parameters_are_errors(ctx):
    from haslr_amd import hip
    with pytest.raises(hip.HipError, match="gap open score must be negative"):
        ctx.poa_sequences_affine([["ACGT"]], "sw", 5, -4, 0, 0)
    with pytest.raises(hip.HipError, match="gap extend score must not be positive"):
        ctx.poa_sequences_affine([["ACGT"]], "nw", 5, -4, -8, 1)
    with pytest.raises(hip.HipError, match="gap extend score -8 is below the gap open score -2"):
        ctx.poa_sequences_affine([["ACGT"]], "ov", 5, -4, -2, -8)
    import ctypes as C

    import numpy as np
    from haslr_amd import ctypes_defs as T
    o, ap = T.CnsOut(), T.PoaAffineParams(5, -4, -8, -2, 3)
    off = np.array([0, 1], dtype=np.uint64)
    soff = np.array([0, 4], dtype=np.uint64)
    assert hip.lib().hx_poa_sequences_affine(ctx._h, 1, off.ctypes.data_as(T.u64p), soff.ctypes.data_as(T.u64p), b"ACGT", C.byref(ap), C.byref(o)) != 0
    assert "unknown alignment type 3" in hip.lib().hx_last_error().decode()


@pytest.fixture(scope="module")
def affine_caller(built, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("spoa_affine_gpu") / "spoa_affine_caller")
    lib = os.path.join(ROOT, "haslr_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "spoa_affine_caller.cpp"), "-o", exe,
                           "-L", lib, "-lhaslr_hip", "-pthread", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


@pytest.mark.parametrize("args", [["--threads", "16"], ["--batch"]])
def test_header_callers_with_linear_and_affine_engines_of_mixed_types(affine_caller, ref, lin, args):
    rnd = random.Random(27)
    kinds = [None, (5, -4, -8, -2), (3, -5, -4, 0), (5, -4, -8, -8)]   # None: a four-score engine (5, -4, -8)
    edges = []
    for k in range(96):
        t = "".join(rnd.choice("ACGT") for _ in range(rnd.randrange(40, 600)))
        edges.append((("sw", "nw", "ov")[k % 3], kinds[(k // 3) % 4], [noisy(rnd, t, 0.08) for _ in range(rnd.randrange(1, 7))]))
    text = "\n\n".join(ty + ("" if sc is None else " " + " ".join(str(v) for v in sc)) + "\n" + "\n".join(st) for ty, sc, st in edges) + "\n"
    r = subprocess.run([affine_caller] + args, input=text, capture_output=True, text=True, env=dict(os.environ, HASLR_SPOA_BATCH_US="3000"))
    assert r.returncode == 0, r.stderr
    want = [lin.consensus(st, ty) if sc is None else ref.consensus(st, ty, *sc) for ty, sc, st in edges]
    assert r.stdout.split("\n")[:-1] == want
