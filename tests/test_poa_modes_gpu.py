"""hx_poa_sequences_mode on the MI355X: kSW and kOV through the general path (kernels/poa_modes.hip) equal the CPU restatement
(tests/poa_modes_ref.cpp) bit for bit - on the CPU tests' sets, on sequences of 20 000 bases, on a call of thousands of sets that runs every
instance and the persistent workgroups, and with slots capped so small that every set is rerun in a larger one; kNW through the new entry is
hx_poa_sequences, and kNW through the general path (option poa_general) is the oracle's consensus."""
import os
import random
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

import orclib
import pmrlib
from test_poa_modes_ref import SETS, TRIPLES, noisy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref(built, tmp_path_factory):
    return pmrlib.ModesRef(str(tmp_path_factory.mktemp("pmr_gpu")))


@pytest.fixture(scope="module")
def ctx(built):
    from haslr_amd import hip
    c = hip.HipContext(0)
    yield c
    c.close()


def ref_all(ref, sets, mode, m=5, x=-4, g=-8):
    with ThreadPoolExecutor(16) as ex:   # (the restatement releases the GIL: ctypes)
        res = list(ex.map(lambda st: ref.consensus_cells(st, mode, m, x, g), sets))
    return [r[0] for r in res], sum(r[1] for r in res)


def many_sets(seed, n):
    """n sets whose longest sequences fall in every instance of the general path (up to 1023, 4095, 8191 and 32767 bases + 1 columns)"""
    rnd = random.Random(seed)
    out = []
    for k in range(n):
        L = rnd.choice([1, 3, 30, 120, 400, 900]) if k % 50 else rnd.choice([1500, 3000, 5000, 9500])
        t = "".join(rnd.choice("ACGT") for _ in range(L))
        out.append([noisy(rnd, t, 0.1) for _ in range(rnd.randrange(1, 5 if L < 1000 else 3))])
    return out


@pytest.mark.parametrize("mode", ["sw", "ov"])
def test_modes_equal_the_restatement_on_the_cpu_sets(ctx, ref, mode):
    for triple in TRIPLES:
        sets = SETS if triple == (5, -4, -8) else SETS[:120]
        want, cells = ref_all(ref, sets, mode, *triple)
        got, st = ctx.poa_sequences_mode(sets, mode, *triple, stats=True)
        for k in range(len(sets)):
            assert got[k] == want[k], (mode, triple, k)
        assert st["dp_cells"] == cells
        assert st["seq_bases"] == sum(len(q) for s in sets for q in s) and st["n_aligned"] == sum(1 for s in sets for q in s if q)


@pytest.mark.parametrize("mode", ["sw", "ov"])
def test_sequences_of_20000_bases(ctx, ref, mode):
    rnd = random.Random(21)
    t = "".join(rnd.choice("ACGT") for _ in range(20000))
    sets = [[t], [t, noisy(rnd, t, 0.08)], ["ACGTACGT", t[5000:15000], t]]
    assert ctx.poa_sequences_mode(sets, mode) == ref_all(ref, sets, mode)[0]


@pytest.mark.parametrize("mode", ["sw", "ov"])
def test_thousands_of_sets_in_one_call(ctx, ref, mode):
    sets = many_sets(22, 2000)
    want, cells = ref_all(ref, sets, mode)
    got, st = ctx.poa_sequences_mode(sets, mode, stats=True)
    assert [k for k in range(len(sets)) if got[k] != want[k]] == []
    assert st["dp_cells"] == cells


@pytest.mark.parametrize("mode", ["sw", "ov"])
def test_overflowing_slots_are_rerun_in_larger_ones(ctx, ref, mode):
    sets = many_sets(23, 300)
    want = ref_all(ref, sets, mode)[0]
    with ctx.options(poa_modes_slot_kb=1):   # (first-round slots hold little more than the largest graph pools of their instance: sets stop and are rerun)
        got = ctx.poa_sequences_mode(sets, mode)
    assert [k for k in range(len(sets)) if got[k] != want[k]] == []


def test_nw_through_the_new_entry_is_the_tuned_path(ctx):
    sets = SETS[:200]
    assert ctx.poa_sequences_mode(sets, "nw") == ctx.poa_sequences(sets)
    assert ctx.poa_sequences_mode(sets, "nw", 3, -5, -4) == ctx.poa_sequences(sets, 3, -5, -4)
    # (both sides above are one tuned call: what it computes under 3 / -5 / -4 is the oracle's consensus)
    got = ctx.poa_sequences_mode(sets, "nw", 3, -5, -4)
    with ThreadPoolExecutor(16) as ex:
        want = list(ex.map(lambda st: orclib.poa_consensus(st, 3, -5, -4), sets))
    assert [k for k in range(len(sets)) if got[k] != want[k]] == []


def test_nw_through_the_general_path_is_the_oracle(ctx):
    with ctx.options(poa_general=1):
        for triple in TRIPLES:
            sets = SETS if triple == (5, -4, -8) else SETS[:120]
            got = ctx.poa_sequences_mode(sets, "nw", *triple)
            assert [k for k in range(len(sets)) if got[k] != orclib.poa_consensus(sets[k], *triple)] == [], triple
        sets = many_sets(24, 400)
        got = ctx.poa_sequences_mode(sets, "nw")
        assert [k for k in range(len(sets)) if got[k] != orclib.poa_consensus(sets[k])] == []


def test_bad_parameters_are_errors(ctx):
    from haslr_amd import hip
    with pytest.raises(hip.HipError, match="gap score must be negative"):
        ctx.poa_sequences_mode([["ACGT"]], "sw", 5, -4, 0)
    import ctypes as C

    import numpy as np
    from haslr_amd import ctypes_defs as T
    o, mp = T.CnsOut(), T.PoaModeParams(5, -4, -8, 3)
    off = np.array([0, 1], dtype=np.uint64)
    soff = np.array([0, 4], dtype=np.uint64)
    assert hip.lib().hx_poa_sequences_mode(ctx._h, 1, off.ctypes.data_as(T.u64p), soff.ctypes.data_as(T.u64p), b"ACGT", C.byref(mp), C.byref(o)) != 0
    assert "unknown alignment type" in hip.lib().hx_last_error().decode()


@pytest.fixture(scope="module")
def modes_caller(built, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("spoa_modes_gpu") / "spoa_modes_caller")
    lib = os.path.join(ROOT, "haslr_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "spoa_modes_caller.cpp"), "-o", exe,
                           "-L", lib, "-lhaslr_hip", "-pthread", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


@pytest.mark.parametrize("args", [["--threads", "16"], ["--batch"]])
def test_header_callers_with_engines_of_mixed_types(modes_caller, ref, args):
    rnd = random.Random(25)
    edges = []
    for k in range(96):
        t = "".join(rnd.choice("ACGT") for _ in range(rnd.randrange(40, 600)))
        edges.append((("sw", "nw", "ov")[k % 3], [noisy(rnd, t, 0.08) for _ in range(rnd.randrange(1, 7))]))
    text = "\n\n".join(ty + "\n" + "\n".join(st) for ty, st in edges) + "\n"
    r = subprocess.run([modes_caller] + args, input=text, capture_output=True, text=True, env=dict(os.environ, HASLR_SPOA_BATCH_US="3000"))
    assert r.returncode == 0, r.stderr
    assert r.stdout.split("\n")[:-1] == [ref.consensus(st, ty) for ty, st in edges]
