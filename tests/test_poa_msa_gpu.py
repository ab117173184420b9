"""hx_poa_msa on the MI355X: the rows (and the consensus row, and the consensus beside them) equal the CPU restatement
(tests/poa_msa_ref.cpp) character for character - on the CPU tests' sets in three modes, linear and affine, on long sequences, on a
call of 2 000 sets that runs every instance and the persistent workgroups, and with slots capped so small that sets are rerun in larger
ones; the row invariants hold on the GPU output by themselves; the counters and the consensus are those of the consensus-only entries;
header callers mix types and gap models in one process."""
import os
import random
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

import msalib
from test_poa_affine_gpu import many_sets as many_sets_affine
from test_poa_modes_gpu import many_sets
from test_poa_modes_ref import SETS, noisy
from test_poa_msa_ref import check_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
MODES = ["sw", "nw", "ov"]
LINEAR = [(5, -4, -8, -8), (3, -5, -4, -4)]
AFFINE = [(5, -4, -8, -2), (3, -5, -4, 0)]


@pytest.fixture(scope="module")
def ref(built, tmp_path_factory):
    return msalib.MsaRef(str(tmp_path_factory.mktemp("pma_gpu")))


@pytest.fixture(scope="module")
def ctx(built):
    from haslr_amd import hip
    c = hip.HipContext(0)
    yield c
    c.close()


def ref_all(ref, sets, mode, m=5, x=-4, g=-8, e=None, cns=False, threads=16):
    with ThreadPoolExecutor(threads) as ex:   # (the restatement releases the GIL: ctypes)
        return list(ex.map(lambda st: ref.msa(st, mode, m, x, g, e, cns), sets))


def assert_equal(sets, got_rows, got_cns, want, tag):
    bad = [k for k in range(len(sets)) if got_rows[k] != want[k].rows or got_cns[k] != want[k].consensus]
    assert bad == [], (tag, bad[:10])


@pytest.mark.parametrize("cns", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_msa_equals_the_restatement_on_the_cpu_sets(ctx, ref, mode, cns):
    for scores in LINEAR + AFFINE:
        sets = SETS if scores in (LINEAR[0], AFFINE[0]) else SETS[:120]
        want = ref_all(ref, sets, mode, *scores, cns=cns)
        rows, cons, st = ctx.poa_msa(sets, mode, *scores, include_consensus=cns, stats=True)
        assert_equal(sets, rows, cons, want, (mode, scores, cns))
        # the counters are those of the consensus-only entry on the same sets (the general path under every type)
        with ctx.options(poa_general=1):
            only, st0 = ctx.poa_sequences_affine(sets, mode, *scores, stats=True)
        assert only == cons
        assert {k: st[k] for k in ("dp_cells", "seq_bases", "n_aligned")} == st0


@pytest.mark.parametrize("scores", [LINEAR[0], AFFINE[0]])
@pytest.mark.parametrize("mode", MODES)
def test_row_invariants_hold_on_the_gpu_output_by_themselves(ctx, mode, scores):
    rows, cons = ctx.poa_msa(SETS, mode, *scores, include_consensus=True, stats=True)[:2]
    plain = ctx.poa_msa(SETS, mode, *scores)
    for k, st in enumerate(SETS):
        n_cols = len(rows[k][0])
        check_rows(st, rows[k], n_cols, cons[k])
        assert plain[k] == rows[k][:-1], k


def test_the_consensus_beside_the_msa_is_the_consensus_entries(ctx):
    sets = SETS[:200]
    for mode in MODES:   # (under nw the first is the tuned path, which equals the oracle)
        assert ctx.poa_msa(sets, mode, stats=True)[1] == ctx.poa_sequences_mode(sets, mode)
        assert ctx.poa_msa(sets, mode, 5, -4, -8, -2, stats=True)[1] == ctx.poa_sequences_affine(sets, mode, 5, -4, -8, -2)


def test_known_answers(ctx):
    assert ctx.poa_msa([["ACGT", "AGT"], ["ACGT", "", "ACT"], [], [""], ["ACGT", "ACAGT"]], include_consensus=True) == \
        [["ACGT", "A-GT", "ACGT"], ["ACGT", "----", "AC-T", "ACGT"], [""], ["", ""], ["AC-GT", "ACAGT", "ACAGT"]]
    assert ctx.poa_msa([["ACGTACGGTCA", "CGGTCATTGAC", "TTGACCA"]], "ov", include_consensus=True) == \
        [["ACGTACGGTCA-------", "-----CGGTCATTGAC--", "-----------TTGACCA", "ACGTACGGTCATTGACCA"]]
    assert ctx.poa_msa([["A", "C"]], "sw") == [["A-", "-C"]] and ctx.poa_msa([["A", "C"]], "ov", 5, -20, -1) == [["A-", "-C"]]
    st = ["ACGTTTACGGACCA", "ACGTACCA"]
    assert ctx.poa_msa([st])[0][1] == "ACG--T----ACCA" and ctx.poa_msa([st], "nw", 5, -4, -8, -2)[0][1] == "ACGT------ACCA"
    assert ctx.poa_msa([]) == []


@pytest.mark.parametrize("mode", MODES)
def test_long_sequences(ctx, ref, mode):
    rnd = random.Random(31)
    t = "".join(rnd.choice("ACGT") for _ in range(20000))
    for L, e in ((20000, None), (16000, -2)):   # linear, affine
        u = t[:L]
        sets = [[u], [u, noisy(rnd, u, 0.08)], ["ACGTACGT", u[5000:15000], u]]
        want = ref_all(ref, sets, mode, e=e, cns=True, threads=3)
        rows, cons = ctx.poa_msa(sets, mode, gap_extend=e, include_consensus=True, stats=True)[:2]
        assert_equal(sets, rows, cons, want, (mode, L))


@pytest.mark.parametrize("mode", MODES)
def test_two_thousand_sets_in_one_call(ctx, ref, mode):
    sets = many_sets(32, 2000)
    rows, cons = ctx.poa_msa(sets, mode, include_consensus=True, stats=True)[:2]
    assert_equal(sets, rows, cons, ref_all(ref, sets, mode, cns=True), mode)
    sets = many_sets_affine(33, 2000)
    rows, cons = ctx.poa_msa(sets, mode, gap_extend=-6, stats=True)[:2]
    assert_equal(sets, rows, cons, ref_all(ref, sets, mode, e=-6), (mode, "affine"))


@pytest.mark.parametrize("mode", MODES)
def test_sets_rerun_in_larger_slots_give_the_same_rows(ctx, ref, mode):
    sets = many_sets(34, 300)
    for e in (None, -6):
        want = ref_all(ref, sets, mode, e=e, cns=True)
        with ctx.options(poa_modes_slot_kb=1):   # (first-round slots hold little more than the graph pools: sets stop and are rerun)
            rows, cons = ctx.poa_msa(sets, mode, gap_extend=e, include_consensus=True, stats=True)[:2]
        assert_equal(sets, rows, cons, want, (mode, e))


def test_bad_parameters_are_errors(ctx):
    from haslr_amd import hip
    with pytest.raises(hip.HipError, match="hx_poa_msa: the gap open score must be negative"):
        ctx.poa_msa([["ACGT"]], "sw", 5, -4, 0, 0)
    with pytest.raises(hip.HipError, match="hx_poa_msa: the gap extend score must not be positive"):
        ctx.poa_msa([["ACGT"]], "nw", 5, -4, -8, 1)
    with pytest.raises(hip.HipError, match="hx_poa_msa: the gap extend score -8 is below the gap open score -2"):
        ctx.poa_msa([["ACGT"]], "ov", 5, -4, -2, -8)
    with pytest.raises(ValueError, match="unknown alignment type"):
        ctx.poa_msa([["ACGT"]], "xx")
    import ctypes as C

    import numpy as np
    from haslr_amd import ctypes_defs as T
    o, mp = T.MsaOut(), T.PoaMsaParams(5, -4, -8, -2, 3, 0)
    off = np.array([0, 1], dtype=np.uint64)
    soff = np.array([0, 4], dtype=np.uint64)
    assert hip.lib().hx_poa_msa(ctx._h, 1, off.ctypes.data_as(T.u64p), soff.ctypes.data_as(T.u64p), b"ACGT", C.byref(mp), C.byref(o)) != 0
    assert "hx_poa_msa: unknown alignment type 3" in hip.lib().hx_last_error().decode()


def test_a_sequence_over_the_limit_is_an_error_that_names_its_set(ctx):
    from haslr_amd import hip
    rnd = random.Random(36)
    t = "".join(rnd.choice("ACGT") for _ in range(32768))
    for limit, e in ((32767, None), (16383, -2)):
        assert ctx.poa_msa([["ACGT"], [t[:limit]]], "ov", gap_extend=e) == [["ACGT"], [t[:limit]]]
        with pytest.raises(hip.HipError, match=rf"hx_poa_msa: set 2 holds a sequence of {limit + 1} bases, longer than {limit}"):
            ctx.poa_msa([["ACGT"], ["ACGT", "ACGA"], ["ACGT", t[:limit + 1]]], "ov", gap_extend=e)


@pytest.fixture(scope="module")
def msa_caller(built, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("spoa_msa_gpu") / "spoa_msa_caller")
    lib = os.path.join(ROOT, "haslr_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "spoa_msa_caller.cpp"), "-o", exe,
                           "-L", lib, "-lhaslr_hip", "-pthread", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


@pytest.mark.parametrize("args", [["--threads", "16"], ["--batch"]])
def test_header_callers_of_mixed_types_and_gap_models(msa_caller, ref, args):
    rnd = random.Random(37)
    kinds = [None, (5, -4, -8, -2), (3, -5, -4, 0), (5, -4, -8, -8)]   # None: a four-score engine (5, -4, -8)
    edges = []
    for k in range(96):
        t = "".join(rnd.choice("ACGT") for _ in range(rnd.randrange(40, 600)))
        st = [noisy(rnd, t, 0.08) for _ in range(rnd.randrange(1, 7))]
        if k % 10 == 0:
            st.insert(1, "")   # an empty member: ignored by add_alignment as in spoa, so it has no row
        edges.append((("sw", "nw", "ov")[k % 3], kinds[(k // 3) % 4], k % 2 == 1, st))
    text = "\n\n".join(ty + ("" if sc is None else " " + " ".join(str(v) for v in sc)) + (" +c" if c else "") + "\n" + "\n".join(q or "-" for q in st)
                       for ty, sc, c, st in edges) + "\n"
    r = subprocess.run([msa_caller] + args, input=text, capture_output=True, text=True, env=dict(os.environ, HASLR_SPOA_BATCH_US="3000"))
    assert r.returncode == 0, r.stderr
    got = [blk.split("\n")[:-1] for blk in r.stdout.split("=\n")[:-1]]
    want = [ref.rows([q for q in st if q], ty, *(sc or (5, -4, -8, -8)), include_consensus=c) for ty, sc, c, st in edges]
    assert got == want
