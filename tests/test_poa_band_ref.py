"""The CPU restatement of adaptive banded alignment (tests/poa_band_ref.cpp) against what is known without it: with a window that holds
every column it is, field for field, the existing restatement of the gap model (linear, affine, convex; tests/poa_modes_ref.cpp and the
files that include it); the hand-built escalation case misses at w = 8, ends on a larger band and does not miss at w = 64; a set that misses
every band ends on the full matrix; identical sequences keep the narrowest band."""
import random

import pytest

import bandlib
import cvxlib
import msalib
import wgtlib

MODES = ["sw", "nw", "ov"]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return bandlib.BandRef(str(tmp_path_factory.mktemp("band_ref")))


@pytest.fixture(scope="module")
def full(tmp_path_factory):
    return cvxlib.ConvexRef(str(tmp_path_factory.mktemp("band_cvx")))


def seeded_sets(seed, n=12):
    rnd = random.Random(seed)
    return [bandlib.copies(rnd.randrange(1 << 30), rnd.randrange(20, 90), rnd.randrange(2, 7), rnd.uniform(0.05, 0.3)) for _ in range(n)] + [["ACGT", "", "A", "TTTT"], ["A"], [""], []]


@pytest.mark.parametrize("mode", MODES)
def test_a_window_that_holds_every_column_is_the_convex_restatement(ref, full, mode):
    # (the windowed DP is kept where the rules send the set to the full matrix: force_window)
    for st in seeded_sets(1):
        w = max(1, max([len(q) for q in st] + [0]))   # B = 2 w + 1 >= Lmax + 1
        wts = wgtlib.uniform_weights([st], 2)[0]
        rec, cells, reruns = ref.banded_cells(st, w, mode, bandlib.CONVEX, include_consensus=True, force_window=True)
        msa = full.msa(st, mode, bandlib.CONVEX, include_consensus=True)
        assert (rec.consensus, rec.rows) == (msa.consensus, msa.rows) and rec.band_used == w and reruns == 0
        wrec = ref.banded(st, w, mode, bandlib.CONVEX, weights=wts, force_window=True)
        want = full.weighted(st, wts, mode, bandlib.CONVEX)
        assert (wrec.consensus, wrec.coverage, wrec.profile) == (want.consensus, want.coverage, want.profile)
        # cells: V x (L + 1) inside a window that holds every column, V x L on the full matrix - V more per alignment
        plain, pcells, _ = ref.banded_cells(st, w, mode, bandlib.CONVEX, include_consensus=True)
        assert plain == rec._replace(band_used=0) and pcells == full.consensus_cells(st, mode, bandlib.CONVEX)[1] <= cells


@pytest.mark.parametrize("model", ["linear", "affine"])
@pytest.mark.parametrize("mode", MODES)
def test_and_the_linear_and_the_affine_one(ref, tmp_path_factory, mode, model):
    # (their own restatements, through the MSA loader: the tracebacks of the three models differ where scores tie)
    mref = msalib.MsaRef(str(tmp_path_factory.mktemp("band_msa")))
    sc = bandlib.MODELS[model]
    for st in seeded_sets(3):
        w = max(1, max([len(q) for q in st] + [0]))
        rec = ref.banded(st, w, mode, sc, include_consensus=True, force_window=True)
        want = mref.msa(st, mode, sc[0], sc[1], sc[2], sc[3], include_consensus=True)
        assert (rec.consensus, rec.rows) == (want.consensus, want.rows)
        assert ref.banded(st, w, mode, sc, include_consensus=True) == rec._replace(band_used=0)


def test_the_escalation_case(ref):
    for model, sc in bandlib.MODELS.items():
        rec, cells, reruns = ref.banded_cells(bandlib.ESC_SET, 8, "nw", sc)
        assert (rec.band_used, reruns) == (32, 2), model   # 17 and 33 columns do not reach the end cell past 40 extra bases at the front, 65 do
        assert cells == 200 * 65
        wide, _, reruns64 = ref.banded_cells(bandlib.ESC_SET, 64, "nw", sc)
        assert (wide.band_used, reruns64) == (64, 0)
        # 129 columns hold the true alignment, the full matrix's; 65 reach the end cell on another path (a band bounds the search, it does not prove the optimum)
        assert wide.consensus == ref.banded(bandlib.ESC_SET, 0, "nw", sc).consensus
        # local and overlap alignment have an end cell inside any band
        for mode in ("sw", "ov"):
            assert ref.banded_cells(bandlib.ESC_SET, 8, mode, sc)[2] == 0


def test_the_last_rung_is_the_full_matrix(ref):
    rec, cells, reruns = ref.banded_cells(bandlib.LAST_RUNG_SET, 8, "nw")
    assert rec.band_used == 0 and reruns == len(bandlib.ladder(8, 2400)) - 1 == 6 and cells == 200 * 2400
    assert bandlib.ladder(8, 2400) == [8, 16, 32, 64, 128, 256, 0] and bandlib.ladder(300, 2400) == [300, 0] and bandlib.ladder(8, 16) == [0] and bandlib.ladder(8, 17) == [8, 0]
    assert rec == ref.banded(bandlib.LAST_RUNG_SET, 0, "nw")


def test_identical_sequences_keep_the_narrowest_band(ref):
    t = bandlib.template(random.Random(5), 120)
    for model, sc in bandlib.MODELS.items():
        for mode in MODES:
            rec, cells, reruns = ref.banded_cells([t] * 4, 1, mode, sc, include_consensus=True)
            assert rec.consensus == t and rec.band_used == 1 and reruns == 0 and rec.rows == [t] * 5 and cells == 3 * 120 * 3


def test_the_two_branch_set_is_followed_at_w_8(ref):
    for model, sc in bandlib.TWO_BRANCH.items():
        st = bandlib.two_branch_set(700)
        rec, _, reruns = ref.banded_cells(st, 8, "nw", sc)
        assert reruns == 0 and rec.band_used == 8 and rec == ref.banded(st, 0, "nw", sc)._replace(band_used=8)
        assert "-" * 150 in rec.rows[1] and "T" * 150 in rec.rows[2]
