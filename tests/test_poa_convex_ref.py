"""The CPU restatement of the POA under two-piece affine (convex) gaps (tests/poa_convex_ref.cpp, DESIGN.md "General POA path", "Convex
gaps"), without a GPU: with a second piece that never wins it is the affine restatement pair for pair (with four equal gap scores the linear
one, and under kNW the oracle), its end scores are those of a plain pairwise two-piece Gotoh written here, the seeded pairs separate the
model from both of its pieces, two hand-derived cases pin the walk, and the MSA rows and the coverage keep their invariants."""
import random
from concurrent.futures import ThreadPoolExecutor

import pytest

import cvxlib
import orclib
import parlib
import pmrlib
from test_poa_modes_ref import SETS

MODES = ["sw", "nw", "ov"]
NEG = -10**9
# (match, mismatch, g, e, q, c): spoa's defaults, a second piece that opens dear and extends almost free, and one with c = 0 and g == e
CONVEX_SCORES = [(5, -4, -8, -6, -10, -4), (5, -4, -8, -6, -24, -1), (2, -7, -2, -2, -9, 0)]


@pytest.fixture(scope="module")
def cvx(built, tmp_path_factory):
    return cvxlib.ConvexRef(str(tmp_path_factory.mktemp("cvx")))


@pytest.fixture(scope="module")
def aff(built, tmp_path_factory):
    return parlib.AffineRef(str(tmp_path_factory.mktemp("cvx_par")))


@pytest.fixture(scope="module")
def lin(built, tmp_path_factory):
    return pmrlib.ModesRef(str(tmp_path_factory.mktemp("cvx_pmr")))


def indel_noisy(rnd, t, noise=0.03, indel=0.01, lo=8, hi=40):
    """copy of t with 1-base noise (substitutions, insertions, deletions) at rate `noise`, and deletions and insertions of lo..hi bases
    starting at rate `indel` per position each"""
    out, k = [], 0
    while k < len(t):
        r = rnd.random()
        if r < indel:
            k += rnd.randrange(lo, hi + 1)
            continue
        if r < 2 * indel:
            out.append("".join(rnd.choice("ACGT") for _ in range(rnd.randrange(lo, hi + 1))))
        elif r < 2 * indel + noise / 3:
            k += 1
            continue
        elif r < 2 * indel + 2 * noise / 3:
            out.append(rnd.choice("ACGT"))
            k += 1
            continue
        elif r < 2 * indel + noise:
            out.append(rnd.choice("ACGT"))
        out.append(t[k])
        k += 1
    return "".join(out) or "A"


def long_pairs(seed, n):
    """templates of 150-300 bases against copies with 1-base noise and indels of 8-40 bases at about 1 % per position each"""
    rnd = random.Random(seed)
    out = []
    for _ in range(n):
        a = "".join(rnd.choice("ACGT") for _ in range(rnd.randrange(150, 301)))
        out.append((a, indel_noisy(rnd, a)))
    return out


def short_pairs(seed, n):
    """templates of 12-48 bases against copies with 1-base noise and indels of 2-12 bases (both pieces win on some), a third of them with
    overhangs, so that the local and overlap ends are not the corners"""
    rnd = random.Random(seed)
    out = []
    for _ in range(n):
        a = "".join(rnd.choice("ACGT") for _ in range(rnd.randrange(12, 49)))
        b = indel_noisy(rnd, a, noise=0.06, indel=0.03, lo=2, hi=12)
        if rnd.random() < 0.3:
            a = "".join(rnd.choice("ACGT") for _ in range(rnd.randrange(0, 8))) + a
            b = b + "".join(rnd.choice("ACGT") for _ in range(rnd.randrange(0, 8)))
        out.append((a, b))
    return out


LONG_PAIRS = long_pairs(131, 60)
GOTOH_PAIRS = short_pairs(137, 300) + LONG_PAIRS[:4]


def all_sets(fn, sets):
    with ThreadPoolExecutor(16) as ex:   # (the restatements release the GIL and keep the last alignment per thread)
        return list(ex.map(fn, sets))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("second", ["the first piece again", "strictly dominated"])
def test_a_second_piece_that_never_wins_is_the_affine_restatement(cvx, aff, mode, second):
    m, x, g, e = 5, -4, -8, -6
    q, c = (g, e) if second == "the first piece again" else (g - 1, e - 1)

    def both(st):
        a = cvx.consensus_cells(st, mode, (m, x, g, e, q, c))
        pa = cvx.last_alignment()
        b = aff.consensus_cells(st, mode, m, x, g, e)
        return a, pa, b, aff.last_alignment()

    for k, (a, pa, b, pb) in enumerate(all_sets(both, SETS)):
        assert a == b, (mode, second, k)
        assert pa == pb, (mode, second, k)


@pytest.mark.parametrize("mode", MODES)
def test_four_equal_gap_scores_are_the_linear_restatement(cvx, lin, mode):
    for m, x, g in [(5, -4, -8), (3, -5, -4)]:
        sets = SETS if g == -8 else SETS[:120]

        def both(st):
            a = cvx.consensus_cells(st, mode, (m, x, g, g, g, g))
            pa = cvx.last_alignment()
            b = lin.consensus_cells(st, mode, m, x, g)
            return a, pa, b, lin.last_alignment()

        res = all_sets(both, sets)
        for k, (a, pa, b, pb) in enumerate(res):
            assert a == b, (mode, g, k)
            assert pa == pb, (mode, g, k)
        if mode == "nw":
            for k, st in enumerate(sets):
                assert res[k][0][0] == orclib.poa_consensus(st, m, x, g), (g, k)


def gotoh2(a, b, mode, m, x, g, e, q, c):
    """end score of b against a by the textbook recurrences with two gap pieces: M ends in a pair, X1 / X2 in a base of a against a gap
    under the first / second piece, Y1 / Y2 in a base of b against a gap; global, local (0 when nothing is above 0) and overlap (free ends
    on both sequences) ends"""
    n, L = len(a), len(b)
    free = mode != "nw"
    best = 0 if mode == "sw" else NEG
    # the previous row: X1, X2 and the cell maximum T (row 0: M = 0 at the free ends, else Y1 and Y2 of the boundary)
    pX1, pX2 = [NEG] * (L + 1), [NEG] * (L + 1)
    pT = [0] * (L + 1)
    for j in range(1, L + 1):
        if not free:
            pT[j] = max(g + (j - 1) * e, q + (j - 1) * c)
    for i in range(1, n + 1):
        X1, X2, T = [NEG] * (L + 1), [NEG] * (L + 1), [NEG] * (L + 1)
        if free:
            T[0] = 0
        else:
            X1[0], X2[0] = g + (i - 1) * e, q + (i - 1) * c
            T[0] = max(X1[0], X2[0])
        y1 = y2 = NEG
        ai = a[i - 1]
        for j in range(1, L + 1):
            mm = pT[j - 1] + (m if ai == b[j - 1] else x)
            if mode == "sw" and mm < 0:
                mm = 0
            x1 = max(pT[j] + g, pX1[j] + e)
            x2 = max(pT[j] + q, pX2[j] + c)
            y1 = max(T[j - 1] + g, y1 + e)
            y2 = max(T[j - 1] + q, y2 + c)
            X1[j], X2[j] = x1, x2
            h = T[j] = max(mm, x1, x2, y1, y2)
            if (mode == "sw" or (mode == "ov" and (i == n or j == L))) and h > best:
                best = h
        pX1, pX2, pT = X1, X2, T
    return pT[L] if mode == "nw" else best


@pytest.mark.parametrize("mode", MODES)
def test_end_scores_are_two_piece_gotoh_on_chains(cvx, mode):
    assert len(GOTOH_PAIRS) >= 300
    for scores in CONVEX_SCORES + [(5, -4, -8, -6, -8, -6), (1, -1, -3, -2, -5, -1)]:
        for k, (a, b) in enumerate(GOTOH_PAIRS):
            assert cvx.align_pair(a, b, mode, scores)[1] == gotoh2(a, b, mode, *scores), (mode, scores, k, a, b)


@pytest.mark.parametrize("mode", MODES)
def test_the_seeded_pairs_separate_the_model_from_both_of_its_pieces(cvx, aff, mode):
    for scores in CONVEX_SCORES:
        m, x, g, e, q, c = scores
        differ = 0
        for a, b in LONG_PAIRS:
            s = cvx.align_pair(a, b, mode, scores)[1]
            differ += s != aff.align_pair(a, b, mode, m, x, g, e)[1] and s != aff.align_pair(a, b, mode, m, x, q, c)[1]
        print(f"{mode} {scores}: the end score differs from affine(g, e) and from affine(q, c) on {differ} of {len(LONG_PAIRS)} pairs")
        assert 2 * differ >= len(LONG_PAIRS), (mode, scores, differ)


def test_a_deleted_block_is_one_gap_under_the_second_piece(cvx, aff):
    """Chain AACCGGAG TTTTTTTTTT CAGACAGA (nodes 0-7, 8-17, 18-25), sequence AACCGGAG CAGACAGA (the ten T of nodes 8-17 are missing), kSW,
    (5, -4, -8, -6, -24, -1). A gap of 10 nodes scores max(-8 - 9 * 6, -24 - 9 * 1) = max(-62, -33) = -33: the second piece. Both flanks
    matched around that gap: 8 * 5 - 33 + 8 * 5 = 47, more than the 40 of one flank alone, so the local alignment spans the gap and ends
    at (26, 16) = 47. The walk takes the diagonal over nodes 25-18 down to (18, 8) = 47 - 40 = 7. There no diagonal fits (node 17 is T,
    position 7 is G), and F[18][8] is at most H[8][8] - 62 = -22, so H is not F; it is O: O[9][8] = H[8][8] + q = 40 - 24 = 16 opens the
    gap at node 8 and nine extensions (c = -1) take it to O[18][8] = 7. State O passes nodes 17-9 on extensions and node 8 on the open,
    and the diagonal runs over nodes 7-0 to H[0][0] = 0, where kSW stops.
    Under affine (5, -4, -8, -6) the same gap scores -62: 80 - 62 = 18 is less than one flank, the best local alignment is a flank of 40,
    and the first maximum in row-major order is the first flank's end (8, 8)."""
    chain, seq = "AACCGGAG" + "T" * 10 + "CAGACAGA", "AACCGGAG" + "CAGACAGA"
    pairs, score = cvx.align_pair(chain, seq, "sw", (5, -4, -8, -6, -24, -1))
    assert score == 47
    assert pairs == [(k, k) for k in range(8)] + [(k, -1) for k in range(8, 18)] + [(k, k - 10) for k in range(18, 26)]
    pairs, score = aff.align_pair(chain, seq, "sw", 5, -4, -8, -6)
    assert (pairs, score) == ([(k, k) for k in range(8)], 40)


def test_an_inserted_block_is_one_gap_resolved_by_its_length(cvx, aff):
    """Chain ACGGACG CAGGCAA (nodes 0-6, 7-13), sequence ACGGACG TTTTTT CAGGCAA (six T inserted after position 6), kSW, spoa's defaults
    (5, -4, -8, -6, -10, -4). A gap of 6 bases scores max(-8 - 5 * 6, -10 - 5 * 4) = max(-38, -30) = -30: the second piece (w(1) = -8
    by the first piece, w(2) = -14 by both, from 3 bases on the second piece is ahead). Both flanks around the gap: 35 - 30 + 35 = 40,
    more than the 35 of one flank, so the local alignment spans the insertion and ends at (14, 20) = 40. The diagonal runs over nodes 13-7
    to (7, 13) = 40 - 35 = 5. There no diagonal fits (node 6 is G, position 12 is T), and a vertical gap into (7, 13) would have to come
    down column 13 from a cell of at least 5 + 8 = 13, which the T column does not hold: H is neither F nor O. Rule 4 looks for the
    smallest k with H[7][13] == H[7][13 - k] + w(k). For k = 1..5 the cell (7, 13 - k) lies on the same gap, H[7][13 - k] = 35 + w(6 - k),
    and w(6 - k) + w(k) is -8 - 26 = -34, -14 - 22 = -36, -18 - 18 = -36, -36 and -34: all below w(6) = -30, as two gaps always score
    below one of their joint length. k = 6 meets H[7][7] = 35, and 35 - 30 = 5. Six pairs (-1, 12) ... (-1, 7), then the diagonal over
    nodes 6-0.
    Under affine (5, -4, -8, -6) the insertion scores -38: 70 - 38 = 32 is less than one flank's 35, and the first maximum in row-major
    order is the first flank's end (7, 7)."""
    chain, seq = "ACGGACG" + "CAGGCAA", "ACGGACG" + "TTTTTT" + "CAGGCAA"
    pairs, score = cvx.align_pair(chain, seq, "sw", (5, -4, -8, -6, -10, -4))
    assert score == 40
    assert pairs == [(k, k) for k in range(7)] + [(-1, k) for k in range(7, 13)] + [(k, k + 6) for k in range(7, 14)]
    pairs, score = aff.align_pair(chain, seq, "sw", 5, -4, -8, -6)
    assert (pairs, score) == ([(k, k) for k in range(7)], 35)


def shown(seq):
    """a sequence as the rows show it: upper case, letters other than ACGT as A"""
    return "".join(ch if ch in "ACGT" else "A" for ch in seq.upper())


@pytest.mark.parametrize("mode", MODES)
def test_msa_rows_spell_the_inputs_and_coverage_stays_below_the_number_of_sequences(cvx, mode):
    scores = CONVEX_SCORES[0]
    sets = SETS[:160]

    def both(st):
        return cvx.msa(st, mode, scores, include_consensus=True), cvx.weighted(st, None, mode, scores), cvx.consensus(st, mode, scores)

    for k, (msa, wt, cns) in enumerate(all_sets(both, sets)):
        st = sets[k]
        assert msa.consensus == cns == wt.consensus, (mode, k)
        assert len(msa.rows) == len(st) + 1 and all(len(r) == msa.n_cols for r in msa.rows), (mode, k)
        assert [r.replace("-", "") for r in msa.rows] == [shown(q) for q in st] + [cns], (mode, k)
        if msa.n_cols:   # every column holds a base of some sequence
            assert all(any(r[j] != "-" for r in msa.rows[:-1]) for j in range(msa.n_cols)), (mode, k)
        assert len(wt.coverage) == len(cns) == len(wt.profile), (mode, k)
        counted = sum(1 for q in st if len(q) >= 2)
        assert all(0 <= v <= counted for v in wt.coverage), (mode, k)
        assert all(sum(p) == v for p, v in zip(wt.profile, wt.coverage)), (mode, k)
        # the coverage is the number of rows with a base in the consensus base's column, among the sequences of two or more bases
        cols = [j for j in range(msa.n_cols) if msa.rows[-1][j] != "-"]
        assert wt.coverage == [sum(1 for q, r in zip(st, msa.rows) if len(q) >= 2 and r[j] != "-") for j in cols], (mode, k)
