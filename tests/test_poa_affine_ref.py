"""The CPU restatement of the affine-gap POA (tests/poa_affine_ref.cpp, DESIGN.md "General POA path", "Affine gaps"): with
gap_extend == gap_open it is the linear restatement pair for pair (and under kNW the oracle), its end scores are those of a plain
three-matrix pairwise Gotoh written here, the seeded sets reach alignments that only an affine gap gives, and two hand-derived cases
pin the walk."""
import random
from concurrent.futures import ThreadPoolExecutor

import pytest

import orclib
import parlib
import pmrlib
from test_poa_modes_ref import SETS, TRIPLES

MODES = ["sw", "nw", "ov"]
NEG = -10**9


@pytest.fixture(scope="module")
def aff(built, tmp_path_factory):
    return parlib.AffineRef(str(tmp_path_factory.mktemp("par")))


@pytest.fixture(scope="module")
def lin(built, tmp_path_factory):
    return pmrlib.ModesRef(str(tmp_path_factory.mktemp("par_pmr")))


def block_noisy(rnd, t, err=0.06, run=0.04):
    """copy of t with substitutions and single-base indels at rate err, and indel runs of 2-9 bases starting at rate run"""
    out, k = [], 0
    while k < len(t):
        r = rnd.random()
        if r < run / 2:
            k += rnd.randrange(2, 10)                                                  # a block is deleted
            continue
        if r < run:
            out.append("".join(rnd.choice("ACGT") for _ in range(rnd.randrange(2, 10))))   # a block is inserted
        elif r < run + err / 3:
            k += 1
            continue
        elif r < run + 2 * err / 3:
            out.append(rnd.choice("ACGT"))
            k += 1
            continue
        elif r < run + err:
            out.append(rnd.choice("ACGT"))
        out.append(t[k])
        k += 1
    return "".join(out)


def seeded_pairs(seed, n, lo, hi):
    rnd = random.Random(seed)
    out = []
    for _ in range(n):
        a = "".join(rnd.choice("ACGT") for _ in range(rnd.randrange(lo, hi)))
        b = block_noisy(rnd, a)
        if rnd.random() < 0.3:   # overhangs, so that the local and overlap ends are not the corners
            a = "".join(rnd.choice("ACGT") for _ in range(rnd.randrange(0, 8))) + a
            b = b + "".join(rnd.choice("ACGT") for _ in range(rnd.randrange(0, 8)))
        out.append((a, b or "A"))
    return out


PAIRS = seeded_pairs(97, 300, 4, 40)
AFFINE_SCORES = [(5, -4, -8, -2), (5, -4, -8, -6), (3, -5, -4, 0), (1, -1, -3, -2), (2, -7, -5, -1), (5, -4, -8, -8)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("triple", TRIPLES)
def test_equal_scores_are_the_linear_restatement(aff, lin, mode, triple):
    m, x, g = triple

    def both(st):
        a = aff.consensus_cells(st, mode, m, x, g, g)
        pa = aff.last_alignment()
        b = lin.consensus_cells(st, mode, m, x, g)
        return a, pa, b, lin.last_alignment()

    with ThreadPoolExecutor(16) as ex:   # (both restatements release the GIL and keep the last alignment per thread)
        res = list(ex.map(both, SETS))
    for k, (a, pa, b, pb) in enumerate(res):
        assert a == b, (mode, triple, k)
        assert pa == pb, (mode, triple, k)
    if mode == "nw":
        for k, st in enumerate(SETS):
            assert res[k][0][0] == orclib.poa_consensus(st, m, x, g), (triple, k)


def gotoh(a, b, mode, m, x, g, e):
    """end score of b against a by the textbook three-matrix recurrences: M ends in a pair, X in a base of a against a gap, Y in a base
    of b against a gap; global, local (0 when nothing is above 0) and overlap (free ends on both sequences) ends"""
    n, L = len(a), len(b)
    M = [[NEG] * (L + 1) for _ in range(n + 1)]
    X = [[NEG] * (L + 1) for _ in range(n + 1)]
    Y = [[NEG] * (L + 1) for _ in range(n + 1)]
    M[0][0] = 0
    free = mode != "nw"
    for i in range(1, n + 1):
        if free:
            M[i][0] = 0
        else:
            X[i][0] = g + (i - 1) * e
    for j in range(1, L + 1):
        if free:
            M[0][j] = 0
        else:
            Y[0][j] = g + (j - 1) * e
    best = 0 if mode == "sw" else NEG
    for i in range(1, n + 1):
        for j in range(1, L + 1):
            prev = max(M[i - 1][j - 1], X[i - 1][j - 1], Y[i - 1][j - 1])
            M[i][j] = prev + (m if a[i - 1] == b[j - 1] else x)
            X[i][j] = max(max(M[i - 1][j], Y[i - 1][j]) + g, X[i - 1][j] + e)
            Y[i][j] = max(max(M[i][j - 1], X[i][j - 1]) + g, Y[i][j - 1] + e)
            if mode == "sw":
                M[i][j] = max(M[i][j], 0)
            h = max(M[i][j], X[i][j], Y[i][j])
            if mode == "sw" or (mode == "ov" and (i == n or j == L)):
                best = max(best, h)
    if mode == "nw":
        best = max(M[n][L], X[n][L], Y[n][L])
    return best


@pytest.mark.parametrize("mode", MODES)
def test_end_scores_are_gotoh_on_chains(aff, mode):
    for scores in AFFINE_SCORES:
        for k, (a, b) in enumerate(PAIRS):
            assert aff.align_pair(a, b, mode, *scores)[1] == gotoh(a, b, mode, *scores), (mode, scores, k, a, b)


@pytest.mark.parametrize("mode", MODES)
def test_the_seeded_pairs_reach_affine_only_alignments(aff, mode):
    differ = sum(1 for a, b in PAIRS if aff.align_pair(a, b, mode, 5, -4, -8, -2)[0] != aff.align_pair(a, b, mode, 5, -4, -8, -8)[0])
    print(f"{mode}: {differ} of {len(PAIRS)} pairs align differently under (5, -4, -8, -2) and (5, -4, -8, -8)")
    assert differ > 0


def test_a_deleted_block_is_one_gap(aff):
    """Chain ACGTTGCAGTCA (nodes 0-11), sequence ACGTGTCA (the block TGCA, nodes 4-7, is missing), kNW, (5, -4, -8, -2).
    Eight matches and one gap of four nodes: 40 + (-8 - 2 - 2 - 2) = 26.

        H     -   A   C   G   T   G   T   C   A        F     -   A   C   G   T   G   T   C   A
        -     0  -8 -10 -12 -14 -16 -18 -20 -22        -     .   .   .   .   .   .   .   .   .
        A    -8   5  -3  -5  -7  -9 -11 -13 -15        A    -8 -16 -18 -20 -22 -24 -26 -28 -30
        C   -10  -3  10   2   0  -2  -4  -6  -8        C   -10  -3 -11 -13 -15 -17 -19 -21 -23
        G   -12  -5   2  15   7   5   3   1  -1        G   -12  -5   2  -6  -8 -10 -12 -14 -16
        T   -14  -7   0   7  20  12  10   8   6        T   -14  -7   0   7  -1  -3  -5  -7  -9
        T   -16  -9  -2   5  12  16  17   9   7        T   -16  -9  -2   5  12   4   2   0  -2
        G   -18 -11  -4   3  10  17  12  13   5        G   -18 -11  -4   3  10   8   9   1  -1
        C   -20 -13  -6   1   8   9  13  17   9        C   -20 -13  -6   1   8   9   7   5  -3
        A   -22 -15  -8  -1   6   7   5   9  22        A   -22 -15  -8  -1   6   7   5   9   1
        G   -24 -17 -10  -3   4  11   3   7  14        G   -24 -17 -10  -3   4   5   3   7  14
        T   -26 -19 -12  -5   2   3  16   8  12        T   -26 -19 -12  -5   2   3   1   5  12
        C   -28 -21 -14  -7   0   1   8  21  13        C   -28 -21 -14  -7   0   1   8   3  10
        A   -30 -23 -16  -9  -2  -1   6  13  26        A   -30 -23 -16  -9  -2  -1   6  13   8

    The walk starts in state H at (12, 8) and takes the diagonal through 26, 21, 16, 11 to (8, 4). There H = 6 has no diagonal
    (A against T: H[7][3] - 4 = -3) and equals F[8][4], so the state is F. F[8][4] = 6 is not H[7][4] + g = 0 but F[7][4] + e = 8 - 2:
    the state stays F; so do rows 7 and 6 (F = 8 = 10 - 2, F = 10 = 12 - 2). F[5][4] = 12 = H[4][4] + g = 20 - 8 opens the gap: the
    state is H at (4, 4), and the diagonal runs to (0, 0). E is never entered."""
    pairs, score = aff.align_pair("ACGTTGCAGTCA", "ACGTGTCA", "nw", 5, -4, -8, -2)
    assert score == 26
    assert pairs == [(0, 0), (1, 1), (2, 2), (3, 3), (4, -1), (5, -1), (6, -1), (7, -1), (8, 4), (9, 5), (10, 6), (11, 7)]


def test_one_gap_of_two_where_the_linear_walk_takes_two_of_one(aff, lin):
    """Chain GGAGT (nodes 0-4), sequence GGT, kNW. With (5, -4, -8, -2):

        H     -   G   G   T        F     -   G   G   T        E     -   G   G   T
        -     0  -8 -10 -12        -     .   .   .   .        -     .  -8 -10 -12
        G    -8   5  -3  -5        G    -8 -16 -18 -20        G     . -16  -3  -5
        G   -10  -3  10   2        G   -10  -3 -11 -13        G     . -18 -11   2
        A   -12  -5   2   6        A   -12  -5   2  -6        A     . -20 -13  -6
        G   -14  -7   0  -2        G   -14  -7   0  -2        G     . -22 -15  -8
        T   -16  -9  -2   5        T   -16  -9  -2  -4        T     . -24 -17 -10

    (5, 3) = 5 = H[4][2] + 5, (4, 2) = 0 = H[3][1] + 5, (3, 1) = -5 has no diagonal (-10 - 4) and equals F[3][1]: state F.
    F[3][1] = -5 is not H[2][1] + g = -11 but F[2][1] + e = -3 - 2: node 2 is passed, the state stays F. F[2][1] = -3 = H[1][1] + g = 5 - 8:
    node 1 is passed, the state is H at (1, 1) = 5 = H[0][0] + 5. One gap over nodes 1-2, score 15 - 8 - 2 = 5.
    With the linear (5, -4, -8, -8) H[5][3] = -1 and the walk is (5, 3), (4, 2), (3, 1) by the diagonal, then H[3][1] = -11 = H[2][1] + g
    passes node 2, then H[2][1] = -3 = H[1][0] + 5 pairs node 1 with position 0, and H[1][0] = -8 passes node 0: two gaps of one."""
    pairs, score = aff.align_pair("GGAGT", "GGT", "nw", 5, -4, -8, -2)
    assert (pairs, score) == ([(0, 0), (1, -1), (2, -1), (3, 1), (4, 2)], 5)
    pairs, score = aff.align_pair("GGAGT", "GGT", "nw", 5, -4, -8, -8)
    assert (pairs, score) == ([(0, -1), (1, 0), (2, -1), (3, 1), (4, 2)], -1)
    lin.consensus(["GGAGT", "GGT"], "nw", 5, -4, -8)
    assert lin.last_alignment() == pairs
