"""The CPU restatement of the three POA alignment modes (tests/poa_modes_ref.cpp): under kNW it is the oracle's consensus on a few
hundred seeded sets (which pins the graph, add_alignment, the order and the consensus the modes share with kNW), and known answers show
that kSW and kOV are honoured, including the empty-alignment paths."""
import random

import pytest

import orclib
import pmrlib

TRIPLES = [(5, -4, -8), (3, -5, -4), (1, -1, -1), (2, -7, -1)]


@pytest.fixture(scope="module")
def ref(built, tmp_path_factory):
    return pmrlib.ModesRef(str(tmp_path_factory.mktemp("pmr")))


def noisy(rnd, t, err):
    out = []
    for c in t:
        r = rnd.random()
        if r < err / 3:
            continue                                   # deletion
        if r < 2 * err / 3:
            out.append(rnd.choice("ACGT"))             # substitution
        elif r < err:
            out.append(c + rnd.choice("ACGT"))         # insertion
        else:
            out.append(c)
    return "".join(out)


def random_sets(seed, n):
    """n seeded sets: empty sets and members, single bases, identical copies, noisy copies (5-15 % error, lengths 1-3 000)"""
    rnd = random.Random(seed)
    sets = [[], [""], ["", ""], ["A"], ["C", "G"], ["T", "", "T"], ["ACGTTGCA"] * 4]
    while len(sets) < n:
        k = rnd.random()
        L = rnd.choice([1, 2, 5, 17, 60, 200, 700]) if rnd.random() < 0.9 else rnd.randrange(1000, 3001)
        t = "".join(rnd.choice("ACGT") for _ in range(L))
        if k < 0.1:
            sets.append([t] * rnd.randrange(1, 5))
        else:
            st = [noisy(rnd, t, rnd.uniform(0.05, 0.15)) for _ in range(rnd.randrange(1, 7 if L < 1000 else 4))]
            if rnd.random() < 0.2:
                st.insert(rnd.randrange(len(st) + 1), "")
            sets.append(st)
    return sets


SETS = random_sets(41, 320)


@pytest.mark.parametrize("triple", TRIPLES)
def test_nw_is_the_oracle(ref, triple):
    m, x, g = triple
    sets = SETS if triple == (5, -4, -8) else SETS[:120]
    for k, st in enumerate(sets):
        assert ref.consensus(st, "nw", m, x, g) == orclib.poa_consensus(st, m, x, g), (k, triple)


@pytest.mark.parametrize("mode", ["sw", "nw", "ov"])
def test_one_sequence_and_copies_give_the_sequence(ref, mode):
    rnd = random.Random(5)
    for L in (1, 2, 9, 150, 800):
        s = "".join(rnd.choice("ACGT") for _ in range(L))
        assert ref.consensus([s], mode) == s
        assert ref.consensus([s] * 5, mode) == s


def test_ov_joins_overlapping_fragments_and_nw_does_not(ref):
    rnd = random.Random(6)
    t = "".join(rnd.choice("ACGT") for _ in range(1200))
    frags = [t[0:500], t[350:850], t[700:1200]]   # error-free, 150-base overlaps, tiling the template
    assert ref.consensus(frags, "ov") == t
    assert ref.consensus(frags, "nw") != t


def test_sw_without_a_positive_cell_takes_the_empty_alignment(ref):
    # "C" against the graph "A" with (5, -4, -8): every cell is clamped to 0, so the alignment is empty and "C" becomes a chain of its own
    assert ref.consensus(["A", "C"], "sw") == "A"
    assert ref.last_alignment() == []
    # with a match the alignment is the match alone
    ref.consensus(["A", "A"], "sw")
    assert ref.last_alignment() == [(0, 0)]


def test_sw_keeps_the_local_match_and_adds_the_flanks_as_chains(ref):
    rnd = random.Random(7)
    core = "".join(rnd.choice("ACGT") for _ in range(200))
    a = "".join(rnd.choice("ACGT") for _ in range(40)) + core
    b = core + "".join(rnd.choice("ACGT") for _ in range(40))
    ref.consensus([a, b], "sw")
    aln = ref.last_alignment()
    # the matched part of b is its core: positions 0..199 on the nodes of a's core (40..239), nothing else
    assert aln == [(40 + k, k) for k in range(200)]
    assert ref.consensus([a, b, b], "sw") == a + b[200:]   # (the heaviest path runs through every chain: a flank is the only way in or out)


def test_ov_alignment_without_a_sequence_position_is_empty(ref):
    # graph "A", sequence "C", n = -20, g = -1: H[1][1] = max(-20, H[0][1] + g = -1, H[1][0] + g = -1) = -1 is the best end cell (a sink,
    # j >= 1), and its traceback is one vertical move to (0, 1) - the pair (node 0, -1). No sequence position is aligned: the alignment counts
    # as empty, "C" becomes a chain of its own, and the consensus is the first chain (node 0, "A", the heavier start in rank order).
    assert ref.consensus(["A", "C"], "ov", 5, -20, -1) == "A"
    assert ref.last_alignment() == [(0, -1)]


def test_cells_are_the_full_matrices(ref):
    # identical copies add no node: V = 4 for the second and the third, the empty member is skipped
    for mode in ("sw", "nw", "ov"):
        assert ref.consensus_cells(["ACGT", "ACGT", "", "ACGT"], mode) == ("ACGT", 4 * 4 + 4 * 4)
