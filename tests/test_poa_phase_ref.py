"""The CPU restatement of two-haplotype consensus with read phasing (tests/poa_phase_ref.cpp) against what is known without it: answers
derived by hand from the rules of DESIGN.md "Two-haplotype consensus" on small sets; the truth of seeded noise-free two-haplotype sets;
and, with noise, the one thing that holds by construction: the output is the label restatement's (tests/poa_label_ref.cpp) for two labels
given the haplotypes the phasing returned.

Why the rounds cannot oscillate. Write z[k] = +1 / -1 / 0 for a read of haplotype 0 / 1 / none, v[k][c] = +1 / -1 / 0 for a read whose
allele at site c is a1 / a2 / anything else or none, and E(z, s) = sum over k, c of z[k] v[k][c] s[c]. The site half of a round sets
s[c] = sign(D[c]) with D[c] = sum over k of z[k] v[k][c], which gives E its maximum over s for this z: sum over c of |D[c]|. The read half
changes z[k] only where S[k] = sum over c of s[c] v[k][c] is not 0 and has another sign than z[k]; read k's share of E, z[k] S[k], then
rises from at most 0 to |S[k]| > 0. So a round that changes a read raises the integer E, which never exceeds the number of (read, site)
pairs, and no assignment comes back: the rounds end by themselves, and PHASE_ROUNDS only cuts a long climb short."""
import random

import pytest

import lbllib
import phaselib
import wgtlib
from phaselib import HAND

MODES = ["sw", "nw", "ov"]
MODEL_NAMES = ["linear", "affine", "convex"]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return phaselib.PhaseRef(str(tmp_path_factory.mktemp("phase_ref")))


@pytest.fixture(scope="module")
def labelled(tmp_path_factory):
    return lbllib.LabelRef(str(tmp_path_factory.mktemp("phase_lbl")))


@pytest.fixture(scope="module")
def weighted(tmp_path_factory):
    return wgtlib.WeightedRef(str(tmp_path_factory.mktemp("phase_wgt")))


def hand(ref, name, model="linear", **kw):
    seqs, mode, mc, mp = HAND[name]
    return ref.phased(seqs, mode, phaselib.MODELS[model], min_count=mc, min_pct=mp, include_consensus=True, **kw)


@pytest.mark.parametrize("model", MODEL_NAMES)
def test_one_snp_splits_three_and_three(ref, model):
    r = hand(ref, "snp", model)
    # column 2 holds G x 3 and T x 3: a1 = G (the smaller code among equals), a2 = T, 3 >= max(2, ceil(25 x 6 / 100) = 2)
    assert r.sites == [(2, 2, 3, 1)] and r.hap == [0, 0, 0, 1, 1, 1] and (r.n_haps, r.rounds) == (2, 1)
    assert r.consensus == ["AAGAA", "AATAA"] and r.columns == [[0, 1, 2, 3, 4]] * 2 and r.coverage == [[3] * 5] * 2
    assert r.profile[0][2] == [0, 0, 3, 0] and r.profile[1][2] == [0, 0, 0, 3]
    assert r.rows == phaselib.SNP + ["AAGAA", "AATAA"]


def test_the_first_read_names_haplotype_0(ref):
    r = hand(ref, "snp_swapped")
    # a1 is still G: the T reads, listed first, are the seed's haplotype 1 and are renamed to 0, and the phase is negated with them
    assert r.sites == [(2, 2, 3, -1)] and r.hap == [0, 0, 0, 1, 1, 1] and (r.n_haps, r.rounds) == (2, 1)
    assert r.consensus == ["AATAA", "AAGAA"] and r.rows[-2:] == ["AATAA", "AAGAA"]


def test_a_deletion_is_an_allele(ref):
    r = hand(ref, "deletion")
    assert r.sites == [(3, 2, 4, 1)] and r.hap == [0, 0, 0, 1, 1, 1] and r.n_haps == 2
    assert r.consensus == ["AACGTT", "AACTT"] and r.columns == [[0, 1, 2, 3, 4, 5], [0, 1, 2, 4, 5]]


def test_sites_in_the_first_and_the_last_column(ref):
    r = hand(ref, "ends")
    # column 0: C x 3 (haplotype 0), T x 3: a1 = C; column 5: G x 3 (haplotype 0), C x 3: a1 = C, which haplotype 1 carries
    assert r.sites == [(0, 1, 3, 1), (5, 1, 2, -1)] and r.hap == [0, 0, 0, 1, 1, 1] and r.rounds == 1
    assert r.consensus == ["CAAAAG", "TAAAAC"]


def test_a_third_allele_votes_nothing(ref):
    r = hand(ref, "three_alleles")
    assert r.sites == [(2, 2, 3, 1)] and r.hap == [0, 0, 0, 1, 1, 1, 255] and r.n_haps == 2
    assert r.consensus == ["AAGAA", "AATAA"] and r.coverage == [[3] * 5] * 2   # (the C read is counted in neither haplotype)


@pytest.mark.parametrize("name", ["short_of_count", "short_of_pct"])
def test_one_short_of_a_threshold_is_unphased(ref, weighted, name):
    r = hand(ref, name)
    seqs = HAND[name][0]
    assert r.sites == [] and r.hap == [0] * len(seqs) and (r.n_haps, r.rounds) == (1, 0) and r.consensus == ["AAGAA", ""]
    want = weighted.weighted(seqs, None, "nw", *phaselib.LINEAR[:4])
    assert (r.consensus[0], r.columns[0], r.coverage[0], r.profile[0]) == (want.consensus, want.cols, want.coverage, want.profile)
    assert (r.columns[1], r.coverage[1], r.profile[1]) == ([], [], []) and r.rows[-1] == "-----"
    # one more minor read, and both thresholds are met
    more = ref.phased(seqs + ["AATAA"], "nw", min_count=HAND[name][2], min_pct=HAND[name][3])
    assert more.sites == [(2, 2, 3, 1)] and more.n_haps == 2


def test_equal_minor_counts_seed_the_smaller_column(ref):
    r = hand(ref, "equal_minors")
    assert r.sites == [(2, 2, 3, 1), (7, 1, 2, 1)] and r.hap == [0, 0, 0, 1, 1, 1] and r.rounds == 1
    # (the seed itself does not show in the output of a clean set; the next test's does)


def test_fragments_off_the_seed_are_assigned_by_their_own_site(ref):
    r = hand(ref, "fragments")
    # column 5: C x 5, G x 5 -> a1 = C, minor count 5; column 24: C x 5, G x 4 -> minor count 4: the seed is column 5. Read 10 spans column
    # 24 only: none after the seed, haplotype 0 after round 1 (which therefore changed something: a second round confirms). Read 11: no site
    assert r.sites == [(5, 1, 2, 1), (24, 1, 2, 1)] and r.hap == [0, 1] * 4 + [0, 1, 0, 255] and (r.n_haps, r.rounds) == (2, 2)
    assert r.consensus == [phaselib.F0, phaselib.F1]
    # haplotype 0: four whole reads, the prefix up to column 11, the suffix from 16; the middle piece (columns 9..20) counts nowhere
    assert r.coverage[0][0] == 5 and r.coverage[0][29] == 5 and r.coverage[0][14] == 4 and r.coverage[1][0] == 5 and r.coverage[1][29] == 4


def test_round_1_moves_a_read_off_its_seed_side(ref):
    r = hand(ref, "moves")
    # column 3: C x 7 (haplotype 1's reads, read 6, two prefixes), A x 5 -> the seed, a1 = C: read 6 starts with haplotype 1. Its five
    # other sites carry haplotype 0's bases: S = 1 - 5 < 0 on the seed's names, and it changes sides
    assert [s[0] for s in r.sites] == [3, 11, 14, 18, 22, 26] and r.sites[0] == (3, 1, 0, -1)
    assert r.hap == [0, 1, 0, 1, 0, 1, 0, 1, 0, 0, 1, 1] and (r.n_haps, r.rounds) == (2, 2)
    assert r.consensus == [phaselib.M0, phaselib.M1]


def test_a_haplotype_that_loses_its_members_leaves_the_set_unphased(ref, weighted):
    r = hand(ref, "loses")
    assert r.sites == [(2, 2, 3, 0), (5, 2, 3, 0), (8, 2, 3, 0)] and r.hap == [0] * 10 and (r.n_haps, r.rounds) == (1, 2)
    want = weighted.weighted(phaselib.LOSES, None, "nw", *phaselib.LINEAR[:4])
    assert r.consensus == [want.consensus, ""] and r.coverage[0] == want.coverage and r.profile[0] == want.profile


def test_empty_and_one_base_sequences(ref):
    r = hand(ref, "empty_and_one_base")
    assert r.hap == [0, 255, 1, 255, 0, 1, 255] and r.sites == [(2, 2, 3, 1)] and r.n_haps == 2   # (the lone A spans column 4 only)
    assert r.rows[1] == r.rows[6] == "-----" and r.rows[3] == "----A"
    for seqs in ([], [""], ["", ""], ["A"], ["A", "C", "A"]):   # (A x 2, C x 1: one short of min_count)
        q = ref.phased(seqs, "nw")
        assert q.n_haps == 1 and q.rounds == 0 and q.sites == [] and q.hap == [0 if s else 255 for s in seqs] and q.consensus[1] == ""
    # four reads of one base: one column, A x 2 and C x 2, a site even at 50 %; the seed splits them and both haplotypes have two members
    q = ref.phased(["A", "C", "A", "C"], "nw", min_pct=50)
    assert q.sites == [(0, 0, 1, 1)] and q.hap == [0, 1, 0, 1] and q.consensus == ["A", "C"] and (q.n_haps, q.rounds) == (2, 1)


def test_the_rounds_end_by_themselves(ref):
    # (the module's docstring has the proof; this holds the restatement to it on sets with up to six conflicting sites)
    rnd = random.Random(5)
    most = 0
    for _ in range(400):
        n_sites, n_reads = rnd.randrange(3, 7), rnd.randrange(4, 10)
        seqs = ["".join("AA" + rnd.choice("GT") for _ in range(n_sites)) + "AA" for _ in range(n_reads)]
        r = ref.phased(seqs, "nw", min_count=rnd.choice([1, 2]), min_pct=rnd.choice([1, 20, 25]))
        assert r.rounds <= 8 and (r.rounds > 0) == bool(r.sites)
        most = max(most, r.rounds)
    assert most >= 3


@pytest.mark.parametrize("model", MODEL_NAMES)
@pytest.mark.parametrize("mode", MODES)
def test_noise_free_haplotypes_are_recovered(ref, mode, model):
    for seed in range(6):
        rnd = random.Random(900 + seed)
        order = [0, 1] * 3 + [rnd.randrange(2) for _ in range(4)]
        if seed % 2:
            order = [1 - g for g in order]   # (the truth's haplotype 1 comes first: the renaming)
        seqs, truth, haps = phaselib.snp_set(500 + seed, 60 + 7 * seed, 0, snps=1 + seed % 4, order=order)
        r = ref.phased(seqs, mode, phaselib.MODELS[model])
        want = [g ^ truth[0] for g in truth]
        assert r.hap == want and r.n_haps == 2 and r.rounds == 1 and len(r.sites) == 1 + seed % 4
        assert r.consensus == [haps[truth[0]], haps[1 - truth[0]]]
        assert all(ph in (1, -1) and {"ACGT"[a1], "ACGT"[a2]} == {haps[0][c], haps[1][c]} for c, a1, a2, ph in r.sites)


@pytest.mark.parametrize("model", MODEL_NAMES)
@pytest.mark.parametrize("mode", MODES)
def test_with_noise_the_output_is_the_label_restatements(ref, labelled, mode, model):
    sc = phaselib.MODELS[model]
    for seed in range(5):
        seqs, _ = lbllib.two_haplotypes(700 + seed, 50 + 11 * seed, 3 + seed % 3, 0.04 + 0.02 * seed)
        seqs += ["", seqs[0][:1]]
        wts = None if seed % 2 else phaselib.hand_weights(seqs)
        r, cells, n_cols = ref.phased_cells(seqs, mode, sc, weights=wts, include_consensus=True)
        w, wcells, wcols = labelled.labelled_cells(seqs, r.hap, 2, mode, sc, weights=wts, include_consensus=True)
        assert (r.consensus, r.columns, r.coverage, r.profile, r.rows, cells, n_cols) == (w.consensus, w.columns, w.coverage, w.profile, w.rows, wcells, wcols)
        assert r.hap[-2] == 255 and set(r.hap) <= {0, 1, 255} and r.n_haps == (2 if 1 in r.hap else 1)
        assert [c for c, _, _, _ in r.sites] == sorted({c for c, _, _, _ in r.sites}) and all(0 <= a1 <= 4 and 0 <= a2 <= 4 and a1 != a2 for _, a1, a2, _ in r.sites)
