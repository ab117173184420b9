"""ctypes loader for tests/poa_phase_ref.cpp, the CPU restatement of two-haplotype consensus with read phasing on the general POA path, and
the sets that the CPU and the GPU tests share. The restatement is compiled with g++ into a directory the caller gives. Scores are always
the six (match, mismatch, gap_open, gap_extend, gap_open2, gap_extend2); the gap model follows from them by the C-ABI's rule
(grflib.model_of). A result is a haslr_amd.hip.PhaseRecord with every field filled, the type HipContext.poa_phased returns, so that both
sides compare field by field."""
import ctypes as C
import os
import random
import subprocess

from grflib import LINEAR, AFFINE, CONVEX, TYPES, kw_of, model_of   # noqa: F401
from haslr_amd.hip import PhaseRecord
from lbllib import MODELS, template   # noqa: F401
from strlib import noisy, substituted   # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
NONE = 255


def _ints(line):
    return [int(v) for v in line.split()]


class PhaseRef:
    def __init__(self, build_dir):
        so = os.path.join(build_dir, "libpoa_phase_ref.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", os.path.join(HERE, "poa_phase_ref.cpp"), "-o", so])
        L = C.CDLL(so)
        L.phr_phased.restype = C.c_void_p
        L.phr_phased.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32]
        L.phr_free.argtypes = [C.c_void_p]
        self._L = L

    def phased_cells(self, seqs, type="nw", scores=LINEAR, weights=None, include_consensus=False, min_count=2, min_pct=25):
        """(PhaseRecord, dp_cells, n_cols)"""
        assert len(scores) == 6 and 1 <= min_count <= 255 and 1 <= min_pct <= 50
        arr = (C.c_char_p * max(1, len(seqs)))(*[s.encode() for s in seqs])
        warr = None
        if weights is not None:
            assert len(weights) == len(seqs) and all(len(w) == len(s) and all(1 <= v <= 255 for v in w) for w, s in zip(weights, seqs))
            warr = (C.c_char_p * max(1, len(seqs)))(*[bytes(w) + b"\0" for w in weights])
        p = self._L.phr_phased(arr, warr, len(seqs), (C.c_int32 * 6)(*scores), model_of(scores), TYPES[type], int(bool(include_consensus)), min_count, min_pct)
        ln = C.string_at(p).decode().split("\n")[:-1]
        self._L.phr_free(p)
        n_haps, rounds, n_sites = _ints(ln[0])
        hap, flat = _ints(ln[1]), _ints(ln[2])
        sites = [tuple(flat[i:i + 4]) for i in range(0, len(flat), 4)]
        assert len(hap) == len(seqs) and len(sites) == n_sites
        cells, n_cols = _ints(ln[3])
        cns, cols, cov, prof = [], [], [], []
        for g in range(2):
            a, b, c, d = ln[4 + 4 * g:8 + 4 * g]
            f4 = _ints(d)
            cns.append(a); cols.append(_ints(b)); cov.append(_ints(c)); prof.append([f4[i:i + 4] for i in range(0, len(f4), 4)])
        rows = ln[12:]
        assert len(rows) == len(seqs) + (2 if include_consensus else 0) and all(len(r) == n_cols for r in rows)
        return PhaseRecord(hap, n_haps, rounds, sites, cns, cols, cov, prof, rows), cells, n_cols

    def phased(self, seqs, type="nw", scores=LINEAR, weights=None, include_consensus=False, min_count=2, min_pct=25):
        return self.phased_cells(seqs, type, scores, weights, include_consensus, min_count, min_pct)[0]


# ---- the sets the CPU and the GPU tests share
def snp_haplotype(rnd, t, snps, lo=5):
    """a copy of t with `snps` substitutions, all at least lo bases away from its ends; (copy, positions)"""
    h = list(t)
    pos = sorted(rnd.sample(range(lo, len(t) - lo), snps))
    for p in pos:
        h[p] = rnd.choice([c for c in "ACGT" if c != h[p]])
    return "".join(h), pos


def snp_set(seed, length, per_hap, snps=3, err=0.0, order=None):
    """(sequences, truth, templates): two haplotypes that differ in `snps` substitutions, per_hap reads of each (copies, or with err > 0
    noisy reads), interleaved from haplotype 0 on unless order (a list of 0 / 1) says otherwise"""
    rnd = random.Random(seed)
    t = template(rnd, length)
    haps = [t, snp_haplotype(rnd, t, snps)[0]]
    truth = order if order is not None else [k % 2 for k in range(2 * per_hap)]
    seqs = [(noisy(rnd, haps[g], err) or "A") if err else haps[g] for g in truth]
    return seqs, list(truth), haps


def many_sites(n_sites, per_hap=3, gap=2):
    """two haplotypes of 1 + n_sites * (gap + 1) bases that differ in n_sites substitutions (A against C, every gap + 1 bases, G's
    between), per_hap exact reads of each, haplotype 0 first: n_sites sites, at columns gap, 2 gap + 1, ..."""
    h0 = "G" + "".join("G" * (gap - 1) + "A" + "G" for _ in range(n_sites))
    h1 = h0.replace("A", "C")
    return [h0] * per_hap + [h1] * per_hap


# hand-built sets (tests/test_poa_phase_ref.py derives the answers); all kNW unless the name says otherwise
SNP = ["AAGAA"] * 3 + ["AATAA"] * 3
SNP_SWAPPED = ["AATAA"] * 3 + ["AAGAA"] * 3
DELETION = ["AACGTT"] * 3 + ["AACTT"] * 3
ENDS = ["CAAAAG"] * 3 + ["TAAAAC"] * 3                              # a site in column 0 and one in the last column
THREE_ALLELES = ["AAGAA"] * 3 + ["AATAA"] * 3 + ["AACAA"]           # the C votes 0 at the site, its read has no other site
SHORT_OF_COUNT = ["AAGAA"] * 5 + ["AATAA"]                           # one T: one short of min_count = 2
SHORT_OF_PCT = ["AAGAA"] * 7 + ["AATAA"] * 2                         # depth 9 at 25 %: ceil(2.25) = 3 needed, 2 there
EQUAL_MINORS = ["AAGAAAACAA"] * 3 + ["AATAAAAGAA"] * 3               # two sites of minor count 3: the seed is column 2
EMPTY_AND_ONE_BASE = ["AAGAA", "", "AATAA", "A", "AAGAA", "AATAA", ""]

def _shifted(t, positions):
    h = list(t)
    for p in positions:
        h[p] = {"A": "C", "C": "G", "G": "T", "T": "A"}[h[p]]
    return "".join(h)


TEMPLATE = "CTGACCATGTTAGCAATCGGTACGCTTAGA"
# kOV. Two haplotypes that differ in columns 5 and 24, four reads of each; a prefix of each makes column 5 the seed (minor count 5 against
# 4); the suffix of haplotype 0 does not span the seed and is assigned by column 24 in round 1; the middle piece spans no site
F0, F1 = TEMPLATE, _shifted(TEMPLATE, [5, 24])
FRAGMENTS = [F0, F1] * 4 + [F0[:12], F1[:12], F0[16:], F0[9:21]]
# kOV. Six sites; the prefixes make column 3 the seed (5 against 4). Read 6 is a haplotype-0 read with haplotype 1's base in the seed
# column: the seed puts it with haplotype 1, its five other sites move it back in round 1
M0, M1 = TEMPLATE, _shifted(TEMPLATE, [3, 11, 14, 18, 22, 26])
MOVES = [M0, M1, M0, M1, M0, M1, _shifted(M0, [3]), M1, M0[:9], M0[:9], M1[:9], M1[:9]]
# min_pct 20. Three sites of minor count 2 whose carriers differ: the seed (column 2) makes reads 4 and 5 haplotype 1, round 1 moves both
# to haplotype 0 by their two other sites, nothing is left in haplotype 1
LOSES = ["AAGAAGAAGAA"] * 4 + ["AATAAGAAGAA"] * 2 + ["AAGAATAAGAA"] * 2 + ["AAGAAGAATAA"] * 2
# name: (sequences, type, min_count, min_pct)
HAND = {"snp": (SNP, "nw", 2, 25), "snp_swapped": (SNP_SWAPPED, "nw", 2, 25), "deletion": (DELETION, "nw", 2, 25), "ends": (ENDS, "nw", 2, 25),
        "three_alleles": (THREE_ALLELES, "nw", 2, 25), "short_of_count": (SHORT_OF_COUNT, "nw", 2, 10), "short_of_pct": (SHORT_OF_PCT, "nw", 2, 25),
        "equal_minors": (EQUAL_MINORS, "nw", 2, 25), "empty_and_one_base": (EMPTY_AND_ONE_BASE, "nw", 2, 25), "fragments": (FRAGMENTS, "ov", 2, 25),
        "moves": (MOVES, "ov", 2, 25), "loses": (LOSES, "nw", 2, 20)}


def hand_weights(seqs, seed=78):
    rnd = random.Random(seed)
    return [[rnd.randrange(1, 41) for _ in q] for q in seqs]
