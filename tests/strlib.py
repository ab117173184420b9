"""ctypes loader for tests/poa_strand_ref.cpp, the CPU restatement of strand-ambiguous sets on the general POA path. It is compiled with g++
into a directory the caller gives (a pytest temporary directory, or one of tools/poa_modes_bench.py's own). Scores are always the six
(match, mismatch, gap_open, gap_extend, gap_open2, gap_extend2); the gap model follows from them by the C-ABI's rule (grflib.model_of). A
result is a haslr_amd.hip.StrandRecord with every field filled, the type HipContext.poa_strand returns, so that both sides compare field
by field."""
import ctypes as C
import os
import random
import subprocess

from grflib import LINEAR, AFFINE, CONVEX, TYPES, kw_of, model_of, read   # noqa: F401 (the score sets and rules are the graph restatement's)
from haslr_amd.hip import StrandRecord

HERE = os.path.dirname(os.path.abspath(__file__))
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def rc(s):
    """the reverse complement as the path reads it: a letter that is not ACGT is A, and its complement is T"""
    return "".join(COMP[read(c)] for c in reversed(s))


def oriented(seqs, flags):
    """the set with its flagged sequences reverse-complemented"""
    return [rc(s) if f else s for s, f in zip(seqs, flags)]


def oriented_weights(weights, flags):
    return [list(reversed(w)) if f else list(w) for w, f in zip(weights, flags)]


class StrandRef:
    def __init__(self, build_dir):
        so = os.path.join(build_dir, "libpoa_strand_ref.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", os.path.join(HERE, "poa_strand_ref.cpp"), "-o", so])
        L = C.CDLL(so)
        L.psr_strand.restype = C.c_void_p
        L.psr_strand.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32]
        L.psr_free.argtypes = [C.c_void_p]
        self._L = L

    def strand_cells(self, seqs, type="nw", scores=LINEAR, weights=None, include_consensus=False):
        """(StrandRecord, cells of both orientations over the alignments, sequences whose reverse complement won)"""
        assert len(scores) == 6
        arr = (C.c_char_p * max(1, len(seqs)))(*[s.encode() for s in seqs])
        warr = None
        if weights is not None:
            assert len(weights) == len(seqs) and all(len(w) == len(s) and all(1 <= v <= 255 for v in w) for w, s in zip(weights, seqs))
            warr = (C.c_char_p * max(1, len(seqs)))(*[bytes(w) + b"\0" for w in weights])
        p = self._L.psr_strand(arr, warr, len(seqs), (C.c_int32 * 6)(*scores), model_of(scores), TYPES[type], int(bool(include_consensus)))
        ln = C.string_at(p).decode().split("\n")[:-1]
        self._L.psr_free(p)
        flags, sf, sr = ([int(v) for v in ln[k].split()] for k in (1, 2, 3))
        cells, third, n_cols = (int(v) for v in ln[4].split())
        prof = [int(v) for v in ln[6].split()]
        rows = ln[7:]
        assert len(rows) == len(seqs) + int(bool(include_consensus)) and all(len(r) == n_cols for r in rows)
        rec = StrandRecord(ln[0], [bool(f) for f in flags], list(zip(sf, sr)), rows, [int(v) for v in ln[5].split()],
                           [prof[i:i + 4] for i in range(0, len(prof), 4)])
        return rec, cells, third

    def strand(self, seqs, type="nw", scores=LINEAR, weights=None, include_consensus=False):
        return self.strand_cells(seqs, type, scores, weights, include_consensus)[0]


# ---- the sets the CPU and the GPU tests share
def noisy(rnd, t, err, letters="ACGT"):
    """a copy of t with about err errors: a third deletions, a third substitutions, a third insertions"""
    out = []
    for c in t:
        r = rnd.random()
        if r < err / 3:
            continue
        if r < 2 * err / 3:
            out.append(rnd.choice(letters))
        elif r < err:
            out.append(c + rnd.choice(letters))
        else:
            out.append(c)
    return "".join(out)


def substituted(rnd, t, err):
    """a copy of t of the same length with about err substitutions"""
    return "".join(rnd.choice("ACGT") if rnd.random() < err else c for c in t)


def mixed_set(rnd, length, n, exact=False):
    """n copies of a random template of `length` bases at 5-15 % errors, every one after the first reverse-complemented with probability
    1/2; the first is the template itself and the second a reverse-complemented copy of exactly that length, so that reversed indexing
    meets the length as it is; exact: substitutions only, so that `length` is the set's longest sequence and decides its kernel
    instance. Returns (the set, the orientation each member was given in)"""
    t = "".join(rnd.choice("ACGT") for _ in range(length))
    st, given = [t], [0]
    for k in range(1, n):
        q = substituted(rnd, t, rnd.uniform(0.05, 0.15)) if k == 1 or exact else noisy(rnd, t, rnd.uniform(0.05, 0.15)) or "A"
        f = 1 if k == 1 else int(rnd.random() < 0.5)
        st.append(rc(q) if f else q)
        given.append(f)
    return st, given


# the lane and instance edges of reversed indexing: one base, a lane's 16 columns +- 1, and the last length of the 64 x 16 instance (1023) with its neighbours
EDGE_LENGTHS = [1, 15, 16, 17, 1022, 1023, 1024]


def edge_sets(seed):
    rnd = random.Random(seed)
    return [mixed_set(rnd, L, rnd.randrange(3, 9), exact)[0] for L in EDGE_LENGTHS for exact in (False, True)]


def long_set(seed, length):
    return mixed_set(random.Random(seed), length, 3)[0]


def tie_sets(seed, n=60):
    """short sequences over two letters that are each other's complement: an orientation and its reverse often score alike"""
    rnd = random.Random(seed)
    return [["".join(rnd.choice(ab) for _ in range(rnd.randrange(4, 11))) for _ in range(rnd.randrange(3, 7))] for ab in (rnd.choice(["AT", "AT", "CG"]) for _ in range(n))]


# hand-derived cases (tests/test_poa_strand_ref.py states the answers)
S1 = "ACGTTGCAAGGCTATTC"
PALINDROME = "ACGCGT"
# the weighted case: V is A with a substitution at 4 and one at 15; the second sequence is rc(V), heavy (60) on ITS first half, which is V's second half
WA = "ACGTTGCAAGGCTATTCAGG"
WV = WA[:4] + "A" + WA[5:15] + "G" + WA[16:]
W_WEIGHTS = [[3] * 20, [60] * 10 + [1] * 10]
# the four-member case: s, rc(s'), s'', rc(s''') with one substitution each in s', s'' and s'''
F0 = "ACGTTGCAAGGCTATTCAGGTCCATGA"
FOUR = [F0, rc(F0[:6] + "A" + F0[7:]), F0[:13] + "G" + F0[14:], rc(F0[:20] + "A" + F0[21:])]
