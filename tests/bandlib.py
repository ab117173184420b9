"""ctypes loader for tests/poa_band_ref.cpp, the CPU restatement of adaptive banded alignment on the general POA path, and the sets that
the CPU and the GPU tests share. The restatement is compiled with g++ into a directory the caller gives (a pytest temporary directory, or
one of tools/poa_modes_bench.py's own). Scores are always the six (match, mismatch, gap_open, gap_extend, gap_open2, gap_extend2); the gap
model follows from them by the C-ABI's rule (grflib.model_of). A result is a haslr_amd.hip.BandRecord with every field filled, the type
HipContext.poa_banded returns, so that both sides compare field by field."""
import ctypes as C
import os
import random
import subprocess

from grflib import LINEAR, AFFINE, CONVEX, TYPES, kw_of, model_of   # noqa: F401 (the score sets and rules are the graph restatement's)
from haslr_amd.hip import BandRecord
from strlib import noisy, substituted   # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
MODELS = {"linear": LINEAR, "affine": AFFINE, "convex": CONVEX}
MAX_HALF = 511


class BandRef:
    def __init__(self, build_dir):
        so = os.path.join(build_dir, "libpoa_band_ref.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", os.path.join(HERE, "poa_band_ref.cpp"), "-o", so])
        L = C.CDLL(so)
        L.pbr_banded.restype = C.c_void_p
        L.pbr_banded.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_uint32, C.c_int32, C.c_int32]
        L.pbr_free.argtypes = [C.c_void_p]
        self._L = L

    def banded_cells(self, seqs, band, type="nw", scores=LINEAR, weights=None, include_consensus=False, force_window=False):
        """(BandRecord, dp_cells of the final attempt, band reruns of the set). force_window keeps the windowed DP where the rules send the
        set to the full matrix because its longest sequence + 1 fits the window."""
        assert len(scores) == 6
        arr = (C.c_char_p * max(1, len(seqs)))(*[s.encode() for s in seqs])
        warr = None
        if weights is not None:
            assert len(weights) == len(seqs) and all(len(w) == len(s) and all(1 <= v <= 255 for v in w) for w, s in zip(weights, seqs))
            warr = (C.c_char_p * max(1, len(seqs)))(*[bytes(w) + b"\0" for w in weights])
        p = self._L.pbr_banded(arr, warr, len(seqs), (C.c_int32 * 6)(*scores), model_of(scores), TYPES[type], band, int(bool(force_window)), int(bool(include_consensus)))
        ln = C.string_at(p).decode().split("\n")[:-1]
        self._L.pbr_free(p)
        cells, used, reruns, n_cols = (int(v) for v in ln[1].split())
        prof = [int(v) for v in ln[3].split()]
        rows = ln[4:]
        assert len(rows) == len(seqs) + int(bool(include_consensus)) and all(len(r) == n_cols for r in rows)
        return BandRecord(ln[0], used, rows, [int(v) for v in ln[2].split()], [prof[i:i + 4] for i in range(0, len(prof), 4)]), cells, reruns

    def banded(self, seqs, band, type="nw", scores=LINEAR, weights=None, include_consensus=False, force_window=False):
        return self.banded_cells(seqs, band, type, scores, weights, include_consensus, force_window)[0]


def ladder(w, lmax):
    """the half-widths a set that always misses goes through, 0 the full matrix: w, 2w, ... while the window holds at most 1023 columns and
    the longest sequence + 1 does not fit it"""
    out = []
    while w and lmax + 1 > 2 * w + 1:
        out.append(w)
        w = 2 * w if 2 * w <= MAX_HALF else 0
    return out + [0]


# ---- the sets the CPU and the GPU tests share
def template(rnd, length):
    return "".join(rnd.choice("ACGT") for _ in range(length))


def copies(seed, length, n, err):
    """the template and n - 1 noisy copies of it"""
    rnd = random.Random(seed)
    t = template(rnd, length)
    return [t] + [noisy(rnd, t, err) or "A" for _ in range(n - 1)]


def exact_copies(seed, length, n, err=0.1):
    """the template and n - 1 copies with substitutions only: every member has `length` bases"""
    rnd = random.Random(seed)
    t = template(rnd, length)
    return [t] + [substituted(rnd, t, err) for _ in range(n - 1)]


# the hand-built escalation case: under kNW the copy's 40 extra bases at its front move the path 40 columns off the diagonal at once, which a
# window of 17 columns cannot follow (the end cell, the sink's row at the last column, stays out of reach)
ESC_T = template(random.Random(4001), 200)
ESC_SET = [ESC_T, template(random.Random(4002), 40) + ESC_T]
# two sequences that share nothing and differ in length by more than any window: every rung misses under kNW, the set ends on the full matrix
LAST_RUNG_SET = ["AC" * 100, "GT" * 1200]


# A two-branch graph that a window of 17 columns can build and follow. The first sequence is P + T^150 + S, with P and S of 60 bases over
# A, C and G; the second is P + S: under TWO_BRANCH scores a mismatch costs more than a gap base, so through the 150 rows of T the best cell
# of its rows stays in column 60 and the window with it, and the add leaves the edge from P's last node to S's first, which now has two
# in-edges. The third sequence carries the T's again: its windows follow the matches to column 210, the fan-in row takes its centre from
# the T branch, and its other predecessor, P's last node, kept its window at columns 52..68, wholly disjoint from the row's own.
TWO_BRANCH = {"linear": (5, -9, -8, -8, -8, -8), "affine": (5, -9, -8, -6, -8, -6), "convex": (5, -9, -8, -6, -10, -4)}


def two_branch_set(seed):
    rnd = random.Random(seed)
    p, s = ("".join(rnd.choice("ACG") for _ in range(60)) for _ in range(2))

    def sub(t):
        return "".join(rnd.choice("ACG") if rnd.random() < 0.03 else c for c in t)
    return [p + "T" * 150 + s, p + s, sub(p) + "T" * 150 + sub(s), sub(p) + sub(s), p + "T" * 150 + s]
