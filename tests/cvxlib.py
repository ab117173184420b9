"""ctypes loader for tests/poa_convex_ref.cpp, the CPU restatement of the POA under two-piece affine (convex) gap penalties in the three
alignment modes. It is compiled with g++ into a directory the caller gives (a pytest temporary directory, or one of
tools/poa_modes_bench.py's own). Scores are always the six (match, mismatch, gap_open, gap_extend, gap_open2, gap_extend2)."""
import ctypes as C
import os
import subprocess
from collections import namedtuple

HERE = os.path.dirname(os.path.abspath(__file__))
TYPES = {"sw": 0, "nw": 1, "ov": 2}
DEFAULT = (5, -4, -8, -6, -10, -4)   # spoa's and minimap2's command-line defaults

Msa = namedtuple("Msa", "n_cols consensus rows")
Weighted = namedtuple("Weighted", "consensus coverage profile")


def gap_score(scores, k):
    """the score of a gap of k >= 1 bases"""
    _, _, g, e, q, c = scores
    return max(g + (k - 1) * e, q + (k - 1) * c)


class ConvexRef:
    def __init__(self, build_dir):
        so = os.path.join(build_dir, "libpoa_convex_ref.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", os.path.join(HERE, "poa_convex_ref.cpp"), "-o", so])
        L = C.CDLL(so)
        sc = C.POINTER(C.c_int32)
        L.pcr_consensus.restype = C.c_void_p
        L.pcr_consensus.argtypes = [C.POINTER(C.c_char_p), C.c_uint32, sc, C.c_int32, C.POINTER(C.c_uint64)]
        L.pcr_last_alignment.restype = C.c_int32
        L.pcr_last_alignment.argtypes = [C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32]
        L.pcr_last_score.restype = C.c_int32
        L.pcr_msa.restype = C.c_void_p
        L.pcr_msa.argtypes = [C.POINTER(C.c_char_p), C.c_uint32, sc, C.c_int32, C.c_int32]
        L.pcr_weighted.restype = C.c_void_p
        L.pcr_weighted.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.c_uint32, sc, C.c_int32]
        L.pcr_free.argtypes = [C.c_void_p]
        self._L = L

    @staticmethod
    def _args(seqs, scores):
        assert len(scores) == 6
        return (C.c_char_p * max(1, len(seqs)))(*[s.encode() for s in seqs]), len(seqs), (C.c_int32 * 6)(*scores)

    def _take(self, p):
        s = C.string_at(p).decode()
        self._L.pcr_free(p)
        return s

    def consensus_cells(self, seqs, type="nw", scores=DEFAULT):
        """(consensus, sum of V * L over the alignments)"""
        cells = C.c_uint64(0)
        return self._take(self._L.pcr_consensus(*self._args(seqs, scores), TYPES[type], C.byref(cells))), cells.value

    def consensus(self, seqs, type="nw", scores=DEFAULT):
        return self.consensus_cells(seqs, type, scores)[0]

    def last_alignment(self):
        """the (node | -1, position | -1) pairs of the last alignment the calling thread made"""
        n = self._L.pcr_last_alignment(None, None, 0)
        a, b = (C.c_int32 * max(1, n))(), (C.c_int32 * max(1, n))()
        self._L.pcr_last_alignment(a, b, n)
        return [(a[k], b[k]) for k in range(n)]

    def last_score(self):
        """H of the end cell of the last alignment the calling thread made (0 when there was none)"""
        return self._L.pcr_last_score()

    def align_pair(self, a, b, type, scores=DEFAULT):
        """b against the chain of a: (alignment pairs, end score)"""
        self.consensus([a, b], type, scores)
        return self.last_alignment(), self.last_score()

    def msa(self, seqs, type="nw", scores=DEFAULT, include_consensus=False):
        lines = self._take(self._L.pcr_msa(*self._args(seqs, scores), TYPES[type], int(bool(include_consensus)))).split("\n")[:-1]
        return Msa(int(lines[0]), lines[1], lines[2:])

    def weighted(self, seqs, weights=None, type="nw", scores=DEFAULT):
        """weights: one list of integers 1..255 per sequence, or None (all 1)"""
        arr, n, sc = self._args(seqs, scores)
        warr = None
        if weights is not None:
            assert len(weights) == len(seqs) and all(len(w) == len(s) and all(1 <= v <= 255 for v in w) for w, s in zip(weights, seqs))
            warr = (C.c_char_p * max(1, len(seqs)))(*[bytes(w) + b"\0" for w in weights])
        lines = self._take(self._L.pcr_weighted(arr, warr, n, sc, TYPES[type])).split("\n")[:-1]
        prof = [int(v) for v in lines[2].split()]
        return Weighted(lines[0], [int(v) for v in lines[1].split()], [prof[i:i + 4] for i in range(0, len(prof), 4)])
