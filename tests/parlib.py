"""ctypes loader for tests/poa_affine_ref.cpp, the CPU restatement of the affine-gap POA in the three alignment modes. It is compiled
with g++ into a directory the caller gives (a pytest temporary directory, or one of tools/poa_modes_bench.py's own)."""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
TYPES = {"sw": 0, "nw": 1, "ov": 2}


class AffineRef:
    def __init__(self, build_dir):
        so = os.path.join(build_dir, "libpoa_affine_ref.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", os.path.join(HERE, "poa_affine_ref.cpp"), "-o", so])
        L = C.CDLL(so)
        L.par_consensus.restype = C.c_void_p
        L.par_consensus.argtypes = [C.POINTER(C.c_char_p), C.c_uint32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint64)]
        L.par_last_alignment.restype = C.c_int32
        L.par_last_alignment.argtypes = [C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32]
        L.par_last_score.restype = C.c_int32
        L.par_free.argtypes = [C.c_void_p]
        self._L = L

    def consensus_cells(self, seqs, type="nw", match=5, mismatch=-4, gap_open=-8, gap_extend=-6):
        """(consensus, sum of V * L over the alignments)"""
        arr = (C.c_char_p * max(1, len(seqs)))(*[s.encode() for s in seqs])
        cells = C.c_uint64(0)
        p = self._L.par_consensus(arr, len(seqs), match, mismatch, gap_open, gap_extend, TYPES[type], C.byref(cells))
        s = C.string_at(p).decode()
        self._L.par_free(p)
        return s, cells.value

    def consensus(self, seqs, type="nw", match=5, mismatch=-4, gap_open=-8, gap_extend=-6):
        return self.consensus_cells(seqs, type, match, mismatch, gap_open, gap_extend)[0]

    def last_alignment(self):
        """the (node | -1, position | -1) pairs of the last alignment the calling thread made"""
        n = self._L.par_last_alignment(None, None, 0)
        a, b = (C.c_int32 * max(1, n))(), (C.c_int32 * max(1, n))()
        self._L.par_last_alignment(a, b, n)
        return [(a[k], b[k]) for k in range(n)]

    def last_score(self):
        """H of the end cell of the last alignment the calling thread made (0 when there was none)"""
        return self._L.par_last_score()

    def align_pair(self, a, b, type, match, mismatch, gap_open, gap_extend):
        """b against the chain of a: (alignment pairs, end score)"""
        self.consensus([a, b], type, match, mismatch, gap_open, gap_extend)
        return self.last_alignment(), self.last_score()
