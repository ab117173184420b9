"""ctypes loader for tests/poa_modes_ref.cpp, the CPU restatement of the three POA alignment modes. It is compiled with g++ into a
directory the caller gives (a pytest temporary directory, or one of tools/poa_modes_bench.py's own)."""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
TYPES = {"sw": 0, "nw": 1, "ov": 2}
# the tie-break mutants of the restatement (poa_modes_ref.cpp, PMR_MUTANT): each breaks one rule, for tests that ask whether their inputs tell the rules apart
MUTANTS = {"last_end_cell": 1, "vertical_first": 2, "horizontal_first": 3, "last_predecessor": 4, "strict_bundle_tie": 5}
STATS = ("tied", "max_candidates", "ties_above_8", "closure_above_32", "max_in_degree", "wide_rows", "max_sinks")


class ModesRef:
    def __init__(self, build_dir, mutant=None):
        so = os.path.join(build_dir, "libpoa_modes_ref%s.so" % ("" if mutant is None else "_" + mutant))
        define = [] if mutant is None else ["-DPMR_MUTANT=%d" % MUTANTS[mutant]]
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", *define, os.path.join(HERE, "poa_modes_ref.cpp"), "-o", so])
        L = C.CDLL(so)
        L.pmr_consensus.restype = C.c_void_p
        L.pmr_consensus.argtypes = [C.POINTER(C.c_char_p), C.c_uint32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint64)]
        L.pmr_last_alignment.restype = C.c_int32
        L.pmr_last_alignment.argtypes = [C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32]
        L.pmr_free.argtypes = [C.c_void_p]
        L.pmr_last_stats.restype = None
        L.pmr_last_stats.argtypes = [C.POINTER(C.c_uint64 * 7)]
        self._L = L

    def consensus_cells(self, seqs, type="nw", match=5, mismatch=-4, gap=-8):
        """(consensus, sum of V * L over the alignments)"""
        arr = (C.c_char_p * max(1, len(seqs)))(*[s.encode() for s in seqs])
        cells = C.c_uint64(0)
        p = self._L.pmr_consensus(arr, len(seqs), match, mismatch, gap, TYPES[type], C.byref(cells))
        s = C.string_at(p).decode()
        self._L.pmr_free(p)
        return s, cells.value

    def consensus(self, seqs, type="nw", match=5, mismatch=-4, gap=-8):
        return self.consensus_cells(seqs, type, match, mismatch, gap)[0]

    def last_alignment(self):
        """the (node | -1, position | -1) pairs of the last alignment the calling thread made"""
        n = self._L.pmr_last_alignment(None, None, 0)
        a, b = (C.c_int32 * max(1, n))(), (C.c_int32 * max(1, n))()
        self._L.pmr_last_alignment(a, b, n)
        return [(a[k], b[k]) for k in range(n)]

    def last_stats(self):
        """what the last consensus of the calling thread met, as a dict over STATS (poa_modes_ref.cpp: pmr_last_stats)"""
        o = (C.c_uint64 * 7)()
        self._L.pmr_last_stats(C.byref(o))
        return dict(zip(STATS, o))

    def consensus_stats(self, seqs, type="nw", match=5, mismatch=-4, gap=-8):
        """(consensus, sum of V * L, statistics)"""
        s, cells = self.consensus_cells(seqs, type, match, mismatch, gap)
        return s, cells, self.last_stats()
