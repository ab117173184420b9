"""ctypes loader for tests/poa_msa_ref.cpp, the CPU restatement of the multiple sequence alignment of a POA graph. It is compiled with g++
into a directory the caller gives (a pytest temporary directory, or one of tools/poa_modes_bench.py's own)."""
import ctypes as C
import os
import subprocess
from collections import namedtuple

HERE = os.path.dirname(os.path.abspath(__file__))
TYPES = {"sw": 0, "nw": 1, "ov": 2}
# the checks the restatement makes on its own node derivation and columns, as bits of Msa.flags (a set bit: the check FAILED)
FLAGS = {1: "a derived node does not hold its base's letter", 2: "consecutive bases are not joined by a graph edge",
         4: "the derivation and add_alignment created different numbers of nodes", 8: "aligned nodes are not contiguous in the rank order",
         16: "the smallest-rank-opens rule gives other columns than the serial walk", 32: "columns do not rise strictly along a sequence"}

# rows: one per given sequence (+ the consensus row when asked for); walked: the consensus by the restated walk that also yields the
# nodes; consensus: Graph::consensus() of the linear / affine restatement
Msa = namedtuple("Msa", "n_cols flags walked consensus rows")


class MsaRef:
    def __init__(self, build_dir):
        so = os.path.join(build_dir, "libpoa_msa_ref.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", os.path.join(HERE, "poa_msa_ref.cpp"), "-o", so])
        L = C.CDLL(so)
        L.pma_msa.restype = C.c_void_p
        L.pma_msa.argtypes = [C.POINTER(C.c_char_p), C.c_uint32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
        L.pma_free.argtypes = [C.c_void_p]
        self._L = L

    def msa(self, seqs, type="nw", match=5, mismatch=-4, gap_open=-8, gap_extend=None, include_consensus=False):
        """gap_extend None or equal to gap_open: the linear restatement's DP, else the affine one's"""
        arr = (C.c_char_p * max(1, len(seqs)))(*[s.encode() for s in seqs])
        p = self._L.pma_msa(arr, len(seqs), match, mismatch, gap_open, gap_open if gap_extend is None else gap_extend, TYPES[type], int(include_consensus))
        lines = C.string_at(p).decode().split("\n")[:-1]
        self._L.pma_free(p)
        n_cols, flags = (int(v) for v in lines[0].split())
        rows = lines[3:]
        assert len(rows) == len(seqs) + int(include_consensus)
        return Msa(n_cols, flags, lines[1], lines[2], rows)

    def rows(self, seqs, type="nw", match=5, mismatch=-4, gap_open=-8, gap_extend=None, include_consensus=False):
        return self.msa(seqs, type, match, mismatch, gap_open, gap_extend, include_consensus).rows
