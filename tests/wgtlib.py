"""ctypes loader for tests/poa_weighted_ref.cpp, the CPU restatement of a POA graph under per-base weights and of the coverage of its
consensus. It is compiled with g++ into a directory the caller gives (a pytest temporary directory, or one of tools/poa_modes_bench.py's
own). Also the seeded weightings the CPU and the GPU tests share."""
import ctypes as C
import os
import random
import subprocess
from collections import namedtuple

HERE = os.path.dirname(os.path.abspath(__file__))
TYPES = {"sw": 0, "nw": 1, "ov": 2}
# the checks the restatement makes on its own weighting and counting, as bits of Weighted.flags (a set bit: the check FAILED)
FLAGS = {1: "consecutive bases are not joined by a graph edge", 2: "a sequence passes through a node twice",
         4: "a node does not hold the letter of a base that went to it"}

# consensus: Graph::consensus() on the weighted edges; walked: the same by the walk that yields the nodes; coverage: one count per
# consensus base; profile: [A, C, G, T] per consensus base; through: sequences of >= 2 bases through the consensus node itself; cols: the
# MSA column of every consensus base
Weighted = namedtuple("Weighted", "consensus walked coverage profile through cols flags")


def _ints(line):
    return [int(v) for v in line.split()]


class WeightedRef:
    def __init__(self, build_dir):
        so = os.path.join(build_dir, "libpoa_weighted_ref.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", os.path.join(HERE, "poa_weighted_ref.cpp"), "-o", so])
        L = C.CDLL(so)
        L.pwr_weighted.restype = C.c_void_p
        L.pwr_weighted.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.c_uint32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
        L.pwr_free.argtypes = [C.c_void_p]
        self._L = L

    def weighted(self, seqs, weights=None, type="nw", match=5, mismatch=-4, gap_open=-8, gap_extend=None):
        """weights: one list of integers 1..255 per sequence, or None (all 1). gap_extend None or equal to gap_open: the linear DP."""
        arr = (C.c_char_p * max(1, len(seqs)))(*[s.encode() for s in seqs])
        warr = None
        if weights is not None:
            assert len(weights) == len(seqs) and all(len(w) == len(s) and all(1 <= v <= 255 for v in w) for w, s in zip(weights, seqs))
            warr = (C.c_char_p * max(1, len(seqs)))(*[bytes(w) + b"\0" for w in weights])
        p = self._L.pwr_weighted(arr, warr, len(seqs), match, mismatch, gap_open, gap_open if gap_extend is None else gap_extend, TYPES[type])
        lines = C.string_at(p).decode().split("\n")[:-1]
        self._L.pwr_free(p)
        prof = _ints(lines[3])
        return Weighted(lines[1], lines[0], _ints(lines[2]), [prof[i:i + 4] for i in range(0, len(prof), 4)], _ints(lines[4]), _ints(lines[5]), int(lines[6]))


def uniform_weights(sets, seed):
    """per base a weight uniform in 1..255"""
    rnd = random.Random(seed)
    return [[[rnd.randrange(1, 256) for _ in q] for q in st] for st in sets]


def quality_weights(sets, seed):
    """quality-like: per sequence a level in 5..40, per base the level +- a few, with occasional dips; all in 1..60"""
    rnd = random.Random(seed)
    out = []
    for st in sets:
        ws = []
        for q in st:
            level = rnd.randrange(5, 41)
            ws.append([max(1, min(60, (rnd.randrange(1, 8) if rnd.random() < 0.1 else level + rnd.randrange(-4, 5)))) for _ in q])
        out.append(ws)
    return out


def quality_strings(weights):
    """the weights (1..93) of one set as quality strings: character = weight + 33"""
    return ["".join(chr(v + 33) for v in w) for w in weights]
