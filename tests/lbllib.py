"""ctypes loader for tests/poa_label_ref.cpp, the CPU restatement of per-label consensus over one shared graph on the general POA path, and
the sets that the CPU and the GPU tests share. The restatement is compiled with g++ into a directory the caller gives (a pytest temporary
directory, or one of tools/poa_modes_bench.py's own). Scores are always the six (match, mismatch, gap_open, gap_extend, gap_open2,
gap_extend2); the gap model follows from them by the C-ABI's rule (grflib.model_of). A result is a haslr_amd.hip.LabelRecord with every
field filled, the type HipContext.poa_labelled returns, so that both sides compare field by field."""
import ctypes as C
import os
import random
import subprocess

from grflib import LINEAR, AFFINE, CONVEX, TYPES, kw_of, model_of   # noqa: F401 (the score sets and rules are the graph restatement's)
from haslr_amd.hip import NO_LABEL, LabelRecord
from strlib import noisy, substituted   # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
MODELS = {"linear": LINEAR, "affine": AFFINE, "convex": CONVEX}


def _ints(line):
    return [int(v) for v in line.split()]


class LabelRef:
    def __init__(self, build_dir):
        so = os.path.join(build_dir, "libpoa_label_ref.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", os.path.join(HERE, "poa_label_ref.cpp"), "-o", so])
        L = C.CDLL(so)
        L.plr_labelled.restype = C.c_void_p
        L.plr_labelled.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.c_char_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32]
        L.plr_free.argtypes = [C.c_void_p]
        self._L = L

    def labelled_cells(self, seqs, labels, n_labels, type="nw", scores=LINEAR, weights=None, include_consensus=False):
        """(LabelRecord, dp_cells, n_cols)"""
        assert len(scores) == 6 and len(labels) == len(seqs) and all(0 <= v < n_labels or v == NO_LABEL for v in labels)
        arr = (C.c_char_p * max(1, len(seqs)))(*[s.encode() for s in seqs])
        warr = None
        if weights is not None:
            assert len(weights) == len(seqs) and all(len(w) == len(s) and all(1 <= v <= 255 for v in w) for w, s in zip(weights, seqs))
            warr = (C.c_char_p * max(1, len(seqs)))(*[bytes(w) + b"\0" for w in weights])
        p = self._L.plr_labelled(arr, warr, bytes(labels) + b"\0", len(seqs), n_labels, (C.c_int32 * 6)(*scores), model_of(scores), TYPES[type], int(bool(include_consensus)))
        ln = C.string_at(p).decode().split("\n")[:-1]
        self._L.plr_free(p)
        cells, n_cols = _ints(ln[0])
        cns, cols, cov, prof = [], [], [], []
        for g in range(n_labels):
            a, b, c, d = ln[1 + 4 * g:5 + 4 * g]
            flat = _ints(d)
            cns.append(a); cols.append(_ints(b)); cov.append(_ints(c)); prof.append([flat[i:i + 4] for i in range(0, len(flat), 4)])
        rows = ln[1 + 4 * n_labels:]
        assert len(rows) == len(seqs) + (n_labels if include_consensus else 0) and all(len(r) == n_cols for r in rows)
        return LabelRecord(cns, cols, cov, prof, rows), cells, n_cols

    def labelled(self, seqs, labels, n_labels, type="nw", scores=LINEAR, weights=None, include_consensus=False):
        return self.labelled_cells(seqs, labels, n_labels, type, scores, weights, include_consensus)[0]


# ---- the sets the CPU and the GPU tests share
def template(rnd, length):
    return "".join(rnd.choice("ACGT") for _ in range(length))


def second_haplotype(rnd, t, snps=3):
    """a copy of t with `snps` substitutions and one indel (a deletion of one base or an insertion of two), all away from its ends"""
    h = list(t)
    for p in rnd.sample(range(5, len(t) - 5), snps):
        h[p] = rnd.choice([c for c in "ACGT" if c != h[p]])
    p = rnd.randrange(5, len(t) - 5)
    if rnd.random() < 0.5:
        del h[p]
    else:
        h[p:p] = [rnd.choice("ACGT"), rnd.choice("ACGT")]
    return "".join(h)


def two_haplotypes(seed, length, per_label, err=0.05, exact=False):
    """(sequences, labels): a template and a second haplotype of it, then per_label - 1 noisy reads of each, labels 0 and 1 interleaved;
    exact: the reads carry substitutions only"""
    rnd = random.Random(seed)
    t = template(rnd, length)
    haps = [t, second_haplotype(rnd, t)]
    seqs, labels = list(haps), [0, 1]
    for _ in range(per_label - 1):
        for g in (0, 1):
            seqs.append(substituted(rnd, haps[g], err) if exact else noisy(rnd, haps[g], err) or "A")
            labels.append(g)
    return seqs, labels


def exact_set(seed, length, n=3):
    """n sequences of exactly `length` bases (a template and copies with substitutions) on labels 0, 1, 0, ...: `length` is the set's
    longest sequence and decides its kernel instance"""
    rnd = random.Random(seed)
    t = template(rnd, length)
    return [t] + [substituted(rnd, t, 0.03) for _ in range(n - 1)], [k % 2 for k in range(n)]


# hand-derived cases: (sequences, labels, n_labels, type). tests/test_poa_label_ref.py states the answers
ONE_MISMATCH = (["AAGAA", "AAGAA", "AATAA", "AATAA"], [0, 0, 1, 1], 2, "nw")
MINORITY = (["AAGAA", "AAGAA", "AAGAA", "AATAA"], [0, 0, 0, 1], 2, "nw")
# label 1 carries an A between the C's and the G's
INSERTION = (["AACCGGTT", "AACCAGGTT", "AACCGGTT", "AACCAGGTT"], [0, 1, 0, 1], 2, "nw")
# kSW. Label 0: U + M once, then Z + M twice, Z three bases that match nothing of U, so that they become a chain of their own into M's
# first node. That node's heaviest in-edge comes from Z (4 against 2), so the scores along M restart near 0 and stay below that of U's
# last node, which is the heaviest of the view and no sink of it: branch completion runs, kills Z's last node, and the walk goes on
# through M. Label 1 walks U + M + W: in the whole graph M's last node is no sink, in label 0's view it is.
BC_U, BC_Z, BC_M, BC_W = "ACGACGACCAGCAGCCAGACGACCAGCAAC", "TTT", "GGATTG", "CACACA"
BRANCH = ([BC_U + BC_M, BC_Z + BC_M, BC_Z + BC_M, BC_U + BC_M + BC_W], [0, 0, 0, 1], 2, "sw")
# label 1 holds sequences of one base only (no edge in its view: the smallest-id fallback), label 2 has no member
ONE_BASE = (["ACGT", "ACGT", "G", "C"], [0, 0, 1, 1], 3, "nw")
UNLABELLED = (["ACGT", "ACGA", "ACGT"], [NO_LABEL] * 3, 2, "nw")
HAND = {"one_mismatch": ONE_MISMATCH, "minority": MINORITY, "insertion": INSERTION, "branch": BRANCH, "one_base": ONE_BASE, "unlabelled": UNLABELLED}


def hand_weights(seqs, seed=77):
    rnd = random.Random(seed)
    return [[rnd.randrange(1, 41) for _ in q] for q in seqs]
