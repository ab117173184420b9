"""Score sets other than the well-behaved handful for the general POA path (kernels/poa_modes*.{hip,inl} behind hx_poa_graph and its
siblings), the sets they are tried on, and the score bound of the full matrix. The groups follow scorelib.py, which holds the tuned kNW
path to such scores. A score set is six scores (match, mismatch, g, e, q, c) in grflib's convention (kw_of, model_of) and comes in a
linear, an affine and a convex form, each inside the C ABI's rules (g < 0, g <= e <= 0, q <= c <= 0, q <= g); a convex form has c > e, so
that the call stays on the convex kernel without an option.

    USUAL      match >= mismatch, match >= 0: mismatch 0, mismatch equal to match, nothing positive, everything but the gap open tying at
               0 (the ABI wants g < 0), and extend scores of 0 (the linear form has no extend score: its gap is the smallest, -1)
    UNUSUAL    mismatch above match, both positive with mismatch above match, everything equal and negative
    EXTREME    the ends of int8 in every field the model has

Under NOTHING_POSITIVE no score is above 0, so that kSW never finds a cell above 0 and every local alignment is empty.

The corpus is every third set of poasets.CORPUS (the convention of test_poa_hard_gpu.py), each cut to its first 64 members, and two seeded sets of 1 100 bases: three noisy
copies of a template, and a pair of unrelated sequences. Both lie past the 64 x 16 instance (1 024 columns), so that a row's prefix maxima
cross wavefronts through s_wtot, and on both the scores run far from 0."""
import random
from concurrent.futures import ThreadPoolExecutor

import grflib
import poasets
from scorelib import noisy

MODELS = ["linear", "affine", "convex"]
MODES = ["sw", "nw", "ov"]
DEFAULT = {"linear": grflib.LINEAR, "affine": grflib.AFFINE, "convex": grflib.CONVEX}
# name -> (linear, affine, convex)
USUAL = {
    "mismatch_0": ((1, 0, -1, -1, -1, -1), (1, 0, -2, -1, -2, -1), (1, 0, -2, -1, -4, 0)),
    "mismatch_is_match": ((4, 4, -2, -2, -2, -2), (4, 4, -3, -1, -3, -1), (4, 4, -3, -2, -6, -1)),
    "nothing_positive": ((0, -1, -1, -1, -1, -1), (0, -1, -2, -1, -2, -1), (0, -1, -2, -2, -5, -1)),
    "all_ties": ((0, 0, -1, -1, -1, -1), (0, 0, -1, 0, -1, 0), (0, 0, -1, -1, -3, 0)),
    "extend_0": ((5, -4, -1, -1, -1, -1), (5, -4, -8, 0, -8, 0), (5, -4, -8, -6, -20, 0)),
}
UNUSUAL = {
    "mismatch_above_match": ((-1, 2, -3, -3, -3, -3), (-1, 2, -3, -1, -3, -1), (-1, 2, -3, -2, -5, -1)),
    "both_positive": ((5, 7, -4, -4, -4, -4), (5, 7, -4, -2, -4, -2), (5, 7, -4, -3, -8, -1)),
    "all_equal_negative": ((-3, -3, -3, -3, -3, -3), (-3, -3, -3, -2, -3, -2), (-3, -3, -3, -3, -6, -2)),
}
EXTREME = {
    "int8_ends": ((127, -128, -128, -128, -128, -128), (127, -128, -128, -1, -128, -1), (127, -128, -128, -1, -128, 0)),
    "int8_mismatch": ((1, -128, -1, -1, -1, -1), (1, -128, -2, -1, -2, -1), (1, -128, -2, -1, -128, 0)),
}
GROUPS = {"usual": USUAL, "unusual": UNUSUAL, "extreme": EXTREME}
NAMES = [n for g in GROUPS.values() for n in g]
LEADING = [next(iter(g)) for g in GROUPS.values()]
NOTHING_POSITIVE = ["nothing_positive", "all_ties", "all_equal_negative"]


def scores_of(name, model):
    """the six scores of a named set in the form of a gap model ("linear", "affine", "convex")"""
    six = next(g[name] for g in GROUPS.values() if name in g)[MODELS.index(model)]
    m, x, g, e, q, c = six
    assert g < 0 and g <= e <= 0 and q <= c <= 0 and q <= g and grflib.model_of(six) == MODELS.index(model), six
    return six


def group_of(name):
    return next(k for k, g in GROUPS.items() if name in g)


def scaled(scores, k):
    return tuple(k * v for v in scores)


def same_but_scores(a, b, k):
    """GraphRecord a is GraphRecord b with every end score k times b's"""
    bare = [r._replace(sequences=[sq._replace(score=0) for sq in r.sequences]) for r in (a, b)]
    return grflib.same(*bare) and [sq.score for sq in a.sequences] == [k * sq.score for sq in b.sequences]


def _long():
    rnd = random.Random(7411)
    t = "".join(rnd.choice("ACGT") for _ in range(1100))
    return [noisy(rnd, t) for _ in range(3)], ["".join(rnd.choice("ACGT") for _ in range(1100)) for _ in range(2)]


NOISY_1100, UNRELATED_PAIR = _long()
LONG = [("long", 0, NOISY_1100), ("long", 1, UNRELATED_PAIR)]
assert all(1024 <= max(len(q) for q in st) <= 1300 for _, _, st in LONG)   # past the 64 x 16 instance, and no set larger than that
MAX_MEMBERS = 64   # (a workgroup aligns a set's members one after the other: the sets of hundreds of members are test_poa_hard_gpu.py's subject, here they only take time)
CORPUS = [(f, k, st[:MAX_MEMBERS]) for f, k, st in poasets.sub_sample(3)] + LONG


def light(corpus, bases=8000):
    """the sets of at most `bases` bases: a workgroup aligns a set's members one after the other, so the largest set of a call decides how
    long the call takes, whatever else it holds; for the tests that make many calls"""
    return [c for c in corpus if sum(len(q) for q in c[2]) <= bases]


def chain_cells(seqs):
    """the cells of a set none of whose alignments joins anything: every sequence meets the chains of all earlier ones"""
    done = cells = 0
    for q in seqs:
        cells += done * len(q)
        done += len(q)
    return cells


# Under NOTHING_POSITIVE every kSW alignment is empty and a kOV alignment is a pair or two at a corner: a set's graph is little less than the
# disjoint chains of its members, and a set of 400 members costs the restatement 10^9 cells. There the corpus is the sets that stay under 10^7
# as disjoint chains (the kernel meets the sets of many members under kNW, and under the other score sets)
DISJOINT_CORPUS = [c for c in CORPUS if chain_cells(c[2]) <= 10_000_000]


def corpus_of(name, mode):
    """[(family, index, set)] a named score set is tried on under a type"""
    return DISJOINT_CORPUS if mode != "nw" and name in NOTHING_POSITIVE else CORPUS


# ---- the score bound of the full matrix (kernels/poa_modes_plan.h, SCORE_BOUND; DESIGN.md section 11, "Score range of the full matrix")
SCORE_BOUND = 1 << 29
COLUMNS = {"linear": [64 * 16, 256 * 16, 256 * 32, 1024 * 32], "affine": [64 * 16, 256 * 16, 512 * 16, 1024 * 16], "convex": [64 * 16, 128 * 16, 256 * 16, 512 * 16]}


def columns_of(seqs, model):
    """the columns of the instance a set runs in: the first that holds its longest sequence + 1"""
    return next(c for c in COLUMNS[model] if c >= max(len(q) for q in seqs) + 1)


def bound_product(seqs, scores, model):
    """(bases + columns of the instance) x the largest score magnitude: what describe() holds below 2^29"""
    return (sum(len(q) for q in seqs) + columns_of(seqs, model)) * max(abs(v) for v in scores)


def refusal(who, set_, seqs, scores, model):
    """the text of the refusal of set `set_` of a call"""
    bases, cols, mag = sum(len(q) for q in seqs), columns_of(seqs, model), max(abs(v) for v in scores)
    return (f"{who}: set {set_} holds {bases} bases, its instance {cols} columns: with scores of up to {mag} their product {(bases + cols) * mag} "
            f"reaches 2^29 = {SCORE_BOUND} (a set's scores must stay below it)")


def sets_of(corpus):
    return [st for _, _, st in corpus]


def pmap(fn, items):
    with ThreadPoolExecutor(16) as ex:   # (the restatements release the GIL: ctypes)
        return list(ex.map(fn, items))


def failing(corpus, got, want, same=lambda a, b: a == b):
    """the (family, index) pairs of the sets whose results differ"""
    assert len(got) == len(want) == len(corpus)
    return [(f, k) for (f, k, _), a, b in zip(corpus, got, want) if not same(a, b)]


class References:
    """the graph restatement's records of every (scores, type, corpus), computed once and left unchanged; ref is a grflib.GraphRef"""

    def __init__(self, ref):
        self.ref = ref
        self._done = {}

    def records(self, scores, mode, corpus=None):
        corpus = CORPUS if corpus is None else corpus
        key = (scores, mode, tuple((f, k) for f, k, _ in corpus))
        if key not in self._done:
            self._done[key] = pmap(lambda c: self.ref.graph_cells(c[2], mode, scores), corpus)
        return [r[0] for r in self._done[key]]

    def cells(self, scores, mode, corpus=None):
        self.records(scores, mode, corpus)
        corpus = CORPUS if corpus is None else corpus
        return sum(r[1] for r in self._done[(scores, mode, tuple((f, k) for f, k, _ in corpus))])
