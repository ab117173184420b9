"""Score triples (match, mismatch, gap) other than 5 / -4 / -8 for the tuned kNW path (kernels/poa.hip behind hx_poa_sequences), the sets
they are tried on, and the two CPU references of every triple: the oracle's consensus and the linear restatement's consensus and cell count.

    USUAL      the planner's gate (hx_poa_plan.hip, PoaPlanner::knobs: gap <= 0, mismatch <= match, gap <= match, match >= 0) keeps the exact
               pruning and the column passes on. Under (0, -1, -1) no score is above 0: the pruning threshold (kernels/poa.hip, "PRUNE: the
               threshold of this alignment") takes its branch for negative scores; under (0, 0, 0) every cell ties
    UNUSUAL    the gate must switch both off
    EXTREME    the ends of int8: usual signs, the largest keys
    LONG       seeded noisy sets of up to 4 200 bases (the corpus of poasets.py stops at a few hundred and never leaves the one-wave class
               unforced; 2 100 and 4 200 lie beyond wave_max 2 047) and a pair of unrelated 3 000-base sequences, whose scores run far negative

The first triple of every group runs on the whole corpus, the others on every third set of it (the convention of test_poa_hard_gpu.py),
all of them on LONG."""
import random
from concurrent.futures import ThreadPoolExecutor

import orclib
import poasets

DEFAULT = (5, -4, -8)
USUAL = [(3, -5, -4), (1, -1, -1), (2, -7, -1), (1, 0, -1), (4, 4, -2), (5, -4, 0), (0, -1, -1), (0, 0, 0)]
UNUSUAL = [(-1, 2, -3), (5, -4, 3), (-3, -3, -3)]
EXTREME = [(127, -128, -128), (1, -128, -1)]
GROUPS = {"usual": USUAL, "unusual": UNUSUAL, "extreme": EXTREME}
TRIPLES = USUAL + UNUSUAL + EXTREME
LEADING = [g[0] for g in GROUPS.values()]
NEGATIVE = (0, -1, -1)


def group_of(triple):
    return next(name for name, g in GROUPS.items() if triple in g)


def gate_keeps_pruning(match, mismatch, gap):
    """the four inequalities of the planner's gate (hx_poa_plan.hip, PoaPlanner::knobs)"""
    return gap <= 0 and mismatch <= match and gap <= match and match >= 0


def noisy(rnd, t, ins=0.06, dele=0.04, sub=0.03):
    """the noisy() of test_gpu_parity.py::test_one_workgroup_with_32_columns_per_lane"""
    out = []
    for ch in t:
        r = rnd.random()
        if r < dele:
            continue
        out.append(rnd.choice("ACGT") if r < dele + sub else ch)
        while rnd.random() < ins:
            out.append(rnd.choice("ACGT"))
    return "".join(out)


def _long():
    rnd = random.Random(7400)
    sets = []
    for length, copies in ((65, 6), (300, 5), (700, 4), (2100, 3), (4200, 3)):
        t = "".join(rnd.choice("ACGT") for _ in range(length))
        sets.append([noisy(rnd, t) for _ in range(copies)])
    sets.append(["".join(rnd.choice("ACGT") for _ in range(3000)) for _ in range(2)])
    return sets


LONG_SETS = _long()
UNRELATED_PAIR = LONG_SETS[-1]
LONG = [("long", k, st) for k, st in enumerate(LONG_SETS)]
# the oracle's matrix for the largest set stays under 100 M cells: (nodes + 1) x (columns + 1) with at most one node per base
assert max(sum(len(q) for q in st) * (max(len(q) for q in st) + 1) for st in LONG_SETS) < 100_000_000


def corpus_of(triple):
    """[(family, index, set)] a triple is tried on"""
    return (poasets.CORPUS if triple in LEADING or triple == DEFAULT else poasets.sub_sample(3)) + LONG


def sets_of(corpus):
    return [st for _, _, st in corpus]


def pmap(fn, items):
    with ThreadPoolExecutor(16) as ex:   # (the restatement and the oracle release the GIL: ctypes)
        return list(ex.map(fn, items))


def failing(corpus, got, want):
    """the (family, index) pairs of the sets whose results differ"""
    assert len(got) == len(want) == len(corpus)
    return [(f, k) for (f, k, _), a, b in zip(corpus, got, want) if a != b]


class References:
    """the CPU side of every (triple, corpus), computed once; lin is a pmrlib.ModesRef"""

    def __init__(self, lin):
        self.lin = lin
        self._done = {}

    def both(self, triple, corpus):
        """(the oracle's consensus list, the restatement's, the restatement's cell count) under kNW"""
        key = (triple, tuple((f, k) for f, k, _ in corpus))
        if key not in self._done:
            orc = pmap(lambda c: orclib.poa_consensus([poasets.as_read(q) for q in c[2]], *triple), corpus)
            res = pmap(lambda c: self.lin.consensus_cells(c[2], "nw", *triple), corpus)
            self._done[key] = (orc, [r[0] for r in res], sum(r[1] for r in res))
        return self._done[key]

    def agree(self, triple, corpus):
        """asserts that the two CPU sides give the same consensus for every set"""
        orc, res, _ = self.both(triple, corpus)
        assert failing(corpus, res, orc) == [], triple

    def want(self, triple, corpus):
        """(consensus list by the oracle, dp_cells by the restatement), the two sides having agreed"""
        self.agree(triple, corpus)
        orc, _, cells = self.both(triple, corpus)
        return orc, cells
