"""The exhaustive reference of the general POA path's end scores. The best score of a sequence against a directed acyclic graph is the
maximum, over the graph's source-to-sink paths, of the best pairwise score against the path's letters: a gap along the graph is a gap
along one path, a global alignment runs from a source to a sink, a local one lies inside some such path, and an overlap's free ends on
the graph are the free ends on the path that its nodes lie on. So this file needs no recurrence over predecessors, no rank order and no
sink flags, which is what the restatements (tests/poa_*_ref.cpp) share with the kernels: it lists the paths and hands each to a plain
pairwise DP (tests/pairwise_ref.cpp, int64, compiled with g++ into a directory the caller gives).

A graph here is a Graph(letter, succ): the letter of every node and the sorted successors of every node, keyed by whatever names the
nodes. The graph a sequence was aligned to is the union of the paths of the sequences before it (graph_before from a GraphRecord's
paths, graph_from_rows from MSA rows, where a node is a (column, letter) pair)."""
import ctypes as C
import os
import subprocess
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import grflib

HERE = os.path.dirname(os.path.abspath(__file__))
CAP = 2048   # source-to-sink paths per add; an add with more is reported, never skipped (the tests assert that there is none)
Graph = namedtuple("Graph", "letter succ")


def gap_scores(scores):
    """the six scores as the pairwise DP takes them: a linear gap is e = q = c = g, an affine one (q, c) = (g, e)"""
    m, x, g, e, q, c = scores
    model = grflib.model_of(scores)
    return (m, x, g, g, g, g) if model == 0 else (m, x, g, e, g, e) if model == 1 else (m, x, g, e, q, c)


class Pairwise:
    def __init__(self, build_dir):
        so = os.path.join(build_dir, "libpairwise_ref.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", os.path.join(HERE, "pairwise_ref.cpp"), "-o", so])
        L = C.CDLL(so)
        L.pw_score.restype = C.c_int64
        L.pw_score.argtypes = [C.c_char_p, C.c_int64, C.c_char_p, C.c_int64, C.c_int32, C.POINTER(C.c_int64)]
        L.pw_max.restype = C.c_int64
        L.pw_max.argtypes = [C.c_char_p, C.POINTER(C.c_int64), C.c_int64, C.c_char_p, C.c_int64, C.c_int32, C.POINTER(C.c_int64)]
        self._L = L

    def score(self, a, b, mode, scores):
        """the end score of b against a; `scores` are the DP's own six (gap_scores gives them for a gap model)"""
        assert a and b
        return self._L.pw_score(a.encode(), len(a), b.encode(), len(b), grflib.TYPES[mode], (C.c_int64 * 6)(*scores))

    def best(self, paths, b, mode, scores):
        """the maximum of score(p, b) over the strings `paths`"""
        assert paths and b and all(paths)
        off = [0]
        for p in paths:
            off.append(off[-1] + len(p))
        return self._L.pw_max("".join(paths).encode(), (C.c_int64 * len(off))(*off), len(paths), b.encode(), len(b), grflib.TYPES[mode], (C.c_int64 * 6)(*scores))


def _graph(letter, edges):
    succ = {n: [] for n in letter}
    for f, t in sorted(edges):
        succ[f].append(t)
    return Graph(letter, succ)


def graph_before(rec, k):
    """the graph sequence k of a GraphRecord was aligned to: nodes and edges of the union of the paths of sequences 0 .. k - 1"""
    letter, edges = {}, set()
    for sq in rec.sequences[:k]:
        p = [int(n) for n in sq.path]
        for n in p:
            letter[n] = rec.node_base[n]
        edges.update(zip(p, p[1:]))
    return _graph(letter, edges)


def graph_from_rows(rows, k):
    """the same graph rebuilt from the MSA rows of sequences 0 .. k - 1: a node is a (column, letter) pair, a row's path its non-gap
    columns in order"""
    letter, edges = {}, set()
    for row in rows[:k]:
        p = [(j, ch) for j, ch in enumerate(row) if ch != "-"]
        for n in p:
            letter[n] = n[1]
        edges.update(zip(p, p[1:]))
    return _graph(letter, edges)


def _order(graph):
    """the nodes in a topological order (Kahn)"""
    indeg = {n: 0 for n in graph.letter}
    for ss in graph.succ.values():
        for t in ss:
            indeg[t] += 1
    ready = sorted(n for n, d in indeg.items() if d == 0)
    order = []
    while ready:
        n = ready.pop()
        order.append(n)
        for t in graph.succ[n]:
            indeg[t] -= 1
            if indeg[t] == 0:
                ready.append(t)
    assert len(order) == len(graph.letter), "the graph has a cycle"
    return order


def sources(graph):
    has_in = {t for ss in graph.succ.values() for t in ss}
    return sorted(n for n in graph.letter if n not in has_in)


def fan_in(graph):
    """the largest number of predecessors of a node"""
    indeg = {}
    for ss in graph.succ.values():
        for t in ss:
            indeg[t] = indeg.get(t, 0) + 1
    return max(indeg.values(), default=0)


def count_paths(graph):
    """the number of source-to-sink paths (Python integers: it can be astronomic)"""
    cnt = {}
    for n in reversed(_order(graph)):
        cnt[n] = sum(cnt[t] for t in graph.succ[n]) if graph.succ[n] else 1
    return sum(cnt[n] for n in sources(graph))


def path_strings(graph):
    """the letters of every source-to-sink path, each string once. Only the sources and the successors of a node that branches keep a set
    of strings (a chain between two branches is walked, not stored), so a long near-chain costs little."""
    srcs = sources(graph)
    keep = set(srcs)
    for ss in graph.succ.values():
        if len(ss) > 1:
            keep.update(ss)
    tails = {}
    for n in reversed(_order(graph)):
        if n not in keep:
            continue
        run, at = [graph.letter[n]], n
        while len(graph.succ[at]) == 1:
            at = graph.succ[at][0]
            run.append(graph.letter[at])
        run = "".join(run)
        tails[n] = {run + s for t in graph.succ[at] for s in tails[t]} if graph.succ[at] else {run}
    return sorted(set().union(*(tails[n] for n in srcs))) if srcs else []


def optimum(pw, graph, seq, mode, scores, cap=CAP, strings=None):
    """(the best end score of seq against the graph, the number of the graph's source-to-sink paths); the score is None when the graph
    holds more than `cap` paths, which a test must report as a failure. `scores` are the six of grflib's convention; `strings`: the
    graph's path_strings, where the caller has them already."""
    n_paths = count_paths(graph)
    if n_paths > cap:
        return None, n_paths
    best = pw.best(path_strings(graph) if strings is None else strings, "".join(grflib.read(c) for c in seq), mode, gap_scores(scores))
    return (max(best, 0) if mode == "sw" else best), n_paths


def first_aligned(seqs):
    """the index of the first non-empty sequence (aligned to an empty graph), or len(seqs)"""
    return next((k for k, q in enumerate(seqs) if q), len(seqs))


def compared(seqs):
    """the sequences whose score is compared: the non-empty ones behind the first non-empty one"""
    return [k for k in range(first_aligned(seqs) + 1, len(seqs)) if seqs[k]]


def graph_optima(pw, rec, seqs, mode, scores, cap=CAP):
    """per sequence of a GraphRecord None (not compared), or (the optimum against the graph before its add, that graph's paths)"""
    out = [None] * len(seqs)
    for k in compared(seqs):
        out[k] = optimum(pw, graph_before(rec, k), seqs[k], mode, scores, cap)
    return out


def strand_optima(pw, rows, seqs, rc, mode, scores, cap=CAP):
    """per sequence of a strand-ambiguous set None (not compared), or ((the optimum of the sequence as given, of rc(the sequence)), the
    paths of the graph before its add); rows: the MSA rows of the sequences as they were added"""
    out = [None] * len(seqs)
    for k in compared(seqs):
        g = graph_from_rows(rows, k)
        strings = path_strings(g) if count_paths(g) <= cap else None
        fwd, n = optimum(pw, g, seqs[k], mode, scores, cap, strings)
        out[k] = ((fwd, optimum(pw, g, rc(seqs[k]), mode, scores, cap, strings)[0]), n)
    return out


def _tally(optima, over_cap):
    flat = [(s, k, o) for s, per in enumerate(optima) for k, o in enumerate(per) if o is not None]
    return len(flat), sum(1 for _, _, o in flat if o[1] > 1), max((o[1] for _, _, o in flat), default=0), [(s, k) for s, k, o in flat if over_cap(o)]


def tally_graph(optima):
    """over the graph_optima of many sets: (alignments compared, those that faced more than one path, the largest path count, the (set,
    sequence) pairs over the cap)"""
    return _tally(optima, lambda o: o[0] is None)


def tally_strand(optima):
    """the same over the strand_optima of many sets, whose entries hold a pair of scores"""
    return _tally(optima, lambda o: o[0][0] is None)


class Reference:
    """the restatements' records of every (inputs, type, scores) and their optima, computed once on the CPU and left unchanged; ref is a
    grflib.GraphRef, sref a strlib.StrandRef (or None), pw a Pairwise. inputs: [(family, index, set)]"""

    def __init__(self, ref, sref, pw):
        self.ref, self.sref, self.pw = ref, sref, pw
        self._done = {}

    def _pmap(self, fn, items):
        with ThreadPoolExecutor(16) as ex:   # (the restatements and the pairwise DP release the GIL: ctypes)
            return list(ex.map(fn, items))

    def graph(self, inputs, mode, scores):
        """(the graph restatement's records, per set the graph_optima)"""
        key = ("graph", tuple((f, k) for f, k, _ in inputs), mode, scores)
        if key not in self._done:
            recs = self._pmap(lambda c: self.ref.graph(c[2], mode, scores), inputs)
            self._done[key] = recs, self._pmap(lambda p: graph_optima(self.pw, p[0], p[1][2], mode, scores), list(zip(recs, inputs)))
        return self._done[key]

    def strand(self, inputs, rc, mode, scores):
        """(the strand restatement's records with rows, per set the strand_optima)"""
        key = ("strand", tuple((f, k) for f, k, _ in inputs), mode, scores)
        if key not in self._done:
            recs = self._pmap(lambda c: self.sref.strand(c[2], mode, scores), inputs)
            self._done[key] = recs, self._pmap(lambda p: strand_optima(self.pw, p[0].rows, p[1][2], rc, mode, scores), list(zip(recs, inputs)))
        return self._done[key]
