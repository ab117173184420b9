"""ctypes loader for tests/poa_graph_ref.cpp, the CPU restatement of the graph and alignment output of the general POA path. It is compiled
with g++ into a directory the caller gives (a pytest temporary directory, or one of tools/poa_modes_bench.py's own). Scores are always the
six (match, mismatch, gap_open, gap_extend, gap_open2, gap_extend2); the gap model follows from them by the C-ABI's rule (model_of). A
result is a haslr_amd.hip.GraphRecord, the type HipContext.poa_graph returns, so that both sides compare field by field; checks(),
rescore() and ends() state the properties such a record must have by itself, whoever made it."""
import ctypes as C
import os
import subprocess

import numpy as np

from haslr_amd.hip import GraphRecord, GraphSequence

HERE = os.path.dirname(os.path.abspath(__file__))
TYPES = {"sw": 0, "nw": 1, "ov": 2}
LINEAR, AFFINE, CONVEX = (5, -4, -8, -8, -8, -8), (5, -4, -8, -6, -8, -6), (5, -4, -8, -6, -10, -4)


def model_of(scores):
    """0 linear, 1 affine, 2 convex: a second piece that extends no cheaper than the first never wins, and then equal open and extend are the linear model"""
    _, _, g, e, _, c = scores
    return 2 if c > e else 1 if e != g else 0


def kw_of(scores, mode):
    """the keyword arguments of HipContext.poa_graph for six scores"""
    return dict(type=mode, match=scores[0], mismatch=scores[1], gap_open=scores[2], gap_extend=scores[3], gap_open2=scores[4], gap_extend2=scores[5])


def gap_score(scores, k):
    """the score of a gap of k >= 1 bases under the model of the scores"""
    _, _, g, e, q, c = scores
    return max(g + (k - 1) * e, q + (k - 1) * c) if model_of(scores) == 2 else g + (k - 1) * e


def _ints(line, dtype):
    return np.fromstring(line, dtype=np.int64, sep=" ").astype(dtype)


class GraphRef:
    def __init__(self, build_dir):
        so = os.path.join(build_dir, "libpoa_graph_ref.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", os.path.join(HERE, "poa_graph_ref.cpp"), "-o", so])
        L = C.CDLL(so)
        L.pgr_graph.restype = C.c_void_p
        L.pgr_graph.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(C.c_int32), C.c_int32, C.c_int32]
        L.pgr_replay.restype = C.c_void_p
        L.pgr_replay.argtypes = [C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.pgr_free.argtypes = [C.c_void_p]
        self._L = L

    def _take(self, p):
        s = C.string_at(p).decode()
        self._L.pgr_free(p)
        return s.split("\n")[:-1]

    def graph_cells(self, seqs, type="nw", scores=LINEAR, weights=None):
        """(GraphRecord, sum of V * L over the alignments, per sequence the (nodes, edges) of the graph it was aligned to)"""
        assert len(scores) == 6
        arr = (C.c_char_p * max(1, len(seqs)))(*[s.encode() for s in seqs])
        warr = None
        if weights is not None:
            assert len(weights) == len(seqs) and all(len(w) == len(s) and all(1 <= v <= 255 for v in w) for w, s in zip(weights, seqs))
            warr = (C.c_char_p * max(1, len(seqs)))(*[bytes(w) + b"\0" for w in weights])
        ln = self._take(self._L.pgr_graph(arr, warr, len(seqs), (C.c_int32 * 6)(*scores), model_of(scores), TYPES[type]))
        cells, n_cols = (int(v) for v in ln[8].split())
        sq, before = [], []
        for k in range(len(seqs)):
            path, aln, tail = ln[9 + 3 * k:12 + 3 * k]
            score, vb, eb = (int(v) for v in tail.split())
            flat = np.fromstring(aln.replace(":", " "), dtype=np.int64, sep=" ").tolist()   # (node:pos pairs; parsed in one go: the corpus tests read millions)
            sq.append(GraphSequence(_ints(path, np.uint32), list(zip(flat[0::2], flat[1::2])), score))
            before.append((vb, eb))
        rec = GraphRecord(ln[0], _ints(ln[1], np.uint32), _ints(ln[2], np.uint32), _ints(ln[3], np.uint32), _ints(ln[4], np.uint32), _ints(ln[5], np.int32), n_cols, sq,
                          ln[6], _ints(ln[7], np.uint32))
        return rec, cells, before

    def graph(self, seqs, type="nw", scores=LINEAR, weights=None):
        return self.graph_cells(seqs, type, scores, weights)[0]

    def replay(self, seqs, rec):
        """the sequences' alignments through a fresh graph's add_alignment: (node letters, edge_from, edge_to, edge_w on unit weights)"""
        off = np.zeros(len(seqs) + 1, dtype=np.uint64)
        for k, sq in enumerate(rec.sequences):
            off[k + 1] = off[k] + len(sq.alignment)
        flat = [p for sq in rec.sequences for p in sq.alignment]
        an, ap = (C.c_int32 * max(1, len(flat)))(*[p[0] for p in flat]), (C.c_int32 * max(1, len(flat)))(*[p[1] for p in flat])
        arr = (C.c_char_p * max(1, len(seqs)))(*[s.encode() for s in seqs])
        ln = self._take(self._L.pgr_replay(arr, len(seqs), off.ctypes.data_as(C.POINTER(C.c_uint64)), an, ap))
        return ln[0], _ints(ln[3], np.uint32), _ints(ln[4], np.uint32), _ints(ln[5], np.int32)


def same(a, b):
    """two GraphRecords hold the same values, element for element"""
    return (a.node_base == b.node_base and a.consensus == b.consensus and a.n_cols == b.n_cols and len(a.sequences) == len(b.sequences)
            and all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("node_rank", "node_col", "edge_from", "edge_to", "edge_w", "consensus_nodes"))
            and all(np.array_equal(x.path, y.path) and x.alignment == y.alignment and x.score == y.score for x, y in zip(a.sequences, b.sequences)))


def read(c):
    """a letter as every entry point reads it: lower case is upper case, anything but ACGT is A"""
    c = c.upper()
    return c if c in "ACGT" else "A"


def rows_of(rec, seqs):
    """the MSA rows of the given sequences, rebuilt from their paths and the nodes' columns"""
    rows = []
    for q, sq in zip(seqs, rec.sequences):
        row = ["-"] * rec.n_cols
        for ch, nd in zip(q, sq.path):
            row[int(rec.node_col[nd])] = read(ch)
        rows.append("".join(row))
    return rows


def checks(rec, seqs, weights=None):
    """the properties a record has by itself; returns the list of those that do NOT hold (empty: all hold)"""
    bad = []
    V, E = len(rec.node_base), len(rec.edge_from)
    edge = {(int(f), int(t)): e for e, (f, t) in enumerate(zip(rec.edge_from, rec.edge_to))}
    if len(edge) != E:
        bad.append("an edge stands twice")
    want_w = [0] * E
    for k, (q, sq) in enumerate(zip(seqs, rec.sequences)):
        p = [int(n) for n in sq.path]
        if len(p) != len(q) or any(n >= V for n in p) or "".join(rec.node_base[n] for n in p) != "".join(read(c) for c in q):
            bad.append(f"path {k} does not spell its sequence")
            continue
        for i in range(1, len(p)):
            e = edge.get((p[i - 1], p[i]))
            if e is None:
                bad.append(f"path {k}: no edge between the nodes of bases {i - 1} and {i}")
            else:
                want_w[e] += (weights[k][i - 1] + weights[k][i]) if weights is not None else 2
        if any(rec.node_col[p[i]] <= rec.node_col[p[i - 1]] for i in range(1, len(p))):
            bad.append(f"path {k}: columns do not rise strictly")
    if want_w != [int(w) for w in rec.edge_w]:
        bad.append("an edge's weight is not the sum over the paths' traversals")
    rank = [int(r) for r in rec.node_rank]
    if sorted(rank) != list(range(V)):
        bad.append("node_rank is no permutation")
    elif any(rank[int(f)] >= rank[int(t)] for f, t in zip(rec.edge_from, rec.edge_to)):
        bad.append("an edge runs against the rank order")
    else:
        by_col = {}
        for n in range(V):
            by_col.setdefault(int(rec.node_col[n]), []).append(n)
        if sorted(by_col) != list(range(rec.n_cols)):
            bad.append("the columns are not 0 .. n_cols - 1")
        for c, ns in by_col.items():
            rs = sorted(rank[n] for n in ns)
            if rs != list(range(rs[0], rs[0] + len(ns))) or len(set(rec.node_base[n] for n in ns)) != len(ns):
                bad.append(f"column {c}: its nodes are not consecutive in rank with distinct letters")
        order = sorted(range(V), key=lambda n: rank[n])
        if any(rec.node_col[order[r]] < rec.node_col[order[r - 1]] for r in range(1, V)):
            bad.append("columns fall along the rank order")
    cn = [int(n) for n in rec.consensus_nodes]
    if "".join(rec.node_base[n] for n in cn) != rec.consensus:
        bad.append("the consensus nodes do not spell the consensus")
    if any((cn[i - 1], cn[i]) not in edge for i in range(1, len(cn))):
        bad.append("two consecutive consensus nodes are not joined by an edge")
    return bad


def rescore(rec, seqs, scores, type, before=None):
    """every alignment's pairs scored again under the gap model: matches and mismatches against the graph's letters, runs of pairs
    without a node or without a position as gaps; consecutive pairs with a node must be joined by an edge that existed before the add
    (edge ids below before[k][1]; without `before`, the edges made by sequences 0 .. k-1 are derived from the paths). Returns the list of
    what does NOT hold."""
    bad = []
    m, x = scores[0], scores[1]
    edge = {(int(f), int(t)): e for e, (f, t) in enumerate(zip(rec.edge_from, rec.edge_to))}
    seen_e, seen_v = -1, -1   # the largest edge and node id the earlier paths reach
    for k, (q, sq) in enumerate(zip(seqs, rec.sequences)):
        vb, eb = before[k] if before is not None else (seen_v + 1, seen_e + 1)
        a = sq.alignment
        if a:
            total, i = 0, 0
            prev = None
            while i < len(a):
                nd, ps = a[i]
                if nd != -1 and ps != -1:
                    total += m if rec.node_base[nd] == read(q[ps]) else x
                    j = i + 1
                else:
                    j = i
                    while j < len(a) and (a[j][0] == -1) == (nd == -1) and (a[j][1] == -1) == (ps == -1):
                        j += 1
                    total += gap_score(scores, j - i)
                for t in range(i, j):
                    if a[t][0] != -1:
                        if a[t][0] >= vb:
                            bad.append(f"alignment {k}: node {a[t][0]} did not exist before the add")
                        elif prev is not None and edge.get((prev, a[t][0]), 1 << 62) >= eb:
                            bad.append(f"alignment {k}: nodes {prev} and {a[t][0]} were not joined before the add")
                        prev = a[t][0]
                i = j
            pos = [p for _, p in a if p != -1]
            if pos != list(range(pos[0], pos[0] + len(pos))) if pos else False:
                bad.append(f"alignment {k}: its positions are not consecutive")
            if type == "nw" and pos != list(range(len(q))):
                bad.append(f"alignment {k}: a global alignment does not hold every position")
            if total != sq.score:
                bad.append(f"alignment {k}: its pairs score {total}, the end cell {sq.score}")
        elif sq.score != 0:
            bad.append(f"alignment {k}: empty with score {sq.score}")
        p = [int(n) for n in sq.path]
        if p:
            seen_v = max(seen_v, max(p))
            seen_e = max([seen_e] + [edge.get((p[i - 1], p[i]), -1) for i in range(1, len(p))])
    return bad


def ends(rec, seqs, type):
    """where every alignment starts and ends in the graph as it was before the add (the union of the earlier paths), which rescore does not
    look at. The rules are read off the DP's boundary, end and stop rules (DESIGN.md "General POA path"; dp_rows and the restatements):
    row 0 is the predecessor of the rows without in-edges only, and the walk emits a pair per move.

    kNW  the end cell is (a sink, L) and the walk stops at (0, 0) only. Row 0 is left to a source, by a diagonal or a vertical move, which
         both carry the node: the first pair with a node holds a source, the last one the end cell's row, a sink. (rescore holds the
         positions to 0 .. L - 1.)
    kOV  the end cell (i, j), j >= 1, is in a sink's row or in column L; the walk stops in row 0 or in column 0.
         Start: column 0 is entered by a diagonal or a horizontal move, which both carry position 0, and row 0 from a source: the
         alignment holds position 0, or its first pair with a node holds a source.
         End: horizontal moves leave the row, so the last pair with a node, if there is one, holds the end cell's row; vertical moves
         leave the column, so the last position, if there is one, is j - 1. An alignment with both holds position L - 1 or ends in a
         sink. One without a position (a walk straight up column j, as ["A", "C"] under a dear mismatch) records neither j nor anything
         else of its end, and one without a node nothing of its row: of those only the start is checked.
    kSW  may start and end anywhere.
    Returns the list of what does NOT hold."""
    bad = []
    has_in, has_out = set(), set()   # the nodes with an edge into / out of them among the edges the earlier paths walk
    for k, (q, sq) in enumerate(zip(seqs, rec.sequences)):
        nodes = [n for n, _ in sq.alignment if n != -1]
        pos = [p for _, p in sq.alignment if p != -1]
        if sq.alignment and type == "nw":
            if not nodes:
                bad.append(f"alignment {k}: a global alignment holds no node")
            else:
                if nodes[0] in has_in:
                    bad.append(f"alignment {k}: a global alignment starts at node {nodes[0]}, which is no source")
                if nodes[-1] in has_out:
                    bad.append(f"alignment {k}: a global alignment ends at node {nodes[-1]}, which is no sink")
        elif sq.alignment and type == "ov":
            if not (pos and pos[0] == 0) and not (nodes and nodes[0] not in has_in):
                bad.append(f"alignment {k}: an overlap starts neither at position 0 nor at a source")
            if nodes and pos and pos[-1] != len(q) - 1 and nodes[-1] in has_out:
                bad.append(f"alignment {k}: an overlap ends neither at the last position nor at a sink")
        p = [int(n) for n in sq.path]
        has_out.update(p[:-1])
        has_in.update(p[1:])
    return bad


def parse_gfa(text):
    """the graph a GFA 1 text of graph_to_gfa's form holds: dict with nodes (letter, rank, column per id), edges (from, to, weight in
    line order) and paths {name: [node ids]}"""
    lines = text.split("\n")
    assert lines[0] == "H\tVN:Z:1.0" and lines[-1] == ""
    nodes, edges, paths = [], [], {}
    for ln in lines[1:-1]:
        f = ln.split("\t")
        if f[0] == "S":
            assert int(f[1]) == len(nodes) + 1 and len(f[2]) == 1 and f[3].startswith("rk:i:") and f[4].startswith("cl:i:")
            nodes.append((f[2], int(f[3][5:]), int(f[4][5:])))
        elif f[0] == "L":
            assert f[2] == "+" and f[4] == "+" and f[5] == "0M" and f[6].startswith("ew:i:") and not paths
            edges.append((int(f[1]) - 1, int(f[3]) - 1, int(f[6][5:])))
        else:
            assert f[0] == "P" and f[1] not in paths and all(s.endswith("+") for s in f[2].split(","))
            p = [int(s[:-1]) - 1 for s in f[2].split(",")]
            assert f[3] == (",".join(["0M"] * (len(p) - 1)) if len(p) > 1 else "*")
            paths[f[1]] = p
    return dict(nodes=nodes, edges=edges, paths=paths)


def gfa_of(rec, names=None):
    """what parse_gfa must return for a record"""
    paths = {(names[k] if names else f"s{k}"): [int(n) for n in sq.path] for k, sq in enumerate(rec.sequences) if len(sq.path)}
    if len(rec.consensus_nodes):
        paths["consensus"] = [int(n) for n in rec.consensus_nodes]
    return dict(nodes=[(b, int(r), int(c)) for b, r, c in zip(rec.node_base, rec.node_rank, rec.node_col)],
                edges=[(int(f), int(t), int(w)) for f, t, w in zip(rec.edge_from, rec.edge_to, rec.edge_w)], paths=paths)


def parse_dot(text):
    """the graph a DOT text of graph_to_dot's form holds: dict with the digraph's name, nodes (letter per id), filled (ids), edges (from,
    to, weight in line order: per node its out-list) and aligned (pairs, smaller id first)"""
    import re
    lines = text.split("\n")
    m = re.fullmatch(r"digraph (\d+) \{", lines[0])
    assert m and lines[1] == "    graph [rankdir = LR]" and lines[-2:] == ["}", ""]
    nodes, filled, edges, aligned = [], [], [], []
    for ln in lines[2:-2]:
        n = re.fullmatch(r'    (\d+) \[label = "(\d+) - ([ACGT])"(, style = filled, fillcolor = goldenrod1)?\]', ln)
        e = re.fullmatch(r'    (\d+) -> (\d+) \[label = "(-?\d+)"\]', ln)
        a = re.fullmatch(r"    (\d+) -> (\d+) \[style = dotted, arrowhead = none\]", ln)
        assert n or e or a, ln
        if n:
            assert int(n.group(1)) == int(n.group(2)) == len(nodes)
            nodes.append(n.group(3))
            if n.group(4):
                filled.append(len(nodes) - 1)
        elif e:
            assert int(e.group(1)) == len(nodes) - 1   # (an edge stands under its source node)
            edges.append((int(e.group(1)), int(e.group(2)), int(e.group(3))))
        else:
            assert int(a.group(1)) == len(nodes) - 1 and int(a.group(2)) > int(a.group(1))
            aligned.append((int(a.group(1)), int(a.group(2))))
    return dict(name=int(m.group(1)), nodes=nodes, filled=filled, edges=edges, aligned=aligned)


def dot_of(rec):
    """what parse_dot must return for a record"""
    V = len(rec.node_base)
    es = sorted(((int(f), e, int(t), int(w)) for e, (f, t, w) in enumerate(zip(rec.edge_from, rec.edge_to, rec.edge_w))))
    return dict(name=sum(1 for sq in rec.sequences if len(sq.path)), nodes=list(rec.node_base), filled=sorted(set(int(n) for n in rec.consensus_nodes)),
                edges=[(f, t, w) for f, _, t, w in es],
                aligned=[(a, b) for a in range(V) for b in range(a + 1, V) if rec.node_col[a] == rec.node_col[b]])
