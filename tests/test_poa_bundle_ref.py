"""The sets of tests/bundlesets.py, judged by the CPU side alone. The final graph of every set comes from the restatement
(grflib.GraphRef.graph: edges in creation order = in-edge order, node_rank = spoa's order); a plain forward pass of the heaviest bundle
over it (bundlesets.forward_pass) and the chunked scheme of kernels/poa_graph.inl's bundle_pass_free (bundlesets.chunked_pass) must give the
same score and predecessor for every node, the restatement's consensus is the oracle's, and every family's premise is read off the graph
itself - in spoa's order and, where a chunk boundary matters, in that order shifted by every offset 0 .. 63, so that no premise depends on
where the kernel's own order puts its boundaries. tests/test_poa_bundle_gpu.py runs the same sets through the kernel."""
from concurrent.futures import ThreadPoolExecutor

import pytest

import bundlesets
import grflib
import orclib
import pmrlib
from bundlesets import BUILT, CHUNK


class Graph:
    def __init__(self, rec):
        self.rec = rec
        V = len(rec.node_base)
        self.order = sorted(range(V), key=lambda n: int(rec.node_rank[n]))
        self.rank = [int(r) for r in rec.node_rank]
        self.in_edges = [[] for _ in range(V)]
        self.out_deg = [0] * V
        for f, t, w in zip(rec.edge_from, rec.edge_to, rec.edge_w):
            self.in_edges[int(t)].append((int(f), int(w)))
            self.out_deg[int(f)] += 1
        self.score, self.pred = bundlesets.forward_pass(self.order, self.in_edges)

    def top(self, n):
        """the sources of n's in-edges of maximal weight, in in-edge order"""
        es = self.in_edges[n]
        wmax = max((w for _, w in es), default=None)
        return [f for f, w in es if w == wmax]

    def tied(self):
        return [n for n in self.order if len(self.top(n)) > 1]

    def walk_back(self, n):
        out = []
        while n != -1:
            out.append(n)
            n = self.pred[n]
        return out[::-1]


@pytest.fixture(scope="module")
def graphs(built, tmp_path_factory):
    """{name: Graph of the set's final graph}; on the way the restatement's consensus of every set is compared with the oracle's"""
    ref = grflib.GraphRef(str(tmp_path_factory.mktemp("bundle_grf")))
    with ThreadPoolExecutor(16) as ex:   # (the restatement and the oracle release the GIL: ctypes)
        recs = list(ex.map(lambda b: ref.graph(b[2], "nw"), BUILT))
        cns = list(ex.map(lambda b: orclib.poa_consensus(b[2]), BUILT))
    assert [n for (_, n, _), r, c in zip(BUILT, recs, cns) if r.consensus != c] == []
    return {n: Graph(r) for (_, n, _), r in zip(BUILT, recs)}


def of(family):
    return [(n, st) for f, n, st in BUILT if f == family]


def test_the_sets_are_seeded_and_small():
    assert bundlesets._build() == BUILT
    assert sorted({f for f, _, _ in BUILT}) == sorted(bundlesets.FAMILIES)
    assert len({n for _, n, _ in BUILT}) == len(BUILT) and 35 <= len(BUILT) <= 45
    assert all(2 <= len(st) <= bundlesets.MAX_READS and all(q and len(q) <= bundlesets.MAX_LEN and set(q) <= set("ACGT") for q in st) for _, _, st in BUILT)


def test_the_chunked_scheme_is_the_plain_pass(graphs):
    """score and predecessor of every node, every set, the order shifted by every offset"""
    most_tied, most_rounds = 0, 0
    for _, name, _ in BUILT:
        g = graphs[name]
        for offset in range(CHUNK):
            score, pred, rounds, tied = bundlesets.chunked_pass(g.order, g.in_edges, offset)
            assert score == g.score and pred == g.pred, (name, offset)
            most_tied, most_rounds = max(most_tied, max(tied)), max(most_rounds, max(rounds))
    print("most tied ranks in a chunk", most_tied, "most rounds", most_rounds)
    assert most_rounds == 6


def test_the_walk_back_from_a_unique_heaviest_sink_is_the_consensus(graphs):
    """where the fast path applies (one heaviest node, a sink) the consensus is the walk along pred from it: the scores and predecessors
    compared above are what the result is made of"""
    fast = 0
    for _, name, _ in BUILT:
        g = graphs[name]
        best = max(g.score.values())
        ends = [n for n in g.order if g.score[n] == best]
        if len(ends) == 1 and g.out_deg[ends[0]] == 0:
            fast += 1
            assert "".join(g.rec.node_base[n] for n in g.walk_back(ends[0])) == g.rec.consensus, name
    assert fast >= 30


def test_plain_chains(graphs):
    names = [n for n, _ in of("chain")]
    assert sorted(len(graphs[n].order) for n in names) == sorted(bundlesets.CHAIN_NODES + (230,))
    for n in names:
        g = graphs[n]
        assert g.tied() == [] and all(g.in_edges[m] == [(g.order[r - 1], g.in_edges[m][0][1])] for r, m in enumerate(g.order) if r), n
    g = graphs["nodes_230"]
    assert max(bundlesets.chunked_pass(g.order, g.in_edges)[2]) == 6   # a chunk that is one chain of 64 links: every jumping round


def test_symmetric_bubbles_are_decided_by_position(graphs, built, tmp_path):
    lin, strict = pmrlib.ModesRef(str(tmp_path)), pmrlib.ModesRef(str(tmp_path), mutant="strict_bundle_tie")
    for name, st in of("sym_bubble"):
        g = graphs[name]
        full = [n for n in g.tied() if len({g.score[f] for f in g.top(n)}) == 1]
        assert full and all(g.pred[n] == g.top(n)[-1] for n in full), name       # the later in-edge wins a full tie
        assert any(n in g.walk_back(max(g.order, key=lambda m: g.score[m])) for n in full), name
        assert lin.consensus(st) == g.rec.consensus != strict.consensus(st), name


def test_asymmetric_bubbles_are_decided_by_score_against_position(graphs):
    for name, _ in of("asym_bubble"):
        g = graphs[name]
        hit = [n for n in g.tied() if g.score[g.top(n)[0]] > max(g.score[f] for f in g.top(n)[1:])]
        assert hit and all(g.pred[n] == g.top(n)[0] for n in hit), name
        assert any(n in g.walk_back(max(g.order, key=lambda m: g.score[m])) for n in hit), name


def boundary_counts(g, offset):
    """for the order shifted by `offset`: tied ranks with a maximal in-edge from before their chunk, from inside it, with both; tied ranks
    that have another tied rank of the same chunk among their chosen ancestors"""
    chunk = {n: (r + offset) // CHUNK for n, r in zip(range(len(g.rank)), g.rank)}
    tied = set(g.tied())
    before = inside = both = chained = 0
    for n in tied:
        b = any(chunk[f] < chunk[n] for f in g.top(n))
        i = any(chunk[f] == chunk[n] for f in g.top(n))
        before, inside, both = before + b, inside + i, both + (b and i)
        a = g.pred[n]
        while a != -1 and chunk[a] == chunk[n] and a not in tied:
            a = g.pred[a]
        chained += a != -1 and chunk[a] == chunk[n]
    return before, inside, both, chained


def test_bubble_runs_put_tied_ranks_on_every_side_of_every_boundary(graphs):
    before_offsets, split_offsets = set(), set()
    for name, st in of("bubble_run"):
        g = graphs[name]
        assert len(g.order) >= 200 and len(g.tied()) >= len(st[0]) // 12, name
        for offset in range(CHUNK):
            before, inside, both, chained = boundary_counts(g, offset)
            assert inside >= 1 and chained >= 1, (name, offset)
            if before > both:
                before_offsets.add(offset)
            if both:
                split_offsets.add(offset)
        print(name, len(g.order), "nodes", len(g.tied()), "tied", max(bundlesets.chunked_pass(g.order, g.in_edges)[3]), "at most per chunk")
    # a tied rank all of whose maximal in-edges come from before its chunk, and one whose maximal in-edges come from both sides of the chunk's
    # first rank, whatever that rank is modulo 64 (a bubble puts either at one rank: over the family's sets, not in each of them)
    assert before_offsets == set(range(CHUNK)) and split_offsets == set(range(CHUNK))


def test_wide_rows_share_their_maximal_weight_beyond_the_fourth_in_edge(graphs):
    decided_late = 0
    for name, _ in of("wide_row"):
        g = graphs[name]
        wide = [n for n in g.order if len(g.in_edges[n]) > 4]
        hit = [n for n in wide if len(g.top(n)) > 1 and any(w == max(w for _, w in g.in_edges[n]) for _, w in g.in_edges[n][4:])]
        assert hit, name
        decided_late += any(g.pred[n] in [f for f, _ in g.in_edges[n][4:]] and g.pred[n] not in [f for f, _ in g.in_edges[n][:4]] for n in hit)
    assert decided_late >= 3   # ... and in some of them an entry beyond the fourth is the one that wins


def test_mid_order_sources(graphs):
    for name, _ in of("mid_source"):
        g = graphs[name]
        roots = [g.rank[n] for n in g.order if not g.in_edges[n]]
        print(name, "ranks without in-edges", roots)
        assert len(roots) >= 2 and any(0 < r < len(g.order) - 1 for r in roots), (name, roots)
        assert all(g.score[n] == -1 and g.pred[n] == -1 for n in g.order if not g.in_edges[n])
        # a node right behind such a root scores its weight - 1
        assert any(g.score[n] == w - 1 for n in g.order for f, w in g.in_edges[n][:1] if len(g.in_edges[n]) == 1 and not g.in_edges[f]), name


def test_fallback_paths(graphs):
    for name, _ in of("fallback"):
        g = graphs[name]
        best = max(g.score.values())
        ends = [n for n in g.order if g.score[n] == best]
        if name.startswith("inner_max"):
            assert len(ends) == 1 and g.out_deg[ends[0]] > 0, name      # the branch completion goes on from it
        else:
            assert len(ends) >= 2, name                                   # the reference takes the first in ITS order
