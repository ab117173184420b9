// poa_graph_ref.cpp — CPU restatement of the graph and alignment output of the general POA path, as DESIGN.md "General POA path" states
// it under "Graph and alignment output": per set the nodes (letter, rank in spoa's topological order, MSA column), the edges in the order
// add_edge first made them (with spoa's weights, under unit or given base weights), the node of every base of every sequence, the
// alignment of every sequence against the graph as it was before the add with the score of its end cell, the consensus and its nodes.
// Everything it computes with is the existing restatements', taken by inclusion (tests/poa_convex_ref.cpp, which chains down to the MSA,
// the affine and the linear one): the three DPs and tracebacks, Graph::add_alignment, the topological sort, derive_path,
// consensus_nodes. This file only records what they produce. The tests compile it with g++ and load it through ctypes (tests/grflib.py).
//
//   pgr_graph(seqs, weights, n, sc, model, type)   sc: the six scores m, x, g, e, q, c; model 0: the linear DP (gap g), 1: the affine one
//                                                  (g, e), 2: the convex one. weights: one array per sequence (a byte per base), or
//                                                  null: all 1. Text, one item per line: the node letters; node_rank; node_col;
//                                                  edge_from; edge_to; edge_w; the consensus; its nodes; "cells n_cols"; then per GIVEN
//                                                  sequence three lines: its path; its alignment as node:pos pairs; "score
//                                                  nodes_before edges_before" (the size of the graph it was aligned to)
//   pgr_replay(seqs, n, aln_off, aln_node, aln_pos)  a fresh graph, the given alignments (sequence k: pairs aln_off[k] .. aln_off[k+1])
//                                                  through Graph::add_alignment in order: the first six lines of pgr_graph
//   pgr_free(p)                                    frees either
#include "poa_convex_ref.cpp"

namespace {

std::string uints(const std::vector<uint32_t>& v) {
    std::string s;
    for (size_t i = 0; i < v.size(); i++) { if (i) s += ' '; s += std::to_string(v[i]); }
    return s;
}

// the first six lines: nodes in id order, edges in creation order
std::string graph_lines(const Graph& G) {
    const size_t V = G.code.size();
    std::string letters;
    for (size_t n = 0; n < V; n++) letters.push_back("ACGT"[G.code[n]]);
    std::vector<uint32_t> rank(V, 0), col(V, 0);
    for (uint32_t r = 0; r < V; r++) rank[G.rank2node[r]] = r;
    // columns: the serial walk of spoa (the node at a rank opens a column, its aligned nodes follow it directly and share it)
    uint32_t n_cols = 0;
    for (size_t i = 0; i < V; n_cols++) {
        const uint32_t nd = G.rank2node[i++];
        col[nd] = n_cols;
        for (uint32_t a : G.aligned[nd]) { col[a] = n_cols; if (i < V && G.rank2node[i] == a) i++; }
    }
    std::string ef, et, ew;
    for (size_t e = 0; e < G.edges.size(); e++) {
        if (e) { ef += ' '; et += ' '; ew += ' '; }
        ef += std::to_string(G.edges[e].from); et += std::to_string(G.edges[e].to); ew += std::to_string(G.edges[e].w);
    }
    return letters + "\n" + uints(rank) + "\n" + uints(col) + "\n" + ef + "\n" + et + "\n" + ew + "\n";
}

uint32_t columns_of(const Graph& G) {
    const size_t V = G.code.size();
    uint32_t n_cols = 0;
    for (size_t i = 0; i < V; n_cols++) {
        const uint32_t nd = G.rank2node[i++];
        for (uint32_t a : G.aligned[nd]) if (i < V && G.rank2node[i] == a) i++;
    }
    return n_cols;
}

}  // namespace

extern "C" char* pgr_graph(const char* const* seqs, const uint8_t* const* weights, uint32_t n, const int32_t* sc6, int32_t model, int32_t type) {
    const Scores sc{sc6[0], sc6[1], sc6[2], sc6[3], sc6[4], sc6[5]};
    Graph G;
    uint64_t cells = 0, unused = 0;
    std::string per_seq;
    std::vector<uint8_t> s;
    uint32_t non_empty = 0;
    for (uint32_t k = 0; k < n; k++) {
        const size_t L = strlen(seqs[k]);
        if (L == 0) { per_seq += "\n\n0 " + std::to_string(G.code.size()) + " " + std::to_string(G.edges.size()) + "\n"; continue; }
        s.resize(L);
        for (size_t i = 0; i < L; i++) s[i] = read_code(seqs[k][i]);
        const size_t v_before = G.code.size(), e_before = G.edges.size();
        AffineResult r;
        if (model == 2) r = align_convex(G, s.data(), (uint32_t)L, sc, type, &cells);
        else if (model == 1) r = align_affine(G, s.data(), (uint32_t)L, sc.m, sc.x, sc.g, sc.e, type, &cells);
        else {
            // the linear restatement returns no score: the end cell's is the affine recurrences' with e = g (the same maximum, whatever the ties)
            r.aln = align(G, s.data(), (uint32_t)L, sc.m, sc.x, sc.g, type, &cells);
            r.score = align_affine(G, s.data(), (uint32_t)L, sc.m, sc.x, sc.g, sc.g, type, &unused).score;
        }
        uint32_t n_after = 0;
        const std::vector<uint32_t> path = derive_path(G, r.aln, s.data(), (uint32_t)L, &n_after);
        G.add_alignment(r.aln, s.data(), (uint32_t)L);
        non_empty++;
        if (weights && weights[k])
            for (size_t i = 1; i < L; i++)
                for (uint32_t ed : G.outs[path[i - 1]])
                    if (G.edges[ed].to == path[i]) { G.edges[ed].w += (int64_t)weights[k][i - 1] + (int64_t)weights[k][i] - 2; break; }
        std::string al;
        for (size_t i = 0; i < r.aln.size(); i++) { if (i) al += ' '; al += std::to_string(r.aln[i].first) + ":" + std::to_string(r.aln[i].second); }
        per_seq += uints(path) + "\n" + al + "\n" + std::to_string(r.score) + " " + std::to_string(v_before) + " " + std::to_string(e_before) + "\n";
    }
    std::vector<uint32_t> cn;
    if (non_empty) cn = consensus_nodes(G);
    return text(graph_lines(G) + (non_empty ? G.consensus() : std::string()) + "\n" + uints(cn) + "\n" + std::to_string(cells) + " " + std::to_string(columns_of(G)) + "\n" + per_seq);
}

extern "C" char* pgr_replay(const char* const* seqs, uint32_t n, const uint64_t* aln_off, const int32_t* aln_node, const int32_t* aln_pos) {
    Graph G;
    std::vector<uint8_t> s;
    for (uint32_t k = 0; k < n; k++) {
        const size_t L = strlen(seqs[k]);
        if (L == 0) continue;
        s.resize(L);
        for (size_t i = 0; i < L; i++) s[i] = read_code(seqs[k][i]);
        std::vector<std::pair<int32_t, int32_t>> aln;
        for (uint64_t p = aln_off[k]; p < aln_off[k + 1]; p++) aln.emplace_back(aln_node[p], aln_pos[p]);
        G.add_alignment(aln, s.data(), (uint32_t)L);
    }
    return text(graph_lines(G));
}

extern "C" void pgr_free(char* p) { free(p); }
