// poa_label_ref.cpp — CPU restatement of per-label consensus over one shared graph on the general POA path, as DESIGN.md "General POA
// path" states it under "Per-label consensus". The graph of a set is built exactly as for a weighted call: labels enter neither the
// alignment nor the graph update, the rank order, the columns or the weights. Per label g the view is restated literally: an edge of the
// view weighs the sum of w[i-1] + w[i] over the label's sequences that walk it, an edge no sequence of the label walks is absent, and
// spoa's heaviest bundle with branch completion runs on the view's in-edges and out-edges alone, falling back to the view's node of
// smallest id where spoa falls back to node 0. Everything that is not the view is the existing restatements', taken by inclusion. The
// weighted restatement proper (tests/poa_weighted_ref.cpp) holds the linear and the affine DP only and its convex sibling lives in
// tests/poa_convex_ref.cpp (pcr_weighted), which chains down to the same MSA, affine and linear restatements; neither file has an
// include guard, so this one includes the convex one, which brings all three DPs. The tests compile this file with g++ and load it through
// ctypes (tests/lbllib.py).
//
//   plr_labelled(seqs, weights, labels, n, n_labels, sc, model, type, include_consensus)
//                  sc: the six scores m, x, g, e, q, c; model 0: the linear DP (gap g), 1: the affine one (g, e), 2: the convex one.
//                  weights: one array per sequence (a byte per base), or null: all 1. labels: a byte per sequence, 0 .. n_labels - 1 or
//                  255. Text, one item per line: "cells n_cols"; per label four lines (the consensus; the column of every consensus base;
//                  its coverage; its profile, four counts per base: A C G T); then one row per given sequence (an empty one: gaps), then
//                  with include_consensus one row per label
//   plr_free(p)    frees it
#include "poa_convex_ref.cpp"

namespace {

constexpr uint32_t NO_NODE = 0xffffffffu;

std::vector<std::pair<int32_t, int32_t>> align_model(const Graph& G, const uint8_t* s, uint32_t L, const Scores& sc, int model, int type, uint64_t* cells) {
    if (model == 2) return align_convex(G, s, L, sc, type, cells).aln;
    if (model == 1) return align_affine(G, s, L, sc.m, sc.x, sc.g, sc.e, type, cells).aln;
    return align(G, s, L, sc.m, sc.x, sc.g, type, cells);
}

// the nodes of label g's consensus: Graph::consensus() (tests/poa_modes_ref.cpp) on the view. vw: the weight of every edge in the view
// (0: absent); lowest: the view's node of smallest id
std::vector<uint32_t> view_consensus(const Graph& G, const std::vector<int64_t>& vw, uint32_t lowest) {
    const size_t V = G.code.size();
    std::vector<int32_t> pred(V, -1);
    std::vector<int64_t> score(V, -1);
    auto relax = [&](uint32_t n, bool skip_dead) {
        for (uint32_t e : G.in[n]) {
            if (vw[e] == 0) continue;
            const uint32_t f = G.edges[e].from;
            if (skip_dead && score[f] == -1) continue;
            if (score[n] < vw[e] || (score[n] == vw[e] && score[pred[n]] <= score[f])) { score[n] = vw[e]; pred[n] = (int32_t)f; }
        }
        if (pred[n] != -1) score[n] += score[pred[n]];
    };
    auto sink = [&](uint32_t n) {
        for (uint32_t e : G.outs[n]) if (vw[e] != 0) return false;
        return true;
    };
    // spoa starts at node 0 and moves to every node that scores strictly more, in rank order: the first maximum above -1, else node 0
    uint32_t best = NO_NODE;
    int64_t top = -1;
    for (uint32_t n : G.rank2node) { relax(n, false); if (top < score[n]) { top = score[n]; best = n; } }
    if (best == NO_NODE) best = lowest;
    std::vector<uint32_t> rank(V, 0);
    for (uint32_t i = 0; i < G.rank2node.size(); i++) rank[G.rank2node[i]] = i;
    for (size_t round = 0; !sink(best) && round <= V; round++) {   // (the bound only guards against a walk that never reaches a sink)
        const uint32_t n0 = best;
        for (uint32_t e : G.outs[n0]) {
            if (vw[e] == 0) continue;
            for (uint32_t oe : G.in[G.edges[e].to]) if (vw[oe] != 0 && G.edges[oe].from != n0) score[G.edges[oe].from] = -1;
        }
        int64_t mx = 0;
        uint32_t mxid = NO_NODE;
        for (uint32_t i = rank[n0] + 1; i < G.rank2node.size(); i++) {
            const uint32_t n = G.rank2node[i];
            score[n] = -1; pred[n] = -1;
            relax(n, true);
            if (mx < score[n]) { mx = score[n]; mxid = n; }
        }
        best = mxid == NO_NODE ? lowest : mxid;
    }
    std::vector<uint32_t> out;
    for (;;) { out.push_back(best); if (pred[best] == -1) break; best = (uint32_t)pred[best]; }
    std::reverse(out.begin(), out.end());
    return out;
}

std::string ints32(const std::vector<uint32_t>& v) {
    std::string s;
    for (size_t i = 0; i < v.size(); i++) { if (i) s += ' '; s += std::to_string(v[i]); }
    return s;
}

}  // namespace

extern "C" char* plr_labelled(const char* const* seqs, const uint8_t* const* weights, const uint8_t* labels, uint32_t n, uint32_t n_labels, const int32_t* sc6, int32_t model, int32_t type,
                              int32_t include_consensus) {
    const Scores sc{sc6[0], sc6[1], sc6[2], sc6[3], sc6[4], sc6[5]};
    Graph G;
    uint64_t cells = 0;
    std::vector<std::vector<uint32_t>> paths(n);
    std::vector<std::vector<uint8_t>> codes(n);
    for (uint32_t k = 0; k < n; k++) {
        const size_t L = strlen(seqs[k]);
        if (L == 0) continue;
        std::vector<uint8_t>& s = codes[k];
        s.resize(L);
        for (size_t i = 0; i < L; i++) s[i] = read_code(seqs[k][i]);
        const std::vector<std::pair<int32_t, int32_t>> aln = align_model(G, s.data(), (uint32_t)L, sc, model, type, &cells);
        uint32_t n_after = 0;
        paths[k] = derive_path(G, aln, s.data(), (uint32_t)L, &n_after);
        G.add_alignment(aln, s.data(), (uint32_t)L);
        if (weights && weights[k])
            for (size_t i = 1; i < L; i++)
                for (uint32_t ed : G.outs[paths[k][i - 1]])
                    if (G.edges[ed].to == paths[k][i]) { G.edges[ed].w += (int64_t)weights[k][i - 1] + (int64_t)weights[k][i] - 2; break; }
    }
    const size_t V = G.code.size();
    std::vector<uint32_t> col(V, 0);
    uint32_t n_cols = 0;
    for (size_t i = 0; i < V; n_cols++) {
        const uint32_t nd = G.rank2node[i++];
        col[nd] = n_cols;
        for (uint32_t a : G.aligned[nd]) { col[a] = n_cols; if (i < V && G.rank2node[i] == a) i++; }
    }
    std::string out = std::to_string(cells) + " " + std::to_string(n_cols) + "\n";
    std::vector<std::string> cns_rows;
    for (uint32_t g = 0; g < n_labels; g++) {
        std::vector<int64_t> vw(G.edges.size(), 0);
        std::vector<uint64_t> cnt(4 * (size_t)n_cols, 0);
        uint32_t lowest = NO_NODE;
        for (uint32_t k = 0; k < n; k++) {
            if (labels[k] != g || paths[k].empty()) continue;
            const std::vector<uint32_t>& p = paths[k];
            for (uint32_t nd : p) lowest = std::min(lowest, nd);
            for (size_t i = 1; i < p.size(); i++)
                for (uint32_t ed : G.outs[p[i - 1]])
                    if (G.edges[ed].to == p[i]) { vw[ed] += (int64_t)(weights && weights[k] ? weights[k][i - 1] : 1) + (int64_t)(weights && weights[k] ? weights[k][i] : 1); break; }
            if (p.size() >= 2) for (size_t i = 0; i < p.size(); i++) cnt[4 * (size_t)col[p[i]] + codes[k][i]]++;
        }
        std::vector<uint32_t> cn;
        if (lowest != NO_NODE) cn = view_consensus(G, vw, lowest);
        std::string cns, row(n_cols, '-');
        std::vector<uint32_t> cols;
        std::vector<uint64_t> cov, prof;
        for (uint32_t nd : cn) {
            cns.push_back("ACGT"[G.code[nd]]);
            cols.push_back(col[nd]);
            row[col[nd]] = "ACGT"[G.code[nd]];
            const uint64_t* c = &cnt[4 * (size_t)col[nd]];
            cov.push_back(c[0] + c[1] + c[2] + c[3]);
            for (int q = 0; q < 4; q++) prof.push_back(c[q]);
        }
        out += cns + "\n" + ints32(cols) + "\n" + ints(cov) + "\n" + ints(prof) + "\n";
        cns_rows.push_back(row);
    }
    for (uint32_t k = 0; k < n; k++) {
        std::string row(n_cols, '-');
        for (size_t i = 0; i < paths[k].size(); i++) row[col[paths[k][i]]] = "ACGT"[codes[k][i]];
        out += row + "\n";
    }
    if (include_consensus) for (const std::string& r : cns_rows) out += r + "\n";
    return text(out);
}

extern "C" void plr_free(char* p) { free(p); }
