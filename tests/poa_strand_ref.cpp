// poa_strand_ref.cpp — CPU restatement of strand-ambiguous sets on the general POA path, as DESIGN.md "General POA path" states them under
// "Strand-ambiguous sets": the first non-empty sequence of a set goes in forward; every later one is aligned to the graph as it stands twice,
// as given and reverse-complemented (reversed, every code c replaced by 3 - c), and the orientation with the higher end-cell score is added,
// ties forward; a reversed sequence's weights are reversed with it; rows, coverage and profile see the sequence as it was added. Everything
// it computes with is the existing restatements', taken by inclusion (tests/poa_convex_ref.cpp, which chains down to the MSA, the affine and
// the linear one): the three DPs and tracebacks, Graph::add_alignment, the topological sort, derive_path, consensus_nodes. This file only
// calls them twice per sequence and applies the rule. The tests compile it with g++ and load it through ctypes (tests/strlib.py).
//
//   psr_strand(seqs, weights, n, sc, model, type, include_consensus)
//                  sc: the six scores m, x, g, e, q, c; model 0: the linear DP (gap g), 1: the affine one (g, e), 2: the convex one.
//                  weights: one array per sequence (a byte per base), or null: all 1. Text, one item per line: the consensus; the flags
//                  (0 / 1 per GIVEN sequence); score_fwd; score_rev; "cells third_passes n_cols"; the coverage per consensus base; the
//                  profile (four counts per base: A C G T); then one row per given sequence (an empty one: gaps), then the consensus row
//                  when asked for
//   psr_free(p)    frees it
#include "poa_convex_ref.cpp"

namespace {

AffineResult align_model(const Graph& G, const uint8_t* s, uint32_t L, const Scores& sc, int model, int type, uint64_t* cells) {
    if (model == 2) return align_convex(G, s, L, sc, type, cells);
    if (model == 1) return align_affine(G, s, L, sc.m, sc.x, sc.g, sc.e, type, cells);
    // the linear restatement returns no score: the end cell's is the affine recurrences' with e = g (the same maximum, whatever the ties)
    AffineResult r;
    uint64_t unused = 0;
    r.aln = align(G, s, L, sc.m, sc.x, sc.g, type, cells);
    r.score = align_affine(G, s, L, sc.m, sc.x, sc.g, sc.g, type, &unused).score;
    return r;
}

std::string sints(const std::vector<int64_t>& v) {
    std::string s;
    for (size_t i = 0; i < v.size(); i++) { if (i) s += ' '; s += std::to_string(v[i]); }
    return s;
}

}  // namespace

extern "C" char* psr_strand(const char* const* seqs, const uint8_t* const* weights, uint32_t n, const int32_t* sc6, int32_t model, int32_t type, int32_t include_consensus) {
    const Scores sc{sc6[0], sc6[1], sc6[2], sc6[3], sc6[4], sc6[5]};
    Graph G;
    uint64_t cells = 0, third = 0;
    std::vector<std::vector<uint32_t>> paths(n);
    std::vector<std::vector<uint8_t>> added(n);   // the codes of every sequence as it was added
    std::vector<int64_t> flags(n, 0), sf(n, 0), sr(n, 0);
    for (uint32_t k = 0; k < n; k++) {
        const size_t L = strlen(seqs[k]);
        if (L == 0) continue;
        std::vector<uint8_t> s(L), rc(L), w(L, 1), wr(L, 1);
        for (size_t i = 0; i < L; i++) s[i] = read_code(seqs[k][i]);
        for (size_t i = 0; i < L; i++) rc[i] = (uint8_t)(3 - s[L - 1 - i]);
        if (weights && weights[k]) for (size_t i = 0; i < L; i++) { w[i] = weights[k][i]; wr[i] = weights[k][L - 1 - i]; }
        AffineResult r;
        bool rev = false;
        if (!G.code.empty()) {
            const AffineResult f = align_model(G, s.data(), (uint32_t)L, sc, model, type, &cells);
            const AffineResult b = align_model(G, rc.data(), (uint32_t)L, sc, model, type, &cells);
            sf[k] = f.score; sr[k] = b.score;
            rev = !(f.score >= b.score);   // ties go forward
            r = rev ? b : f;
        }
        flags[k] = rev; third += rev;
        const std::vector<uint8_t>& u = rev ? rc : s;
        const std::vector<uint8_t>& uw = rev ? wr : w;
        uint32_t n_after = 0;
        paths[k] = derive_path(G, r.aln, u.data(), (uint32_t)L, &n_after);
        G.add_alignment(r.aln, u.data(), (uint32_t)L);
        for (size_t i = 1; i < L; i++)
            for (uint32_t ed : G.outs[paths[k][i - 1]])
                if (G.edges[ed].to == paths[k][i]) { G.edges[ed].w += (int64_t)uw[i - 1] + (int64_t)uw[i] - 2; break; }
        added[k] = u;
    }
    const size_t V = G.code.size();
    // columns: the serial walk of spoa (the node at a rank opens a column, its aligned nodes follow it directly and share it)
    std::vector<uint32_t> col(V, 0);
    uint32_t n_cols = 0;
    for (size_t i = 0; i < V; n_cols++) {
        const uint32_t nd = G.rank2node[i++];
        col[nd] = n_cols;
        for (uint32_t a : G.aligned[nd]) { col[a] = n_cols; if (i < V && G.rank2node[i] == a) i++; }
    }
    std::vector<uint32_t> cn;
    if (V) cn = consensus_nodes(G);
    // per node: the sequences of two or more bases that pass through it (spoa: the sequence labels on the node's edges)
    std::vector<uint64_t> through(V, 0);
    for (uint32_t k = 0; k < n; k++) if (paths[k].size() >= 2) for (uint32_t nd : paths[k]) through[nd]++;
    std::vector<uint64_t> cov, prof;
    for (uint32_t nd : cn) {
        uint64_t c = through[nd], p[4] = {0, 0, 0, 0};
        p[G.code[nd]] += through[nd];
        for (uint32_t a : G.aligned[nd]) { c += through[a]; p[G.code[a]] += through[a]; }
        cov.push_back(c);
        for (int q = 0; q < 4; q++) prof.push_back(p[q]);
    }
    std::string out = (V ? G.consensus() : std::string()) + "\n" + sints(flags) + "\n" + sints(sf) + "\n" + sints(sr) + "\n" +
                      std::to_string(cells) + " " + std::to_string(third) + " " + std::to_string(n_cols) + "\n" + ints(cov) + "\n" + ints(prof) + "\n";
    for (uint32_t k = 0; k < n; k++) {
        std::string row(n_cols, '-');
        for (size_t i = 0; i < paths[k].size(); i++) row[col[paths[k][i]]] = "ACGT"[added[k][i]];
        out += row + "\n";
    }
    if (include_consensus) {
        std::string row(n_cols, '-');
        for (uint32_t nd : cn) row[col[nd]] = "ACGT"[G.code[nd]];
        out += row + "\n";
    }
    return text(out);
}

extern "C" void psr_free(char* p) { free(p); }
