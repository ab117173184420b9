// poa_weighted_ref.cpp — CPU restatement of a POA graph under per-base weights, and of the coverage of its consensus (spoa's
// add_alignment with weights and generate_consensus(dst)), as DESIGN.md "General POA path" states them under "Base weights and coverage".
// The DP, the graph, the rank order, the node derivation and the consensus walks are the existing restatements', taken by inclusion
// (tests/poa_msa_ref.cpp, which includes the affine and the linear one). Graph::add_alignment there adds 2 per edge, so the weights are
// applied beside it: for consecutive bases i-1 and i of a sequence the edge path[i-1] -> path[i] (path from derive_path) gains
// w[i-1] + w[i] - 2, and Graph::consensus() / consensus_nodes() then run on the weighted edges (scores in int64). Coverage and profile
// follow the literal rule - per node the sequences of two or more bases that pass through it, summed over the node and its aligned nodes -
// not the columns. The tests compile this file with g++ and load it through ctypes (tests/wgtlib.py).
//
//   pwr_weighted(seqs, weights, n, m, x, g, e, type)  weights: one array per sequence (a byte per base), or null: all 1. e == g: the
//                                                      linear DP, else the affine one. Returns text, one item per line: the consensus
//                                                      by the walk that yields the nodes; Graph::consensus(); the coverage per consensus
//                                                      base; the profile (four counts per base: A C G T); per consensus base the number
//                                                      of sequences of >= 2 bases through the consensus node itself; the column of every
//                                                      consensus base (the MSA restatement's serial walk); flags: checks that FAILED,
//                                                      as bits (0 = all hold).
//   pwr_free(p)                                        frees it
#include "poa_msa_ref.cpp"

namespace {

enum {
    W_EDGE = 1,    // two consecutive bases' nodes are not joined by a graph edge (no edge to weigh)
    W_TWICE = 2,   // a sequence passes through a node twice
    W_LETTER = 4,  // a node does not hold the letter of the base that went to it
};

std::string join(const std::vector<uint64_t>& v) {
    std::string s;
    for (size_t i = 0; i < v.size(); i++) { if (i) s += ' '; s += std::to_string(v[i]); }
    return s;
}

}  // namespace

extern "C" char* pwr_weighted(const char* const* seqs, const uint8_t* const* weights, uint32_t n, int32_t m, int32_t x, int32_t g, int32_t e, int32_t type) {
    Graph G;
    uint64_t cells = 0;
    uint32_t flags = 0;
    std::vector<std::vector<uint32_t>> paths(n);
    std::vector<uint8_t> s;
    for (uint32_t k = 0; k < n; k++) {
        const size_t L = strlen(seqs[k]);
        if (L == 0) continue;
        s.resize(L);
        for (size_t i = 0; i < L; i++) s[i] = read_code(seqs[k][i]);
        const std::vector<std::pair<int32_t, int32_t>> aln = e == g ? align(G, s.data(), (uint32_t)L, m, x, g, type, &cells) : align_affine(G, s.data(), (uint32_t)L, m, x, g, e, type, &cells).aln;
        uint32_t n_after = 0;
        paths[k] = derive_path(G, aln, s.data(), (uint32_t)L, &n_after);
        G.add_alignment(aln, s.data(), (uint32_t)L);   // (2 per edge, and the rank order; the order does not look at weights)
        for (size_t i = 0; i < L; i++) if (paths[k][i] >= G.code.size() || G.code[paths[k][i]] != s[i]) flags |= W_LETTER;
        if (weights && weights[k])
            for (size_t i = 1; i < L; i++) {
                bool found = false;
                if (paths[k][i - 1] < G.code.size())
                    for (uint32_t ed : G.outs[paths[k][i - 1]])
                        if (G.edges[ed].to == paths[k][i]) { G.edges[ed].w += (int64_t)weights[k][i - 1] + (int64_t)weights[k][i] - 2; found = true; break; }
                if (!found) flags |= W_EDGE;
            }
    }
    const size_t V = G.code.size();
    // per node: the sequences of two or more bases that pass through it (spoa: the sequence labels on the node's edges; a sequence of one
    // base has no edge)
    std::vector<uint64_t> through(V, 0);
    for (uint32_t k = 0; k < n; k++) {
        if (paths[k].size() < 2) continue;
        std::vector<uint32_t> seen(paths[k]);
        std::sort(seen.begin(), seen.end());
        if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) flags |= W_TWICE;
        for (uint32_t nd : paths[k]) if (nd < V) through[nd]++;
    }
    // columns, for the test's comparison with the MSA restatement's rows: the serial walk of pma_msa
    std::vector<uint32_t> col(V, 0);
    {
        uint32_t n_cols = 0;
        for (size_t i = 0; i < V; n_cols++) {
            const uint32_t nd = G.rank2node[i++];
            col[nd] = n_cols;
            for (uint32_t a : G.aligned[nd]) { col[a] = n_cols; if (i < V && G.rank2node[i] == a) i++; }
        }
    }
    std::vector<uint32_t> cn;
    std::string walked, own;
    if (V) { cn = consensus_nodes(G); for (uint32_t nd : cn) walked.push_back("ACGT"[G.code[nd]]); own = G.consensus(); }
    std::vector<uint64_t> cov, prof, self, cols;
    for (uint32_t nd : cn) {
        uint64_t c = through[nd], p[4] = {0, 0, 0, 0};
        p[G.code[nd]] += through[nd];   // (a node holds the letter of every base that went to it)
        for (uint32_t a : G.aligned[nd]) { c += through[a]; p[G.code[a]] += through[a]; }
        cov.push_back(c);
        for (int q = 0; q < 4; q++) prof.push_back(p[q]);
        self.push_back(through[nd]);
        cols.push_back(col[nd]);
    }
    const std::string out = walked + "\n" + own + "\n" + join(cov) + "\n" + join(prof) + "\n" + join(self) + "\n" + join(cols) + "\n" + std::to_string(flags) + "\n";
    char* r = (char*)malloc(out.size() + 1);
    memcpy(r, out.c_str(), out.size() + 1);
    return r;
}

extern "C" void pwr_free(char* p) { free(p); }
