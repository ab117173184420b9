// poa_msa_ref.cpp — CPU restatement of the multiple sequence alignment of a POA graph (spoa's generate_multiple_sequence_alignment), as
// DESIGN.md "General POA path" states it under "MSA output". The DP, the graph, the rank order and the consensus are the existing
// restatements', taken by inclusion (tests/poa_affine_ref.cpp, which includes tests/poa_modes_ref.cpp). Graph::add_alignment there does
// not record the node of every base, so it is derived beside it, from the graph BEFORE the add and the alignment, in the order
// add_alignment creates nodes: prefix chain, suffix chain, then per pair the given node, the aligned node with the base, or the next new
// id. Columns come from the serial walk over the rank order. The tests compile this file with g++ and load it through ctypes
// (tests/msalib.py).
//
//   pma_msa(seqs, n, m, x, g, e, type, include_consensus)  e == g: the linear DP, else the affine one. Returns text, one item per line:
//                                                           "n_cols flags", the consensus by the restated walk, Graph::consensus(),
//                                                           then one row per GIVEN sequence (an empty one: gaps), then the consensus row
//                                                           when asked for. flags: the checks below that FAILED, as bits (0 = all hold).
//   pma_free(p)                                             frees it
#include "poa_affine_ref.cpp"

namespace {

enum {
    F_LETTER = 1,      // a derived node does not hold its base's letter
    F_EDGE = 2,        // two consecutive bases' nodes are not joined by a graph edge
    F_COUNT = 4,       // the derivation created another number of nodes than add_alignment did
    F_CONTIGUOUS = 8,  // the aligned nodes of a node do not follow it directly in the rank order
    F_RULE = 16,       // "the smallest rank of a group opens a column" gives other columns than the serial walk
    F_RISING = 32,     // columns do not rise strictly along a sequence
};

// the node every base of s goes to when add_alignment(aln, s, len) is applied to G (G as it is BEFORE the add)
std::vector<uint32_t> derive_path(const Graph& G, const std::vector<std::pair<int32_t, int32_t>>& aln, const uint8_t* s, uint32_t len, uint32_t* n_after) {
    std::vector<uint32_t> path(len);
    uint32_t next = (uint32_t)G.code.size();
    std::vector<uint32_t> valid;
    for (auto& p : aln) if (p.second != -1) valid.push_back((uint32_t)p.second);
    if (valid.empty()) { for (uint32_t i = 0; i < len; i++) path[i] = next++; *n_after = next; return path; }
    for (uint32_t i = 0; i < valid.front(); i++) path[i] = next++;          // prefix chain
    for (uint32_t i = valid.back() + 1; i < len; i++) path[i] = next++;     // suffix chain
    for (auto& p : aln) {
        if (p.second == -1) continue;
        const uint8_t c = s[p.second];
        uint32_t nn;
        if (p.first == -1) nn = next++;
        else if (G.code[p.first] == c) nn = (uint32_t)p.first;
        else {
            int32_t hit = -1;
            for (uint32_t a : G.aligned[p.first]) if (G.code[a] == c) { hit = (int32_t)a; break; }
            nn = hit == -1 ? next++ : (uint32_t)hit;
        }
        path[p.second] = nn;
    }
    *n_after = next;
    return path;
}

bool has_edge(const Graph& G, uint32_t f, uint32_t t) {
    for (uint32_t e : G.outs[f]) if (G.edges[e].to == t) return true;
    return false;
}

// Graph::consensus() restated so that it returns the NODES of the consensus (the test compares its letters with Graph::consensus())
std::vector<uint32_t> consensus_nodes(const Graph& G) {
    const size_t V = G.code.size();
    std::vector<int32_t> pred(V, -1);
    std::vector<int64_t> score(V, -1);
    uint32_t best = 0;
    auto relax = [&](uint32_t n, bool skip_dead) {
        for (uint32_t e : G.in[n]) {
            const uint32_t f = G.edges[e].from;
            if (skip_dead && score[f] == -1) continue;
            if (score[n] < G.edges[e].w || (score[n] == G.edges[e].w && score[pred[n]] <= score[f])) { score[n] = G.edges[e].w; pred[n] = (int32_t)f; }
        }
        if (pred[n] != -1) score[n] += score[pred[n]];
    };
    for (uint32_t n : G.rank2node) { relax(n, false); if (score[best] < score[n]) best = n; }
    if (!G.outs[best].empty()) {
        std::vector<uint32_t> rank(V, 0);
        for (uint32_t i = 0; i < G.rank2node.size(); i++) rank[G.rank2node[i]] = i;
        while (!G.outs[best].empty()) {
            const uint32_t n0 = best;
            for (uint32_t e : G.outs[n0]) for (uint32_t oe : G.in[G.edges[e].to]) if (G.edges[oe].from != n0) score[G.edges[oe].from] = -1;
            int64_t mx = 0; uint32_t mxid = 0;
            for (uint32_t i = rank[n0] + 1; i < G.rank2node.size(); i++) {
                const uint32_t n = G.rank2node[i];
                score[n] = -1; pred[n] = -1;
                relax(n, true);
                if (mx < score[n]) { mx = score[n]; mxid = n; }
            }
            best = mxid;
        }
    }
    std::vector<uint32_t> out;
    for (;;) { out.push_back(best); if (pred[best] == -1) break; best = (uint32_t)pred[best]; }
    std::reverse(out.begin(), out.end());
    return out;
}

}  // namespace

extern "C" char* pma_msa(const char* const* seqs, uint32_t n, int32_t m, int32_t x, int32_t g, int32_t e, int32_t type, int32_t include_consensus) {
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
        G.add_alignment(aln, s.data(), (uint32_t)L);
        if (n_after != G.code.size()) flags |= F_COUNT;
        for (size_t i = 0; i < L; i++) {
            if (paths[k][i] >= G.code.size() || G.code[paths[k][i]] != s[i]) { flags |= F_LETTER; continue; }
            if (i && paths[k][i - 1] < G.code.size() && !has_edge(G, paths[k][i - 1], paths[k][i])) flags |= F_EDGE;
        }
    }
    // columns: the serial walk of spoa (the node at a rank opens a column, its aligned nodes follow it directly and share it)
    const size_t V = G.code.size();
    std::vector<uint32_t> col(V, 0);
    uint32_t n_cols = 0;
    for (size_t i = 0; i < V; n_cols++) {
        const uint32_t nd = G.rank2node[i++];
        col[nd] = n_cols;
        for (uint32_t a : G.aligned[nd]) {
            if (i >= V || G.rank2node[i] != a) { flags |= F_CONTIGUOUS; col[a] = n_cols; continue; }
            col[a] = n_cols; i++;
        }
    }
    // the rule without a serial walk: rank r opens a column iff it is the smallest rank of its node and the node's aligned nodes
    {
        std::vector<uint32_t> rank(V, 0);
        for (uint32_t r = 0; r < V; r++) rank[G.rank2node[r]] = r;
        uint32_t opened = 0;
        for (uint32_t r = 0; r < V; r++) {
            const uint32_t nd = G.rank2node[r];
            bool opens = true;
            for (uint32_t a : G.aligned[nd]) if (rank[a] < r) opens = false;
            opened += opens;
            if (opened == 0 || col[nd] != opened - 1) flags |= F_RULE;
        }
        if (opened != n_cols) flags |= F_RULE;
    }
    std::vector<uint32_t> cn;
    std::string walked, own;
    if (V) { cn = consensus_nodes(G); for (uint32_t nd : cn) walked.push_back("ACGT"[G.code[nd]]); own = G.consensus(); }
    std::string out = std::to_string(n_cols) + " " + std::to_string(flags) + "\n" + walked + "\n" + own + "\n";
    auto rising = [&](const std::vector<uint32_t>& nodes) { for (size_t i = 1; i < nodes.size(); i++) if (col[nodes[i]] <= col[nodes[i - 1]]) return false; return true; };
    uint32_t late = 0;
    for (uint32_t k = 0; k < n; k++) {
        std::string row(n_cols, '-');
        if (!rising(paths[k])) late |= F_RISING;
        for (size_t i = 0; i < paths[k].size(); i++) row[col[paths[k][i]]] = "ACGT"[read_code(seqs[k][i])];   // (a row shows what was read: include/haslr_hip.h)
        out += row + "\n";
    }
    if (include_consensus) {
        std::string row(n_cols, '-');
        if (!rising(cn)) late |= F_RISING;
        for (uint32_t nd : cn) row[col[nd]] = "ACGT"[G.code[nd]];
        out += row + "\n";
    }
    if (late) {   // (found after the first line was written: patch the flags in)
        const size_t nl = out.find('\n');
        out = std::to_string(n_cols) + " " + std::to_string(flags | late) + out.substr(nl);
    }
    char* r = (char*)malloc(out.size() + 1);
    memcpy(r, out.c_str(), out.size() + 1);
    return r;
}

extern "C" void pma_free(char* p) { free(p); }
