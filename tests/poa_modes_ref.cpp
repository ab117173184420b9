// poa_modes_ref.cpp — self-contained CPU restatement of spoa's linear-gap POA in its three alignment modes (kSW local, kNW global,
// kOV overlap), as DESIGN.md "General POA path" states them: graph, add_alignment (unit weights), topological sort, the full
// (V+1) x (L+1) int32 DP, the traceback and the heaviest-bundle consensus. The tests compile it with g++ and load it through ctypes;
// it lives under tests/ because oracle/ does not change. Under kNW it computes what oracle/oracle.cpp's restatement computes.
//
//   pmr_consensus(seqs, n, m, x, g, type, cells)   consensus of the sequences in order (empty ones skipped); *cells += sum of V * L
//   pmr_last_alignment(node, pos, cap)              the (node | -1, position | -1) pairs of the last alignment this thread made
//   pmr_free(p)                                     frees a consensus
//   pmr_last_stats(out7)                            what the last pmr_consensus of this thread met: [alignments whose best end cell is tied, the most
//                                                   tied end cells, ties of more than 8, kNW ties whose closure U (the candidates' columns and everything
//                                                   downstream of them, as kernels/poa.hip's tie shortcut and the oracle's ORC_POA_TIES statistic build it)
//                                                   holds more than 32 nodes, the largest in-degree and the nodes with more than 4 in-edges of the final
//                                                   graph, the most sinks an alignment saw]
// PMR_MUTANT (compile time, tests only) breaks ONE tie-break rule, so that a test can show that its inputs tell the rules apart: 1 the LAST best end
// cell instead of the first, 2 vertical before diagonal in the traceback, 3 horizontal first, 4 the LAST matching predecessor instead of the first,
// 5 `<` instead of `<=` in the heaviest-bundle tie.
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#ifndef PMR_MUTANT
#define PMR_MUTANT 0
#endif

namespace {

// a letter as every entry point reads it: A C G T in either case are 0 1 2 3, anything else is 0 (the reference's table, Compressed_sequence.cpp:10-19, with "& 3")
inline uint8_t read_code(char c) { return c == 'C' || c == 'c' ? 1 : c == 'G' || c == 'g' ? 2 : c == 'T' || c == 't' ? 3 : 0; }

struct Stats { uint64_t tied = 0, max_cand = 0, ties_gt8 = 0, closure_gt32 = 0, max_indeg = 0, wide_rows = 0, max_sinks = 0; };
thread_local Stats t_stats;

enum { T_SW = 0, T_NW = 1, T_OV = 2 };
constexpr int32_t NEG_INF = INT32_MIN / 2;

struct Graph {
    struct Edge { uint32_t from, to; int64_t w; };
    std::vector<uint8_t> code;
    std::vector<std::vector<uint32_t>> in, outs, aligned;
    std::vector<Edge> edges;
    std::vector<uint32_t> rank2node;

    uint32_t add_node(uint8_t c) { code.push_back(c); in.emplace_back(); outs.emplace_back(); aligned.emplace_back(); return (uint32_t)code.size() - 1; }
    void add_edge(uint32_t f, uint32_t t, int64_t w) {
        for (uint32_t e : outs[f]) if (edges[e].to == t) { edges[e].w += w; return; }
        edges.push_back({f, t, w});
        outs[f].push_back((uint32_t)edges.size() - 1);
        in[t].push_back((uint32_t)edges.size() - 1);
    }
    int32_t add_chain(const uint8_t* s, uint32_t b, uint32_t e) {
        if (b == e) return -1;
        const uint32_t first = add_node(s[b]);
        for (uint32_t i = b + 1; i < e; i++) { const uint32_t n = add_node(s[i]); add_edge(n - 1, n, 2); }
        return (int32_t)first;
    }
    // spoa Graph::topological_sort
    void toposort() {
        const size_t V = code.size();
        rank2node.clear();
        std::vector<uint8_t> mark(V, 0);
        std::vector<char> check(V, 1);
        std::vector<uint32_t> st;
        for (uint32_t i = 0; i < V; i++) {
            if (mark[i]) continue;
            st.push_back(i);
            while (!st.empty()) {
                const uint32_t n = st.back();
                bool valid = true;
                if (mark[n] != 2) {
                    for (uint32_t e : in[n]) if (mark[edges[e].from] != 2) { st.push_back(edges[e].from); valid = false; }
                    if (check[n]) for (uint32_t a : aligned[n]) if (mark[a] != 2) { st.push_back(a); check[a] = 0; valid = false; }
                    if (valid) {
                        mark[n] = 2;
                        if (check[n]) { rank2node.push_back(n); for (uint32_t a : aligned[n]) rank2node.push_back(a); }
                    } else mark[n] = 1;
                }
                if (valid) st.pop_back();
            }
        }
    }
    // spoa Graph::add_alignment with unit weights. An alignment that holds no sequence position counts as empty (the whole sequence
    // becomes a new chain): spoa leaves that case undefined.
    void add_alignment(const std::vector<std::pair<int32_t, int32_t>>& aln, const uint8_t* s, uint32_t len) {
        if (len == 0) return;
        std::vector<uint32_t> valid;
        for (auto& p : aln) if (p.second != -1) valid.push_back((uint32_t)p.second);
        if (valid.empty()) { add_chain(s, 0, len); toposort(); return; }
        const uint32_t before = (uint32_t)code.size();
        add_chain(s, 0, valid.front());
        int32_t head = before == code.size() ? -1 : (int32_t)code.size() - 1;
        const int32_t tail = add_chain(s, valid.back() + 1, len);
        for (auto& p : aln) {
            if (p.second == -1) continue;
            const uint8_t c = s[p.second];
            int32_t nn;
            if (p.first == -1) nn = (int32_t)add_node(c);
            else if (code[p.first] == c) nn = p.first;
            else {
                int32_t hit = -1;
                for (uint32_t a : aligned[p.first]) if (code[a] == c) { hit = (int32_t)a; break; }
                if (hit == -1) {
                    nn = (int32_t)add_node(c);
                    for (uint32_t a : aligned[p.first]) { aligned[nn].push_back(a); aligned[a].push_back(nn); }
                    aligned[nn].push_back(p.first);
                    aligned[p.first].push_back(nn);
                } else nn = hit;
            }
            if (head != -1) add_edge(head, nn, 2);
            head = nn;
        }
        if (tail != -1) add_edge(head, tail, 2);
        toposort();
    }
    // spoa Graph::traverse_heaviest_bundle + branch_completion
    std::string consensus() const {
        const size_t V = code.size();
        std::vector<int32_t> pred(V, -1);
        std::vector<int64_t> score(V, -1);
        uint32_t best = 0;
        auto relax = [&](uint32_t n, bool skip_dead) {
            for (uint32_t e : in[n]) {
                const uint32_t f = edges[e].from;
                if (skip_dead && score[f] == -1) continue;
                if (score[n] < edges[e].w || (score[n] == edges[e].w && (PMR_MUTANT == 5 ? score[pred[n]] < score[f] : score[pred[n]] <= score[f]))) { score[n] = edges[e].w; pred[n] = (int32_t)f; }
            }
            if (pred[n] != -1) score[n] += score[pred[n]];
        };
        for (uint32_t n : rank2node) { relax(n, false); if (score[best] < score[n]) best = n; }
        if (!outs[best].empty()) {
            std::vector<uint32_t> rank(V, 0);
            for (uint32_t i = 0; i < rank2node.size(); i++) rank[rank2node[i]] = i;
            while (!outs[best].empty()) {
                const uint32_t n0 = best;
                for (uint32_t e : outs[n0]) for (uint32_t oe : in[edges[e].to]) if (edges[oe].from != n0) score[edges[oe].from] = -1;
                int64_t mx = 0; uint32_t mxid = 0;
                for (uint32_t i = rank[n0] + 1; i < rank2node.size(); i++) {
                    const uint32_t n = rank2node[i];
                    score[n] = -1; pred[n] = -1;
                    relax(n, true);
                    if (mx < score[n]) { mx = score[n]; mxid = n; }
                }
                best = mxid;
            }
        }
        std::string out;
        for (;;) { out.push_back("ACGT"[code[best]]); if (pred[best] == -1) break; best = (uint32_t)pred[best]; }
        std::reverse(out.begin(), out.end());
        return out;
    }
};

// the tie shortcut's set U for the candidate nodes of a kNW end-node tie: their columns (a node and its aligned mates) and everything downstream, closed
// under out-edges and aligned mates (growth stops past 4096 nodes, as in the oracle's statistic)
size_t tie_closure(const Graph& G, const std::vector<uint32_t>& cand) {
    std::vector<uint32_t> U;
    std::vector<char> in_u(G.code.size(), 0);
    auto addcol = [&](uint32_t x) {
        if (in_u[x]) return;
        in_u[x] = 1; U.push_back(x);
        for (uint32_t a : G.aligned[x]) if (!in_u[a]) { in_u[a] = 1; U.push_back(a); }
    };
    for (uint32_t c : cand) addcol(c);
    for (size_t q = 0; q < U.size() && U.size() <= 4096; q++) for (uint32_t e : G.outs[U[q]]) addcol(G.edges[e].to);
    return U.size();
}

// the DP and traceback of one sequence against the graph in its current rank order; returns spoa's (node | -1, pos | -1) pairs, in order
std::vector<std::pair<int32_t, int32_t>> align(const Graph& G, const uint8_t* s, uint32_t L, int32_t m, int32_t x, int32_t g, int type, uint64_t* cells) {
    std::vector<std::pair<int32_t, int32_t>> aln;
    const size_t V = G.code.size(), W = (size_t)L + 1;
    if (V == 0 || L == 0) return aln;
    *cells += (uint64_t)V * L;
    std::vector<uint32_t> node2rank(V);
    for (uint32_t r = 0; r < V; r++) node2rank[G.rank2node[r]] = r;
    // P(r): rows of the in-edge sources in in-edge order, {0} without in-edges
    std::vector<std::vector<size_t>> P(V + 1);
    for (size_t i = 1; i <= V; i++) {
        const uint32_t n = G.rank2node[i - 1];
        if (G.in[n].empty()) P[i].push_back(0);
        else for (uint32_t e : G.in[n]) P[i].push_back(node2rank[G.edges[e].from] + 1);
    }
    std::vector<int32_t> H((V + 1) * W);
    H[0] = 0;
    for (size_t j = 1; j < W; j++) H[j] = type == T_NW ? (int32_t)j * g : 0;
    int32_t best = type == T_SW ? 0 : NEG_INF;
    size_t bi = 0, bj = 0;
    bool found = false;
    std::vector<uint32_t> tied;   // (statistics: the nodes of the candidate end cells that hold the best score so far)
    uint64_t sinks = 0;
    for (size_t i = 1; i <= V; i++) {
        const uint32_t n = G.rank2node[i - 1];
        const bool sink = G.outs[n].empty();
        sinks += sink;
        int32_t* row = &H[i * W];
        if (type == T_NW) { int32_t b = NEG_INF; for (size_t p : P[i]) b = std::max(b, H[p * W]); row[0] = b + g; }
        else row[0] = 0;
        for (size_t j = 1; j < W; j++) {
            const int32_t sg = G.code[n] == s[j - 1] ? m : x;
            int32_t a = NEG_INF;
            for (size_t p : P[i]) a = std::max(a, std::max(H[p * W + j - 1] + sg, H[p * W + j] + g));
            int32_t h = std::max(a, row[j - 1] + g);
            if (type == T_SW) h = std::max(h, 0);
            row[j] = h;
            const bool cand = type == T_SW || (type == T_NW ? sink && j == L : (sink || j == L));
            if (cand && found && h == best) tied.push_back(n);
            if (cand && (h > best || (PMR_MUTANT == 1 && found && h == best))) { if (h > best) tied.assign(1, n); best = h; bi = i; bj = j; found = true; }
        }
    }
    t_stats.max_sinks = std::max<uint64_t>(t_stats.max_sinks, sinks);
    if (found && tied.size() > 1) {
        t_stats.tied++;
        t_stats.max_cand = std::max<uint64_t>(t_stats.max_cand, tied.size());
        t_stats.ties_gt8 += tied.size() > 8;
        if (type == T_NW) t_stats.closure_gt32 += tie_closure(G, tied) > 32;
    }
    if (!found) return aln;   // kSW: no cell above 0
    size_t i = bi, j = bj;
    auto go_on = [&]() { return type == T_SW ? H[i * W + j] != 0 : type == T_NW ? !(i == 0 && j == 0) : (i != 0 && j != 0); };
    while (go_on()) {
        const int32_t h = H[i * W + j];
        size_t pi = i, pj = j;
        bool ok = false;
        auto diagonal = [&]() {
            if (ok || i == 0 || j == 0) return;
            const int32_t sg = G.code[G.rank2node[i - 1]] == s[j - 1] ? m : x;
            for (size_t p : P[i]) if (h == H[p * W + j - 1] + sg) { pi = p; pj = j - 1; ok = true; if (PMR_MUTANT != 4) break; }
        };
        auto vertical = [&]() {
            if (ok || i == 0) return;
            for (size_t p : P[i]) if (h == H[p * W + j] + g) { pi = p; pj = j; ok = true; if (PMR_MUTANT != 4) break; }
        };
        if (PMR_MUTANT == 3 && i != 0 && j != 0 && h == H[i * W + j - 1] + g) { pj = j - 1; ok = true; }
        if (PMR_MUTANT == 2) { vertical(); diagonal(); } else { diagonal(); vertical(); }
        if (!ok) { if (j == 0) break; pi = i; pj = j - 1; }   // (horizontal; j = 0 cannot happen on a consistent matrix)
        aln.emplace_back(pi == i ? -1 : (int32_t)G.rank2node[i - 1], pj == j ? -1 : (int32_t)(j - 1));
        i = pi; j = pj;
    }
    std::reverse(aln.begin(), aln.end());
    return aln;
}

thread_local std::vector<std::pair<int32_t, int32_t>> t_last;

}  // namespace

extern "C" char* pmr_consensus(const char* const* seqs, uint32_t n, int32_t m, int32_t x, int32_t g, int32_t type, uint64_t* cells) {
    Graph G;
    uint64_t c = 0;
    uint32_t non_empty = 0;
    std::vector<uint8_t> s;
    t_stats = Stats();
    for (uint32_t k = 0; k < n; k++) {
        const size_t L = strlen(seqs[k]);
        if (L == 0) continue;
        s.resize(L);
        for (size_t i = 0; i < L; i++) s[i] = read_code(seqs[k][i]);
        t_last = align(G, s.data(), (uint32_t)L, m, x, g, type, &c);
        G.add_alignment(t_last, s.data(), (uint32_t)L);
        non_empty++;
    }
    const std::string out = non_empty ? G.consensus() : std::string();
    for (const auto& in : G.in) { t_stats.max_indeg = std::max<uint64_t>(t_stats.max_indeg, in.size()); t_stats.wide_rows += in.size() > 4; }
    if (cells) *cells += c;
    char* r = (char*)malloc(out.size() + 1);
    memcpy(r, out.c_str(), out.size() + 1);
    return r;
}

extern "C" int32_t pmr_last_alignment(int32_t* node, int32_t* pos, int32_t cap) {
    const int32_t n = (int32_t)t_last.size();
    for (int32_t k = 0; k < n && k < cap; k++) { node[k] = t_last[k].first; pos[k] = t_last[k].second; }
    return n;
}

extern "C" void pmr_last_stats(uint64_t* out7) {
    const Stats& t = t_stats;
    const uint64_t v[7] = {t.tied, t.max_cand, t.ties_gt8, t.closure_gt32, t.max_indeg, t.wide_rows, t.max_sinks};
    memcpy(out7, v, sizeof(v));
}

extern "C" void pmr_free(char* p) { free(p); }
