// poa_convex_ref.cpp — CPU restatement of the POA under two-piece affine ("convex") gap penalties in the three alignment modes (kSW local,
// kNW global, kOV overlap), as DESIGN.md "General POA path" states it under "Convex gaps": a literal, scan-free evaluation of the
// H / F / O / E / Q recurrences on five full (V+1) x (L+1) int32 matrices, and the traceback as a walk with a state (H, F or O) whose
// horizontal gaps are resolved by their length. E and Q are computed and stored here, literally, although the traceback does not read them:
// H is their maximum with the rest. The graph (add_alignment, spoa's topological sort, the heaviest bundle), the node of every base
// (derive_path) and the consensus walk that yields nodes (consensus_nodes) are the existing restatements', taken by inclusion
// (tests/poa_msa_ref.cpp, which includes the affine and the linear one). The tests compile this file with g++ and load it through ctypes
// (tests/cvxlib.py).
//
//   pcr_consensus(seqs, n, sc, type, cells)    sc: the six scores m, x, g, e, q, c. Consensus of the sequences in order (empty ones skipped);
//                                              *cells += sum of V * L
//   pcr_last_alignment(node, pos, cap)         the (node | -1, position | -1) pairs of the last alignment this thread made
//   pcr_last_score()                           H of the end cell of the last alignment this thread made (0 when there was none)
//   pcr_msa(seqs, n, sc, type, include_consensus)  text, one item per line: n_cols, the consensus, then one row per GIVEN sequence (an empty
//                                              one: gaps), then the consensus row when asked for
//   pcr_weighted(seqs, weights, n, sc, type)   weights: one array per sequence (a byte per base), or null: all 1. Text, one item per line:
//                                              the consensus on the weighted edges; the coverage per consensus base; the profile (four
//                                              counts per base: A C G T)
//   pcr_free(p)                                frees any of them
#include "poa_msa_ref.cpp"

namespace {

struct Scores { int32_t m, x, g, e, q, c; };

// the score of a gap of k >= 1 bases
inline int32_t gap_score(const Scores& sc, int64_t k) { return (int32_t)std::max<int64_t>(sc.g + (k - 1) * sc.e, sc.q + (k - 1) * sc.c); }

AffineResult align_convex(const Graph& G, const uint8_t* s, uint32_t L, const Scores& sc, int type, uint64_t* cells) {
    AffineResult res;
    const size_t V = G.code.size(), W = (size_t)L + 1;
    if (V == 0 || L == 0) return res;
    *cells += (uint64_t)V * L;
    const int32_t m = sc.m, x = sc.x, g = sc.g, e = sc.e, q = sc.q, c = sc.c;
    std::vector<uint32_t> node2rank(V);
    for (uint32_t r = 0; r < V; r++) node2rank[G.rank2node[r]] = r;
    std::vector<std::vector<size_t>> P(V + 1);
    for (size_t i = 1; i <= V; i++) {
        const uint32_t n = G.rank2node[i - 1];
        if (G.in[n].empty()) P[i].push_back(0);
        else for (uint32_t ed : G.in[n]) P[i].push_back(node2rank[G.edges[ed].from] + 1);
    }
    const size_t N = (V + 1) * W;
    std::vector<int32_t> H(N), F(N, NEG_INF), O(N, NEG_INF), E(N, NEG_INF), Q(N, NEG_INF);
    H[0] = 0;
    for (size_t j = 1; j < W; j++) {
        if (type == T_NW) { E[j] = g + (int32_t)(j - 1) * e; Q[j] = q + (int32_t)(j - 1) * c; H[j] = std::max(E[j], Q[j]); }
        else H[j] = 0;
    }
    int32_t best = type == T_SW ? 0 : NEG_INF;
    size_t bi = 0, bj = 0;
    bool found = false;
    for (size_t i = 1; i <= V; i++) {
        const uint32_t n = G.rank2node[i - 1];
        const bool sink = G.outs[n].empty();
        if (type == T_NW) {
            int32_t f = NEG_INF, o = NEG_INF;
            for (size_t p : P[i]) {
                f = std::max(f, std::max(H[p * W] + g, F[p * W] + e));
                o = std::max(o, std::max(H[p * W] + q, O[p * W] + c));
            }
            F[i * W] = f; O[i * W] = o; H[i * W] = std::max(f, o);
        } else H[i * W] = 0;
        for (size_t j = 1; j < W; j++) {
            const int32_t sg = G.code[n] == s[j - 1] ? m : x;
            int32_t d = NEG_INF, f = NEG_INF, o = NEG_INF;
            for (size_t p : P[i]) {
                d = std::max(d, H[p * W + j - 1] + sg);
                f = std::max(f, std::max(H[p * W + j] + g, F[p * W + j] + e));
                o = std::max(o, std::max(H[p * W + j] + q, O[p * W + j] + c));
            }
            const int32_t ee = std::max(H[i * W + j - 1] + g, E[i * W + j - 1] + e);
            const int32_t qq = std::max(H[i * W + j - 1] + q, Q[i * W + j - 1] + c);
            int32_t h = std::max(std::max(d, std::max(f, o)), std::max(ee, qq));
            if (type == T_SW) h = std::max(h, 0);
            F[i * W + j] = f; O[i * W + j] = o; E[i * W + j] = ee; Q[i * W + j] = qq; H[i * W + j] = h;
            const bool cand = type == T_SW || (type == T_NW ? sink && j == L : (sink || j == L));
            if (cand && h > best) { best = h; bi = i; bj = j; found = true; }
        }
    }
    if (!found) return res;   // kSW: no cell above 0
    res.score = best;
    size_t i = bi, j = bj;
    enum { SH, SF, SO } st = SH;
    for (;;) {
        const size_t cc = i * W + j;
        if (st == SH) {
            if (type == T_SW ? H[cc] == 0 : type == T_NW ? (i == 0 && j == 0) : (i == 0 || j == 0)) break;
            bool ok = false;
            if (i != 0 && j != 0) {   // rule 1: the first predecessor with a diagonal match
                const int32_t sg = G.code[G.rank2node[i - 1]] == s[j - 1] ? m : x;
                for (size_t p : P[i]) if (H[cc] == H[p * W + j - 1] + sg) { res.aln.emplace_back((int32_t)G.rank2node[i - 1], (int32_t)(j - 1)); i = p; j--; ok = true; break; }
            }
            if (ok) continue;
            if (i != 0 && H[cc] == F[cc]) { st = SF; continue; }   // rule 2
            if (i != 0 && H[cc] == O[cc]) { st = SO; continue; }   // rule 3
            size_t k = 1;                                          // rule 4: a horizontal gap, by its length
            while (k <= j && H[cc] != H[cc - k] + gap_score(sc, (int64_t)k)) k++;
            if (k > j) break;   // (cannot happen on a consistent matrix)
            for (size_t d = 1; d <= k; d++) res.aln.emplace_back(-1, (int32_t)(j - d));
            j -= k;
        } else {
            const std::vector<int32_t>& M = st == SF ? F : O;
            const int32_t op = st == SF ? g : q, ex = st == SF ? e : c;
            bool ok = false;
            for (size_t p : P[i]) {
                const bool open = M[cc] == H[p * W + j] + op;
                if (open || M[cc] == M[p * W + j] + ex) { res.aln.emplace_back((int32_t)G.rank2node[i - 1], -1); i = p; if (open) st = SH; ok = true; break; }
            }
            if (!ok) break;   // (cannot happen on a consistent matrix)
        }
    }
    std::reverse(res.aln.begin(), res.aln.end());
    return res;
}

thread_local AffineResult t_last_convex;

// the graph of a set under convex scores, the node of every base, and (weights given) the weighted edges
struct Built { Graph G; std::vector<std::vector<uint32_t>> paths; uint64_t cells = 0; uint32_t non_empty = 0; };

void build(Built& B, const char* const* seqs, const uint8_t* const* weights, uint32_t n, const Scores& sc, int type) {
    B.paths.assign(n, {});
    std::vector<uint8_t> s;
    t_last_convex = AffineResult();
    for (uint32_t k = 0; k < n; k++) {
        const size_t L = strlen(seqs[k]);
        if (L == 0) continue;
        s.resize(L);
        for (size_t i = 0; i < L; i++) s[i] = read_code(seqs[k][i]);
        t_last_convex = align_convex(B.G, s.data(), (uint32_t)L, sc, type, &B.cells);
        uint32_t n_after = 0;
        B.paths[k] = derive_path(B.G, t_last_convex.aln, s.data(), (uint32_t)L, &n_after);
        B.G.add_alignment(t_last_convex.aln, s.data(), (uint32_t)L);
        B.non_empty++;
        if (weights && weights[k])
            for (size_t i = 1; i < L; i++)
                for (uint32_t ed : B.G.outs[B.paths[k][i - 1]])
                    if (B.G.edges[ed].to == B.paths[k][i]) { B.G.edges[ed].w += (int64_t)weights[k][i - 1] + (int64_t)weights[k][i] - 2; break; }
    }
}

char* text(const std::string& out) {
    char* r = (char*)malloc(out.size() + 1);
    memcpy(r, out.c_str(), out.size() + 1);
    return r;
}

std::string ints(const std::vector<uint64_t>& v) {
    std::string s;
    for (size_t i = 0; i < v.size(); i++) { if (i) s += ' '; s += std::to_string(v[i]); }
    return s;
}

}  // namespace

extern "C" char* pcr_consensus(const char* const* seqs, uint32_t n, const int32_t* sc6, int32_t type, uint64_t* cells) {
    Built B;
    build(B, seqs, nullptr, n, Scores{sc6[0], sc6[1], sc6[2], sc6[3], sc6[4], sc6[5]}, type);
    if (cells) *cells += B.cells;
    return text(B.non_empty ? B.G.consensus() : std::string());
}

extern "C" int32_t pcr_last_alignment(int32_t* node, int32_t* pos, int32_t cap) {
    const int32_t n = (int32_t)t_last_convex.aln.size();
    for (int32_t k = 0; k < n && k < cap; k++) { node[k] = t_last_convex.aln[k].first; pos[k] = t_last_convex.aln[k].second; }
    return n;
}

extern "C" int32_t pcr_last_score(void) { return t_last_convex.score; }

extern "C" char* pcr_msa(const char* const* seqs, uint32_t n, const int32_t* sc6, int32_t type, int32_t include_consensus) {
    Built B;
    build(B, seqs, nullptr, n, Scores{sc6[0], sc6[1], sc6[2], sc6[3], sc6[4], sc6[5]}, type);
    const Graph& G = B.G;
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
    std::string out = std::to_string(n_cols) + "\n" + (V ? G.consensus() : std::string()) + "\n";
    for (uint32_t k = 0; k < n; k++) {
        std::string row(n_cols, '-');
        for (size_t i = 0; i < B.paths[k].size(); i++) row[col[B.paths[k][i]]] = "ACGT"[read_code(seqs[k][i])];
        out += row + "\n";
    }
    if (include_consensus) {
        std::string row(n_cols, '-');
        for (uint32_t nd : cn) row[col[nd]] = "ACGT"[G.code[nd]];
        out += row + "\n";
    }
    return text(out);
}

extern "C" char* pcr_weighted(const char* const* seqs, const uint8_t* const* weights, uint32_t n, const int32_t* sc6, int32_t type) {
    Built B;
    build(B, seqs, weights, n, Scores{sc6[0], sc6[1], sc6[2], sc6[3], sc6[4], sc6[5]}, type);
    const Graph& G = B.G;
    const size_t V = G.code.size();
    // per node: the sequences of two or more bases that pass through it (spoa: the sequence labels on the node's edges)
    std::vector<uint64_t> through(V, 0);
    for (uint32_t k = 0; k < n; k++) if (B.paths[k].size() >= 2) for (uint32_t nd : B.paths[k]) through[nd]++;
    std::vector<uint32_t> cn;
    if (V) cn = consensus_nodes(G);
    std::vector<uint64_t> cov, prof;
    for (uint32_t nd : cn) {
        uint64_t c = through[nd], p[4] = {0, 0, 0, 0};
        p[G.code[nd]] += through[nd];
        for (uint32_t a : G.aligned[nd]) { c += through[a]; p[G.code[a]] += through[a]; }
        cov.push_back(c);
        for (int q = 0; q < 4; q++) prof.push_back(p[q]);
    }
    return text((V ? G.consensus() : std::string()) + "\n" + ints(cov) + "\n" + ints(prof) + "\n");
}

extern "C" void pcr_free(char* p) { free(p); }
