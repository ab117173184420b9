// poa_affine_ref.cpp — CPU restatement of the affine-gap POA in the three alignment modes (kSW local, kNW global, kOV overlap), as
// DESIGN.md "General POA path" states it under "Affine gaps": a literal, scan-free evaluation of the H / F / E recurrences on three full
// (V+1) x (L+1) int32 matrices and the traceback as a walk with a state. The graph (add_alignment with unit weights, spoa's topological
// sort, the heaviest bundle) is the linear restatement's, taken from tests/poa_modes_ref.cpp by inclusion. The tests compile this file
// with g++ and load it through ctypes (tests/parlib.py).
//
//   par_consensus(seqs, n, m, x, g, e, type, cells)  consensus of the sequences in order (empty ones skipped); *cells += sum of V * L
//   par_last_alignment(node, pos, cap)                the (node | -1, position | -1) pairs of the last alignment this thread made
//   par_last_score()                                  H of the end cell of the last alignment this thread made (0 when there was none)
//   par_free(p)                                       frees a consensus
#include "poa_modes_ref.cpp"

namespace {

struct AffineResult { std::vector<std::pair<int32_t, int32_t>> aln; int32_t score = 0; };

AffineResult align_affine(const Graph& G, const uint8_t* s, uint32_t L, int32_t m, int32_t x, int32_t g, int32_t e, int type, uint64_t* cells) {
    AffineResult res;
    const size_t V = G.code.size(), W = (size_t)L + 1;
    if (V == 0 || L == 0) return res;
    *cells += (uint64_t)V * L;
    std::vector<uint32_t> node2rank(V);
    for (uint32_t r = 0; r < V; r++) node2rank[G.rank2node[r]] = r;
    std::vector<std::vector<size_t>> P(V + 1);
    for (size_t i = 1; i <= V; i++) {
        const uint32_t n = G.rank2node[i - 1];
        if (G.in[n].empty()) P[i].push_back(0);
        else for (uint32_t ed : G.in[n]) P[i].push_back(node2rank[G.edges[ed].from] + 1);
    }
    std::vector<int32_t> H((V + 1) * W), F((V + 1) * W, NEG_INF), E((V + 1) * W, NEG_INF);
    H[0] = 0;
    for (size_t j = 1; j < W; j++) {
        if (type == T_NW) H[j] = E[j] = g + (int32_t)(j - 1) * e;
        else H[j] = 0;
    }
    int32_t best = type == T_SW ? 0 : NEG_INF;
    size_t bi = 0, bj = 0;
    bool found = false;
    for (size_t i = 1; i <= V; i++) {
        const uint32_t n = G.rank2node[i - 1];
        const bool sink = G.outs[n].empty();
        if (type == T_NW) {
            int32_t f = NEG_INF;
            for (size_t p : P[i]) f = std::max(f, std::max(H[p * W] + g, F[p * W] + e));
            F[i * W] = H[i * W] = f;
        } else H[i * W] = 0;
        for (size_t j = 1; j < W; j++) {
            const int32_t sg = G.code[n] == s[j - 1] ? m : x;
            int32_t d = NEG_INF, f = NEG_INF;
            for (size_t p : P[i]) {
                d = std::max(d, H[p * W + j - 1] + sg);
                f = std::max(f, std::max(H[p * W + j] + g, F[p * W + j] + e));
            }
            const int32_t ee = std::max(H[i * W + j - 1] + g, E[i * W + j - 1] + e);
            int32_t h = std::max(d, std::max(f, ee));
            if (type == T_SW) h = std::max(h, 0);
            F[i * W + j] = f; E[i * W + j] = ee; H[i * W + j] = h;
            const bool cand = type == T_SW || (type == T_NW ? sink && j == L : (sink || j == L));
            if (cand && h > best) { best = h; bi = i; bj = j; found = true; }
        }
    }
    if (!found) return res;   // kSW: no cell above 0
    res.score = best;
    size_t i = bi, j = bj;
    enum { SH, SF, SE } st = SH;
    for (;;) {
        const size_t c = i * W + j;
        if (st == SH) {
            if (type == T_SW ? H[c] == 0 : type == T_NW ? (i == 0 && j == 0) : (i == 0 || j == 0)) break;
            bool ok = false;
            if (i != 0 && j != 0) {
                const int32_t sg = G.code[G.rank2node[i - 1]] == s[j - 1] ? m : x;
                for (size_t p : P[i]) if (H[c] == H[p * W + j - 1] + sg) { res.aln.emplace_back((int32_t)G.rank2node[i - 1], (int32_t)(j - 1)); i = p; j--; ok = true; break; }
            }
            if (!ok) st = i != 0 && H[c] == F[c] ? SF : SE;
        } else if (st == SF) {
            bool ok = false;
            for (size_t p : P[i]) {
                const bool open = F[c] == H[p * W + j] + g;
                if (open || F[c] == F[p * W + j] + e) { res.aln.emplace_back((int32_t)G.rank2node[i - 1], -1); i = p; st = open ? SH : SF; ok = true; break; }
            }
            if (!ok) break;   // (cannot happen on a consistent matrix)
        } else {
            if (j == 0) break;   // (cannot happen on a consistent matrix)
            res.aln.emplace_back(-1, (int32_t)(j - 1));
            st = E[c] == H[c - 1] + g ? SH : SE;
            j--;
        }
    }
    std::reverse(res.aln.begin(), res.aln.end());
    return res;
}

thread_local AffineResult t_last_affine;

}  // namespace

extern "C" char* par_consensus(const char* const* seqs, uint32_t n, int32_t m, int32_t x, int32_t g, int32_t e, int32_t type, uint64_t* cells) {
    Graph G;
    uint64_t c = 0;
    uint32_t non_empty = 0;
    std::vector<uint8_t> s;
    t_last_affine = AffineResult();
    for (uint32_t k = 0; k < n; k++) {
        const size_t L = strlen(seqs[k]);
        if (L == 0) continue;
        s.resize(L);
        for (size_t i = 0; i < L; i++) s[i] = read_code(seqs[k][i]);
        t_last_affine = align_affine(G, s.data(), (uint32_t)L, m, x, g, e, type, &c);
        G.add_alignment(t_last_affine.aln, s.data(), (uint32_t)L);
        non_empty++;
    }
    const std::string out = non_empty ? G.consensus() : std::string();
    if (cells) *cells += c;
    char* r = (char*)malloc(out.size() + 1);
    memcpy(r, out.c_str(), out.size() + 1);
    return r;
}

extern "C" int32_t par_last_alignment(int32_t* node, int32_t* pos, int32_t cap) {
    const int32_t n = (int32_t)t_last_affine.aln.size();
    for (int32_t k = 0; k < n && k < cap; k++) { node[k] = t_last_affine.aln[k].first; pos[k] = t_last_affine.aln[k].second; }
    return n;
}

extern "C" int32_t par_last_score(void) { return t_last_affine.score; }

extern "C" void par_free(char* p) { free(p); }
