// poa_band_ref.cpp — CPU restatement of adaptive banded alignment on the general POA path, as DESIGN.md "General POA path" states it under
// "Banded alignment": every row of the score matrix owns a window of B = 2w + 1 columns around a centre that follows the best cell of its
// best predecessor; cells outside a row's window are minus infinity; an alignment without a reachable end cell is a band miss, and a set
// that misses is run again from its first sequence with twice the half-width, at last on the full matrix. The recurrences are evaluated
// literally, cell by cell, on windowed matrices (a cell is stored at its column minus its row's first one), and every value at or below
// -2^28 is stored as minus infinity. Everything that is not the DP is the existing restatements', taken by inclusion
// (tests/poa_convex_ref.cpp, which chains down to the MSA, the affine and the linear one): Graph::add_alignment, the topological sort,
// derive_path, consensus_nodes, and the three full-matrix DPs that the last rung runs. The tests compile this file with g++ and load it
// through ctypes (tests/bandlib.py).
//
//   pbr_banded(seqs, weights, n, sc, model, type, band, force_window, include_consensus)
//                  sc: the six scores m, x, g, e, q, c; model 0: the linear DP (gap g), 1: the affine one (g, e), 2: the convex one.
//                  band: the half-width w (0: the full matrix at once). force_window: 1 keeps the windowed DP where the rules send a set
//                  to the full matrix because its longest sequence + 1 fits B (the tests hold the two against each other); a band miss
//                  still escalates. weights: one array per sequence (a byte per base), or null: all 1. Text, one item per line: the
//                  consensus; "cells band_used band_reruns n_cols"; the coverage per consensus base; the profile (four counts per base:
//                  A C G T); then one row per given sequence (an empty one: gaps), then the consensus row when asked for
//   pbr_free(p)    frees it
#include "poa_convex_ref.cpp"

namespace {

constexpr int32_t UNREACHABLE = -(1 << 28);   // a value at or below it is minus infinity
constexpr uint32_t MAX_HALF = 511;            // 2 * 511 + 1 columns are the widest window

inline int32_t sat(int32_t v) { return v <= UNREACHABLE ? NEG_INF : v; }

struct BandResult { std::vector<std::pair<int32_t, int32_t>> aln; bool miss = false; };

// the windowed matrices of one alignment: row i owns the columns [lo[i], hi[i]]
struct Band {
    size_t B = 0;
    std::vector<uint32_t> lo, hi;
    std::vector<int32_t> H, F, O, E, Q;
    bool in(size_t i, int64_t j) const { return j >= (int64_t)lo[i] && j <= (int64_t)hi[i]; }
    int32_t get(const std::vector<int32_t>& M, size_t i, int64_t j) const { return in(i, j) ? M[i * B + (size_t)(j - lo[i])] : NEG_INF; }
    int32_t& at(std::vector<int32_t>& M, size_t i, size_t j) { return M[i * B + (j - lo[i])]; }
};

BandResult align_band(const Graph& G, const uint8_t* s, uint32_t L, const Scores& sc, int model, int type, uint32_t w, uint64_t* cells) {
    BandResult res;
    const size_t V = G.code.size();
    if (V == 0 || L == 0) return res;
    const size_t B = 2 * (size_t)w + 1;
    *cells += (uint64_t)V * std::min<uint64_t>(B, (uint64_t)L + 1);
    const int32_t m = sc.m, x = sc.x, g = sc.g, e = sc.e, q = sc.q, c = sc.c;
    std::vector<uint32_t> node2rank(V);
    for (uint32_t r = 0; r < V; r++) node2rank[G.rank2node[r]] = r;
    std::vector<std::vector<size_t>> P(V + 1);
    for (size_t i = 1; i <= V; i++) {
        const uint32_t n = G.rank2node[i - 1];
        if (G.in[n].empty()) P[i].push_back(0);
        else for (uint32_t ed : G.in[n]) P[i].push_back(node2rank[G.edges[ed].from] + 1);
    }
    Band M;
    M.B = B; M.lo.assign(V + 1, 0); M.hi.assign(V + 1, 0);
    const size_t N = (V + 1) * B;
    M.H.assign(N, NEG_INF); M.F.assign(N, NEG_INF); M.O.assign(N, NEG_INF); M.E.assign(N, NEG_INF); M.Q.assign(N, NEG_INF);
    std::vector<int32_t> rbest(V + 1, NEG_INF);   // best_i
    std::vector<uint32_t> rm(V + 1, 0);           // m_i
    const int64_t lo_max = std::max<int64_t>(0, (int64_t)L + 1 - (int64_t)B);
    auto window = [&](size_t i, uint32_t centre) {
        M.lo[i] = (uint32_t)std::min<int64_t>(std::max<int64_t>((int64_t)centre - (int64_t)w, 0), lo_max);
        M.hi[i] = (uint32_t)std::min<uint64_t>(L, (uint64_t)M.lo[i] + B - 1);
    };
    auto row_best = [&](size_t i, uint32_t centre) {
        rbest[i] = NEG_INF; rm[i] = std::min(centre, L);
        for (size_t j = M.lo[i]; j <= M.hi[i]; j++) { const int32_t h = M.get(M.H, i, (int64_t)j); if (h > UNREACHABLE && h > rbest[i]) { rbest[i] = h; rm[i] = (uint32_t)j; } }
    };
    window(0, 0);
    for (size_t j = M.lo[0]; j <= M.hi[0]; j++) {
        int32_t h = 0;
        if (type == T_NW && j) {
            if (model == 0) h = (int32_t)j * g;
            else {
                const int32_t ee = g + (int32_t)(j - 1) * e;
                M.at(M.E, 0, j) = sat(ee);
                h = ee;
                if (model == 2) { const int32_t qq = q + (int32_t)(j - 1) * c; M.at(M.Q, 0, j) = sat(qq); h = std::max(ee, qq); }
            }
        }
        M.at(M.H, 0, j) = sat(h);
    }
    row_best(0, 0);
    int32_t best = type == T_SW ? 0 : NEG_INF;
    size_t bi = 0, bj = 0;
    bool found = false;
    for (size_t i = 1; i <= V; i++) {
        const uint32_t n = G.rank2node[i - 1];
        const bool sink = G.outs[n].empty();
        size_t ps = P[i][0];
        for (size_t p : P[i]) if (rbest[p] > rbest[ps]) ps = p;   // the predecessor with the largest best, the first among equals
        const uint32_t centre = std::min<uint32_t>(rm[ps] + 1, L);
        window(i, centre);
        for (size_t j = M.lo[i]; j <= M.hi[i]; j++) {
            int32_t h, f = NEG_INF, o = NEG_INF, ee = NEG_INF, qq = NEG_INF;
            if (j == 0 && type != T_NW) h = 0;
            else {
                int32_t d = NEG_INF;
                const int32_t sg = j ? (G.code[n] == s[j - 1] ? m : x) : 0;
                for (size_t p : P[i]) {
                    const int32_t hv = M.get(M.H, p, (int64_t)j);
                    if (j) d = std::max(d, M.get(M.H, p, (int64_t)j - 1) + sg);
                    if (model == 0) f = std::max(f, hv + g);
                    else {
                        f = std::max(f, std::max(hv + g, M.get(M.F, p, (int64_t)j) + e));
                        if (model == 2) o = std::max(o, std::max(hv + q, M.get(M.O, p, (int64_t)j) + c));
                    }
                }
                const int32_t hl = M.get(M.H, i, (int64_t)j - 1);
                if (model == 0) ee = hl + g;
                else {
                    ee = std::max(hl + g, M.get(M.E, i, (int64_t)j - 1) + e);
                    if (model == 2) qq = std::max(hl + q, M.get(M.Q, i, (int64_t)j - 1) + c);
                }
                h = std::max(std::max(d, std::max(f, o)), std::max(ee, qq));
                if (type == T_SW) h = std::max(h, 0);
            }
            h = sat(h);
            M.at(M.H, i, j) = h; M.at(M.F, i, j) = sat(f); M.at(M.O, i, j) = sat(o); M.at(M.E, i, j) = sat(ee); M.at(M.Q, i, j) = sat(qq);
            const bool cand = j >= 1 && (type == T_SW || (type == T_NW ? sink && j == L : (sink || j == L)));
            if (cand && h > UNREACHABLE && h > best) { best = h; bi = i; bj = j; found = true; }
        }
        row_best(i, centre);
    }
    if (!found) { res.miss = type != T_SW; return res; }   // kSW: no cell above 0 is the empty alignment
    // the tracebacks of the three models (tests/poa_modes_ref.cpp, poa_affine_ref.cpp, poa_convex_ref.cpp), reading through the windows: an
    // unreachable neighbour never matches
    size_t i = bi, j = bj;
    auto Hn = [&](size_t r, int64_t cj, int32_t add, int32_t want) { const int32_t v = M.get(M.H, r, cj); return v > UNREACHABLE && want == v + add; };
    auto Mn = [&](const std::vector<int32_t>& X, size_t r, int64_t cj, int32_t add, int32_t want) { const int32_t v = M.get(X, r, cj); return v > UNREACHABLE && want == v + add; };
    if (model == 0) {
        for (;;) {
            const int32_t h = M.get(M.H, i, (int64_t)j);
            if (type == T_SW ? h == 0 : type == T_NW ? (i == 0 && j == 0) : (i == 0 || j == 0)) break;
            size_t pi = i, pj = j;
            bool ok = false;
            if (i != 0 && j != 0) {
                const int32_t sg = G.code[G.rank2node[i - 1]] == s[j - 1] ? m : x;
                for (size_t p : P[i]) if (Hn(p, (int64_t)j - 1, sg, h)) { pi = p; pj = j - 1; ok = true; break; }
            }
            if (!ok && i != 0)
                for (size_t p : P[i]) if (Hn(p, (int64_t)j, g, h)) { pi = p; pj = j; ok = true; break; }
            if (!ok) { if (j == 0 || !M.in(i, (int64_t)j - 1)) break; pi = i; pj = j - 1; }   // (the break cannot happen on a consistent matrix)
            res.aln.emplace_back(pi == i ? -1 : (int32_t)G.rank2node[i - 1], pj == j ? -1 : (int32_t)(j - 1));
            i = pi; j = pj;
        }
    } else {
        enum { SH, SF, SO, SE } st = SH;
        for (;;) {
            const int32_t h = M.get(M.H, i, (int64_t)j);
            if (st == SH) {
                if (type == T_SW ? h == 0 : type == T_NW ? (i == 0 && j == 0) : (i == 0 || j == 0)) break;
                bool ok = false;
                if (i != 0 && j != 0) {
                    const int32_t sg = G.code[G.rank2node[i - 1]] == s[j - 1] ? m : x;
                    for (size_t p : P[i]) if (Hn(p, (int64_t)j - 1, sg, h)) { res.aln.emplace_back((int32_t)G.rank2node[i - 1], (int32_t)(j - 1)); i = p; j--; ok = true; break; }
                }
                if (ok) continue;
                if (i != 0 && h == M.get(M.F, i, (int64_t)j)) { st = SF; continue; }
                if (model == 1) { st = SE; continue; }
                if (i != 0 && h == M.get(M.O, i, (int64_t)j)) { st = SO; continue; }
                size_t k = 1;   // a horizontal gap, by its length, inside the row's window
                while (k <= j && M.in(i, (int64_t)j - (int64_t)k) && !Hn(i, (int64_t)j - (int64_t)k, gap_score(sc, (int64_t)k), h)) k++;
                if (k > j || !M.in(i, (int64_t)j - (int64_t)k)) break;   // (cannot happen on a consistent matrix)
                for (size_t d = 1; d <= k; d++) res.aln.emplace_back(-1, (int32_t)(j - d));
                j -= k;
            } else if (st == SF || st == SO) {
                const std::vector<int32_t>& X = st == SF ? M.F : M.O;
                const int32_t op = st == SF ? g : q, ex = st == SF ? e : c;
                const int32_t cur = M.get(X, i, (int64_t)j);
                bool ok = false;
                for (size_t p : P[i]) {
                    const bool open = Hn(p, (int64_t)j, op, cur);
                    if (open || Mn(X, p, (int64_t)j, ex, cur)) { res.aln.emplace_back((int32_t)G.rank2node[i - 1], -1); i = p; if (open) st = SH; ok = true; break; }
                }
                if (!ok) break;   // (cannot happen on a consistent matrix)
            } else {
                if (j == 0 || !M.in(i, (int64_t)j - 1)) break;   // (cannot happen on a consistent matrix)
                res.aln.emplace_back(-1, (int32_t)(j - 1));
                st = Hn(i, (int64_t)j - 1, g, M.get(M.E, i, (int64_t)j)) ? SH : SE;
                j--;
            }
        }
    }
    std::reverse(res.aln.begin(), res.aln.end());
    return res;
}

// the full matrix: the existing restatement of the model
std::vector<std::pair<int32_t, int32_t>> align_full(const Graph& G, const uint8_t* s, uint32_t L, const Scores& sc, int model, int type, uint64_t* cells) {
    if (model == 2) return align_convex(G, s, L, sc, type, cells).aln;
    if (model == 1) return align_affine(G, s, L, sc.m, sc.x, sc.g, sc.e, type, cells).aln;
    return align(G, s, L, sc.m, sc.x, sc.g, type, cells);
}

struct BandBuilt { Graph G; std::vector<std::vector<uint32_t>> paths; uint64_t cells = 0; };

// one attempt at a set: false when an alignment missed its band
bool attempt(BandBuilt& R, const char* const* seqs, const uint8_t* const* weights, uint32_t n, const Scores& sc, int model, int type, uint32_t w) {
    R = BandBuilt();
    R.paths.assign(n, {});
    std::vector<uint8_t> s;
    for (uint32_t k = 0; k < n; k++) {
        const size_t L = strlen(seqs[k]);
        if (L == 0) continue;
        s.resize(L);
        for (size_t i = 0; i < L; i++) s[i] = read_code(seqs[k][i]);
        std::vector<std::pair<int32_t, int32_t>> aln;
        if (w) {
            BandResult r = align_band(R.G, s.data(), (uint32_t)L, sc, model, type, w, &R.cells);
            if (r.miss) return false;
            aln.swap(r.aln);
        } else aln = align_full(R.G, s.data(), (uint32_t)L, sc, model, type, &R.cells);
        uint32_t n_after = 0;
        R.paths[k] = derive_path(R.G, aln, s.data(), (uint32_t)L, &n_after);
        R.G.add_alignment(aln, s.data(), (uint32_t)L);
        if (weights && weights[k])
            for (size_t i = 1; i < L; i++)
                for (uint32_t ed : R.G.outs[R.paths[k][i - 1]])
                    if (R.G.edges[ed].to == R.paths[k][i]) { R.G.edges[ed].w += (int64_t)weights[k][i - 1] + (int64_t)weights[k][i] - 2; break; }
    }
    return true;
}

}  // namespace

extern "C" char* pbr_banded(const char* const* seqs, const uint8_t* const* weights, uint32_t n, const int32_t* sc6, int32_t model, int32_t type, uint32_t band, int32_t force_window,
                            int32_t include_consensus) {
    const Scores sc{sc6[0], sc6[1], sc6[2], sc6[3], sc6[4], sc6[5]};
    size_t lmax = 0;
    for (uint32_t k = 0; k < n; k++) lmax = std::max(lmax, strlen(seqs[k]));
    BandBuilt R;
    uint32_t w = band, reruns = 0, used = 0;
    for (;;) {
        const bool full = w == 0 || (!force_window && lmax + 1 <= 2 * (size_t)w + 1);
        used = full ? 0 : w;
        if (attempt(R, seqs, weights, n, sc, model, type, used)) break;
        reruns++;
        w = 2 * w <= MAX_HALF ? 2 * w : 0;
    }
    const Graph& G = R.G;
    const size_t V = G.code.size();
    std::vector<uint32_t> col(V, 0);
    uint32_t n_cols = 0;
    for (size_t i = 0; i < V; n_cols++) {
        const uint32_t nd = G.rank2node[i++];
        col[nd] = n_cols;
        for (uint32_t a : G.aligned[nd]) { col[a] = n_cols; if (i < V && G.rank2node[i] == a) i++; }
    }
    std::vector<uint32_t> cn;
    if (V) cn = consensus_nodes(G);
    std::vector<uint64_t> through(V, 0);
    for (uint32_t k = 0; k < n; k++) if (R.paths[k].size() >= 2) for (uint32_t nd : R.paths[k]) through[nd]++;
    std::vector<uint64_t> cov, prof;
    for (uint32_t nd : cn) {
        uint64_t cv = through[nd], p[4] = {0, 0, 0, 0};
        p[G.code[nd]] += through[nd];
        for (uint32_t a : G.aligned[nd]) { cv += through[a]; p[G.code[a]] += through[a]; }
        cov.push_back(cv);
        for (int t = 0; t < 4; t++) prof.push_back(p[t]);
    }
    std::string out = (V ? G.consensus() : std::string()) + "\n" + std::to_string(R.cells) + " " + std::to_string(used) + " " + std::to_string(reruns) + " " + std::to_string(n_cols) + "\n" +
                      ints(cov) + "\n" + ints(prof) + "\n";
    for (uint32_t k = 0; k < n; k++) {
        std::string row(n_cols, '-');
        for (size_t i = 0; i < R.paths[k].size(); i++) row[col[R.paths[k][i]]] = "ACGT"[read_code(seqs[k][i])];
        out += row + "\n";
    }
    if (include_consensus) {
        std::string row(n_cols, '-');
        for (uint32_t nd : cn) row[col[nd]] = "ACGT"[G.code[nd]];
        out += row + "\n";
    }
    return text(out);
}

extern "C" void pbr_free(char* p) { free(p); }
