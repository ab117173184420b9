// poa_modes_dp.inl - the DP and the traceback of the general POA path (kernels/poa_modes.hip), linear, affine and convex gaps. Included inside that
// file's anonymous namespace, after MArgs, Shared and the MT_* / GM_* types. One row loop, dp_rows<NT, CPL, GM>, for the three gap models: what they
// share (the sq[] packing, the row-record prefetch, the predecessor fold, the column-0 rule, the end-cell reduction) stands once, with `if constexpr`
// where a model has an accumulator more; from "combine the accumulators" to the row's stores each model keeps a block of its own, because there they
// differ in substance (an inclusive prefix maximum, an exclusive one, two exclusive ones). Every instantiation keeps the statements of the three loops
// it replaces in their order, which is what keeps the machine code ("One row loop"). Small helpers (the end-cell test, the
// predecessor-row lookup, the carry) were measured there and cost instructions or registers: they stay spelt out.

// A cell of the matrix by gap model: H (linear); (H, F), the vertical gap beside the score (affine); (H, F, O), 12 bytes, the vertical gap under the
// first and the second piece (convex). E and Q are not stored: a row needs them only in registers, and the tracebacks rebuild what they need.
struct Cell3 { int32_t x, y, z; };   // H, F, O
template <int GM> struct CellOf { using type = int32_t; };
template <> struct CellOf<GM_AFFINE> { using type = int2; };
template <> struct CellOf<GM_CONVEX> { using type = Cell3; };
template <int GM> using Cell = typename CellOf<GM>::type;
// H of a cell, by reference: h_of(hp[j]) loads the one word
__device__ __forceinline__ int32_t h_of(const int32_t& c) { return c; }
__device__ __forceinline__ int32_t h_of(const int2& c) { return c.x; }
__device__ __forceinline__ int32_t h_of(const Cell3& c) { return c.x; }

// DP of sequence s[0, L) against the V rows; returns through *bi / *bj the end cell (bi = 0: none - kSW without a cell above 0).
// Scores: a.g the gap (linear) or the first piece's gap open, a.e its gap extend (g <= e <= 0), a.q / a.c the second piece (q <= c <= 0, q <= g).
template <int NT, int CPL, int GM>
__device__ void dp_rows(const G& g, Cell<GM>* H, const uint32_t V, const uint8_t* s, const uint32_t L, const MArgs& a, Shared& sh, int* s_wtot,
                        uint32_t* bi_out, uint32_t* bj_out) {
    constexpr int NEG2 = -(1 << 30);   // identity of the scans (below every real and every NEG-derived value)
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    const uint32_t W = L + 1, j0 = t * CPL;
    const int32_t m = a.m, n = a.n, go = a.g, ge = a.e, qo = a.q, qe = a.c;
    const int type = a.type;
    uint32_t sq[(CPL + 15) / 16];   // s[j - 1] of the lane's columns, 2 bits each
#pragma unroll
    for (int q = 0; q < (CPL + 15) / 16; q++) sq[q] = 0;
#pragma unroll
    for (int k = 0; k < CPL; k++) { const uint32_t j = j0 + k; if (j >= 1 && j <= L) sq[k >> 4] |= (uint32_t)s[j - 1] << (2 * (k & 15)); }
#pragma unroll
    for (int k = 0; k < CPL; k++) {   // row 0: 0, under kNW a gap of j bases; F = O = -inf
        const uint32_t j = j0 + k;
        if (j <= L) {
            if constexpr (GM == GM_LINEAR) H[j] = type == MT_NW ? (int32_t)j * go : 0;
            else if constexpr (GM == GM_AFFINE) H[j] = make_int2(type == MT_NW && j ? go + ((int32_t)j - 1) * ge : 0, NEG);
            else H[j] = Cell3{type == MT_NW && j ? max(go + ((int32_t)j - 1) * ge, qo + ((int32_t)j - 1) * qe) : 0, NEG, NEG};
        }
    }
    __syncthreads();
    int32_t bv = type == MT_SW ? 0 : NEG;
    uint32_t bi = 0, bj = 0;
    uint32_t meta = g.row_meta[0], off = g.row_pred_off[0];
    for (uint32_t i = 1; i <= V; i++) {
        const uint32_t cmeta = meta, coff = off;
        if (i < V) { meta = g.row_meta[i]; off = g.row_pred_off[i]; }   // the next row's record, while this one runs
        const uint32_t np = cmeta >> META_NP, code = cmeta & 3u;
        const bool sink = (cmeta & 4u) != 0;
        // per column: x the diagonal candidate (linear: and the vertical one), f / o the vertical gap under the first / the second piece
        int32_t x[CPL], f[GM >= GM_AFFINE ? CPL : 1], o[GM == GM_CONVEX ? CPL : 1];
#pragma unroll
        for (int k = 0; k < CPL; k++) {
            x[k] = NEG;
            if constexpr (GM >= GM_AFFINE) f[k] = NEG;
            if constexpr (GM == GM_CONVEX) o[k] = NEG;
        }
        const uint32_t npp = np ? np : 1u;
        for (uint32_t p = 0; p < npp; p++) {
            const uint32_t prow = np ? g.pred_rank[coff + p] + 1u : 0u;
            const Cell<GM>* hp = H + (size_t)prow * W;
            int32_t left = j0 >= 1 && j0 <= W ? h_of(hp[j0 - 1]) : NEG;
#pragma unroll
            for (int k = 0; k < CPL; k++) {
                const uint32_t j = j0 + k;
                if (j <= L) {
                    const Cell<GM> v = hp[j];
                    const int32_t sg = ((sq[k >> 4] >> (2 * (k & 15))) & 3u) == code ? m : n;
                    if constexpr (GM == GM_LINEAR) x[k] = max(x[k], max(left + sg, v + go));
                    else {
                        x[k] = max(x[k], left + sg);
                        f[k] = max(f[k], max(v.x + go, v.y + ge));
                        if constexpr (GM == GM_CONVEX) o[k] = max(o[k], max(v.x + qo, v.z + qe));
                    }
                    left = h_of(v);
                }
            }
        }
        // column 0 of kSW / kOV: H = 0, F = O = -inf (kNW: H[r][0] is the maximum over P(r) of the vertical candidates, which the fold gave)
        if (type != MT_NW && j0 == 0) {
            x[0] = 0;
            if constexpr (GM >= GM_AFFINE) f[0] = NEG;
            if constexpr (GM == GM_CONVEX) o[0] = NEG;
        }
        if constexpr (GM == GM_LINEAR) {
            // horizontal: H[j] = j g + max over k <= j of (x[k] - k g); kSW clamps after the scan (exact: a clamped 0 only ever propagates g < 0)
#pragma unroll
            for (int k = 0; k < CPL; k++) { x[k] -= (int32_t)(j0 + k) * go; if (k) x[k] = max(x[k], x[k - 1]); }
            const int incl = wave_scan_max(x[CPL - 1]);
            int carry = wave_shift_up1(incl, NEG2);
            if (NT > 64) {
                if (lane == 63) s_wtot[w] = incl;
                __syncthreads();
                for (uint32_t q = 0; q < w; q++) carry = max(carry, s_wtot[q]);
            }
            Cell<GM>* row = H + (size_t)i * W;
#pragma unroll
            for (int k = 0; k < CPL; k++) {
                const uint32_t j = j0 + k;
                int32_t h = max(x[k], carry) + (int32_t)j * go;
                if (type == MT_SW) h = max(h, 0);
                if (j <= L) {
                    row[j] = h;
                    const bool cand = j >= 1 && (type == MT_SW || (type == MT_NW ? sink && j == L : sink || j == L));
                    if (cand && h > bv) { bv = h; bi = i; bj = j; }
                }
            }
        } else if constexpr (GM == GM_AFFINE) {
            // With X[k] = max(diagonal, F) of column k (kSW: clamped at 0; column 0: H[r][0]) the horizontal recurrence E[j] = max(H[j-1] + g,
            // E[j-1] + e), H[j] = max(X[j], E[j]) unrolls to E[j] = g + (j-1) e + max over k < j of (X[k] - k e): a term that passes through an
            // E[k] on its way (H[k] = E[k]) pays g where the direct term from the same X[k'] pays e, and g <= e, so it never wins. e = 0 needs
            // nothing else (the argument uses g <= e only), and the kSW clamp commutes with the maximum: max(X[k], E[k], 0) = max(max(X[k], 0),
            // E[k]). So E is the linear path's prefix maximum made exclusive.
#pragma unroll
            for (int k = 0; k < CPL; k++) { x[k] = max(x[k], f[k]); if (type == MT_SW) x[k] = max(x[k], 0); }
            // y[k] = X[k] - j e, its in-lane inclusive prefix maximum, then the exclusive carry of the lanes before
            int32_t y[CPL];
#pragma unroll
            for (int k = 0; k < CPL; k++) { y[k] = x[k] - (int32_t)(j0 + k) * ge; if (k) y[k] = max(y[k], y[k - 1]); }
            const int incl = wave_scan_max(y[CPL - 1]);
            int carry = wave_shift_up1(incl, NEG2);
            if (NT > 64) {
                if (lane == 63) s_wtot[w] = incl;
                __syncthreads();
                for (uint32_t q = 0; q < w; q++) carry = max(carry, s_wtot[q]);
            }
            Cell<GM>* row = H + (size_t)i * W;
#pragma unroll
            for (int k = 0; k < CPL; k++) {
                const uint32_t j = j0 + k;
                const int32_t ex = k ? max(carry, y[k - 1]) : carry;           // max over columns < j of X - k e
                const int32_t h = max(x[k], ex + go + ((int32_t)j - 1) * ge);  // (column 0: ex is the identity, E stays below every real value)
                if (j <= L) {
                    row[j] = make_int2(h, f[k]);
                    const bool cand = j >= 1 && (type == MT_SW || (type == MT_NW ? sink && j == L : sink || j == L));
                    if (cand && h > bv) { bv = h; bi = i; bj = j; }
                }
            }
        } else {
            // A gap of k bases scores w(k) = max(g + (k-1) e, q + (k-1) c). With X[k] = max(diagonal, F, O) of column k (kSW: clamped at 0;
            // column 0: H[r][0]) the recurrences unroll to H[j] = max(X[j], max over k < j of H[k] + w(j-k)), and w(a) + w(b) <= w(a+b) (each
            // piece opens no cheaper than it extends, and q <= g; DESIGN.md has the cases), so a term that passes through another gap on its way
            // never beats the direct one: H[j] = max(X[j], E'[j], Q'[j]) with E'[j] = g + (j-1) e + max over k < j of (X[k] - k e) and Q'[j] =
            // q + (j-1) c + max over k < j of (X[k] - k c), two exclusive prefix maxima over the same X. E' and Q' can lie below the literal E
            // and Q (a gap that changes its piece on the way); their maximum with X cannot, and only H is kept. The scans share the barrier;
            // the in-lane prefixes are rebuilt in the store loop instead of kept in registers.
            int32_t ya = NEG2, za = NEG2;   // per piece the lane's maximum of X[k] - j e
#pragma unroll
            for (int k = 0; k < CPL; k++) {
                x[k] = max(x[k], max(f[k], o[k]));
                if (type == MT_SW) x[k] = max(x[k], 0);
                ya = max(ya, x[k] - (int32_t)(j0 + k) * ge);
                za = max(za, x[k] - (int32_t)(j0 + k) * qe);
            }
            const int incl1 = wave_scan_max(ya), incl2 = wave_scan_max(za);
            int run1 = wave_shift_up1(incl1, NEG2), run2 = wave_shift_up1(incl2, NEG2);
            if (NT > 64) {
                if (lane == 63) { s_wtot[2 * w] = incl1; s_wtot[2 * w + 1] = incl2; }
                __syncthreads();
                for (uint32_t q = 0; q < w; q++) { run1 = max(run1, s_wtot[2 * q]); run2 = max(run2, s_wtot[2 * q + 1]); }
            }
            Cell<GM>* row = H + (size_t)i * W;
#pragma unroll
            for (int k = 0; k < CPL; k++) {
                const uint32_t j = j0 + k;
                // run1 / run2: max over columns < j of X - k e / X - k c (column 0: the identity, E and Q stay below every real value)
                const int32_t h = max(x[k], max(run1 + go + ((int32_t)j - 1) * ge, run2 + qo + ((int32_t)j - 1) * qe));
                run1 = max(run1, x[k] - (int32_t)j * ge);
                run2 = max(run2, x[k] - (int32_t)j * qe);
                if (j <= L) {
                    row[j] = Cell3{h, f[k], o[k]};
                    const bool cand = j >= 1 && (type == MT_SW || (type == MT_NW ? sink && j == L : sink || j == L));
                    if (cand && h > bv) { bv = h; bi = i; bj = j; }
                }
            }
        }
        __syncthreads();   // the row is visible to every lane before a later row reads it (and s_wtot is free again)
    }
    // the end cell: the first maximum in row-major order, i.e. the smallest (row, column) among the lanes' best
    if (t == 0) { sh.best = type == MT_SW ? 0 : NEG; sh.key = ~0ull; }
    __syncthreads();
    if (bi) atomicMax(&sh.best, bv);
    __syncthreads();
    if (bi && bv == sh.best) atomicMin(&sh.key, ((unsigned long long)bi << 32) | bj);
    __syncthreads();
    const unsigned long long key = sh.key;
    *bi_out = key == ~0ull ? 0u : (uint32_t)(key >> 32);
    *bj_out = key == ~0ull ? 0u : (uint32_t)key;
    __syncthreads();
}

// The traceback from (i, j); thread 0. Leaves the pairs REVERSED in aln_node / aln_pos (add_alignment's layout) and returns their number, 0 when
// no pair holds a sequence position (the alignment counts as empty). This is the walk of the two gapped models, with a state: H, the vertical F or
// (convex) O, and (affine) the horizontal E; the linear walk, which has no states, is the specialisation below.
// Horizontal gaps. Affine: state E is entered where H is neither a diagonal match nor F, so H == E; E of the current cell is carried in ev, and
// E[i][j-1] = E[i][j] - e wherever E[i][j] != H[i][j-1] + g. Convex: resolved by length in state H: the smallest k with H[i][j] == H[i][j-k] +
// w(k), w(k) = max(g + (k-1) e, q + (k-1) c) kept incrementally, gives k pairs and leaves the walk in state H.
template <int GM>
__device__ uint32_t traceback(G& g, const Cell<GM>* H, const uint8_t* s, const uint32_t L, uint32_t i, uint32_t j, const MArgs& a) {
    const uint32_t W = L + 1;
    uint32_t na = 0;
    bool anypos = false;
    int st = 0;   // 0 H, 1 F, 2 O (convex), 3 E (affine)
    int32_t ev = 0;   // state E: E of the current cell
    for (;;) {
        const Cell<GM> c = H[(size_t)i * W + j];
        uint32_t np = 0, off = 0, code = 0;
        if (i != 0) { const uint32_t meta = g.row_meta[i - 1]; np = meta >> META_NP; off = g.row_pred_off[i - 1]; code = meta & 3u; }
        const uint32_t npp = np ? np : 1u;
        if (st == 0) {
            if (a.type == MT_SW ? c.x == 0 : a.type == MT_NW ? (i == 0 && j == 0) : (i == 0 || j == 0)) break;
            bool ok = false;
            if (i != 0 && j != 0) {
                const int32_t sg = s[j - 1] == code ? a.m : a.n;
                for (uint32_t p = 0; p < npp && !ok; p++) {
                    const uint32_t prow = np ? g.pred_rank[off + p] + 1u : 0u;
                    if (c.x == H[(size_t)prow * W + j - 1].x + sg) {
                        g.aln_node[na] = (int32_t)g.rank2node[i - 1]; g.aln_pos[na] = (int32_t)(j - 1); na++;
                        anypos = true; i = prow; j--; ok = true;
                    }
                }
            }
            if (ok) continue;
            if (i != 0 && c.x == c.y) { st = 1; continue; }
            if constexpr (GM == GM_AFFINE) { st = 3; ev = c.x; continue; }
            else {
                if (i != 0 && c.x == c.z) { st = 2; continue; }
                uint32_t k = 1;
                int32_t w1 = a.g, w2 = a.q;
                for (; k <= j; k++, w1 += a.e, w2 += a.c)
                    if (c.x == H[(size_t)i * W + j - k].x + max(w1, w2)) break;
                if (k > j) break;   // (cannot happen on a consistent matrix)
                for (uint32_t d = 1; d <= k; d++) { g.aln_node[na] = -1; g.aln_pos[na] = (int32_t)(j - d); na++; }
                anypos = true;
                j -= k;
            }
        } else if (GM == GM_CONVEX || st == 1) {
            // vertical, F under the first piece or O under the second: the first predecessor that opens the gap (then state H) or extends it
            int32_t cur = c.y;
            if constexpr (GM == GM_CONVEX) cur = st == 1 ? c.y : c.z;
            const int32_t open_s = GM == GM_AFFINE || st == 1 ? a.g : a.q, ext_s = GM == GM_AFFINE || st == 1 ? a.e : a.c;
            bool ok = false;
            for (uint32_t p = 0; p < npp && !ok; p++) {
                const uint32_t prow = np ? g.pred_rank[off + p] + 1u : 0u;
                const Cell<GM> v = H[(size_t)prow * W + j];
                const bool open = cur == v.x + open_s;
                int32_t vg = v.y;
                if constexpr (GM == GM_CONVEX) vg = st == 1 ? v.y : v.z;
                if (open || cur == vg + ext_s) {
                    g.aln_node[na] = (int32_t)g.rank2node[i - 1]; g.aln_pos[na] = -1; na++;
                    i = prow; if (open) st = 0; ok = true;
                }
            }
            if (!ok) break;   // (cannot happen on a consistent matrix)
        } else {   // state E (affine only): one base to the left
            if (j == 0) break;   // (cannot happen on a consistent matrix)
            g.aln_node[na] = -1; g.aln_pos[na] = (int32_t)(j - 1); na++;
            anypos = true;
            if (ev == H[(size_t)i * W + j - 1].x + a.g) st = 0; else ev -= a.e;
            j--;
        }
    }
    return anypos ? na : 0u;
}

// spoa's traceback for linear gaps: a literal compare walk over H (first matching predecessor: diagonal, then vertical, then horizontal)
template <>
__device__ uint32_t traceback<GM_LINEAR>(G& g, const int32_t* H, const uint8_t* s, const uint32_t L, uint32_t i, uint32_t j, const MArgs& a) {
    const uint32_t W = L + 1;
    uint32_t na = 0;
    bool anypos = false;
    for (;;) {
        const int32_t h = H[(size_t)i * W + j];
        if (a.type == MT_SW ? h == 0 : a.type == MT_NW ? (i == 0 && j == 0) : (i == 0 || j == 0)) break;
        uint32_t pi = i, pj = j, np = 0, off = 0, code = 0;
        bool ok = false;
        if (i != 0) { const uint32_t meta = g.row_meta[i - 1]; np = meta >> META_NP; off = g.row_pred_off[i - 1]; code = meta & 3u; }
        const uint32_t npp = np ? np : 1u;
        if (i != 0 && j != 0) {
            const int32_t sg = s[j - 1] == code ? a.m : a.n;
            for (uint32_t p = 0; p < npp && !ok; p++) {
                const uint32_t prow = np ? g.pred_rank[off + p] + 1u : 0u;
                if (h == H[(size_t)prow * W + j - 1] + sg) { pi = prow; pj = j - 1; ok = true; }
            }
        }
        if (!ok && i != 0)
            for (uint32_t p = 0; p < npp && !ok; p++) {
                const uint32_t prow = np ? g.pred_rank[off + p] + 1u : 0u;
                if (h == H[(size_t)prow * W + j] + a.g) { pi = prow; pj = j; ok = true; }
            }
        if (!ok) { if (j == 0) break; pj = j - 1; }   // horizontal (j = 0 cannot happen on a consistent matrix)
        g.aln_node[na] = pi != i ? (int32_t)g.rank2node[i - 1] : -1;
        g.aln_pos[na] = pj != j ? (int32_t)(j - 1) : -1;
        anypos = anypos || pj != j;
        na++;
        i = pi; j = pj;
    }
    return anypos ? na : 0u;
}
