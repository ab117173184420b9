// poa_modes_dp.inl - the DP and the traceback of the general POA path (kernels/poa_modes.hip), linear, affine and convex gaps. Included inside that
// file's anonymous namespace, after MArgs, Shared and the MT_* types. The recurrences keep a row loop each: they differ in substance (one
// accumulator per column against two or three, an inclusive against one or two exclusive prefix maxima). What the loops and the tracebacks still repeat
// (the sq[] packing, the cross-wave carry, the end-cell test and reduction, the row-record and predecessor-row lookups) is spelt out in
// each on purpose for now: every extraction tried reorders the instruction streams of the instances ("Refactor").

// DP of sequence s[0, L) against the V rows; returns through *bi / *bj the end cell (bi = 0: none - kSW without a cell above 0)
template <int NT, int CPL>
__device__ void dp_rows(const G& g, int32_t* H, const uint32_t V, const uint8_t* s, const uint32_t L, const MArgs& a, Shared& sh, int* s_wtot,
                        uint32_t* bi_out, uint32_t* bj_out) {
    constexpr int NEG2 = -(1 << 30);   // identity of the scans (below every real and every NEG-derived value)
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    const uint32_t W = L + 1, j0 = t * CPL;
    const int32_t m = a.m, n = a.n, gp = a.g;
    const int type = a.type;
    uint32_t sq[(CPL + 15) / 16];   // s[j - 1] of the lane's columns, 2 bits each
#pragma unroll
    for (int q = 0; q < (CPL + 15) / 16; q++) sq[q] = 0;
#pragma unroll
    for (int k = 0; k < CPL; k++) { const uint32_t j = j0 + k; if (j >= 1 && j <= L) sq[k >> 4] |= (uint32_t)s[j - 1] << (2 * (k & 15)); }
#pragma unroll
    for (int k = 0; k < CPL; k++) { const uint32_t j = j0 + k; if (j <= L) H[j] = type == MT_NW ? (int32_t)j * gp : 0; }
    __syncthreads();
    int32_t bv = type == MT_SW ? 0 : NEG;
    uint32_t bi = 0, bj = 0;
    uint32_t meta = g.row_meta[0], off = g.row_pred_off[0];
    for (uint32_t i = 1; i <= V; i++) {
        const uint32_t cmeta = meta, coff = off;
        if (i < V) { meta = g.row_meta[i]; off = g.row_pred_off[i]; }   // the next row's record, while this one runs
        const uint32_t np = cmeta >> META_NP, code = cmeta & 3u;
        const bool sink = (cmeta & 4u) != 0;
        int32_t x[CPL];
#pragma unroll
        for (int k = 0; k < CPL; k++) x[k] = NEG;
        const uint32_t npp = np ? np : 1u;
        for (uint32_t p = 0; p < npp; p++) {
            const uint32_t prow = np ? g.pred_rank[coff + p] + 1u : 0u;
            const int32_t* hp = H + (size_t)prow * W;
            int32_t left = j0 >= 1 && j0 <= W ? hp[j0 - 1] : NEG;
#pragma unroll
            for (int k = 0; k < CPL; k++) {
                const uint32_t j = j0 + k;
                if (j <= L) {
                    const int32_t v = hp[j];
                    const int32_t sg = ((sq[k >> 4] >> (2 * (k & 15))) & 3u) == code ? m : n;
                    x[k] = max(x[k], max(left + sg, v + gp));
                    left = v;
                }
            }
        }
        if (type != MT_NW && j0 == 0) x[0] = 0;   // H[r][0] of kSW / kOV (kNW: max over P(r) of H[p][0] + g, which the fold above gave)
        // horizontal: H[j] = j g + max over k <= j of (x[k] - k g)
#pragma unroll
        for (int k = 0; k < CPL; k++) { x[k] -= (int32_t)(j0 + k) * gp; if (k) x[k] = max(x[k], x[k - 1]); }
        const int incl = wave_scan_max(x[CPL - 1]);
        int carry = wave_shift_up1(incl, NEG2);
        if (NT > 64) {
            if (lane == 63) s_wtot[w] = incl;
            __syncthreads();
            for (uint32_t q = 0; q < w; q++) carry = max(carry, s_wtot[q]);
        }
        int32_t* row = H + (size_t)i * W;
#pragma unroll
        for (int k = 0; k < CPL; k++) {
            const uint32_t j = j0 + k;
            int32_t h = max(x[k], carry) + (int32_t)j * gp;
            if (type == MT_SW) h = max(h, 0);
            if (j <= L) {
                row[j] = h;
                const bool cand = j >= 1 && (type == MT_SW || (type == MT_NW ? sink && j == L : sink || j == L));
                if (cand && h > bv) { bv = h; bi = i; bj = j; }
            }
        }
        __syncthreads();   // the row is visible to every lane before a later row reads it (and s_wtot is free again)
    }
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

// spoa's traceback from (i, j); thread 0. Leaves the pairs REVERSED in aln_node / aln_pos (add_alignment's layout) and returns their number,
// 0 when no pair holds a sequence position (the alignment counts as empty).
__device__ uint32_t traceback(G& g, const int32_t* H, const uint8_t* s, const uint32_t L, uint32_t i, uint32_t j, const MArgs& a) {
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

// ---- affine gaps (DESIGN.md "General POA path", "Affine gaps"): gap open a.g, gap extend a.e, g <= e <= 0 ----
// A cell of the matrix is the pair (H, F). E is not stored: a row needs it only in registers, and the traceback rebuilds it as it walks.
//
// DP row: per predecessor, H[p][j-1] + sigma is folded into the diagonal candidate and max(H[p][j] + g, F[p][j] + e) into F. With
// X[k] = max(diagonal, F) of column k (kSW: clamped at 0; column 0: H[r][0]) the horizontal recurrence E[j] = max(H[j-1] + g, E[j-1] + e),
// H[j] = max(X[j], E[j]) unrolls to E[j] = g + (j-1) e + max over k < j of (X[k] - k e): a term that passes through an E[k] on its way
// (H[k] = E[k]) pays g where the direct term from the same X[k'] pays e, and g <= e, so it never wins. e = 0 needs nothing else (the
// argument uses g <= e only), and the kSW clamp commutes with the maximum: max(X[k], E[k], 0) = max(max(X[k], 0), E[k]). So E is the
// linear path's prefix maximum made exclusive.
template <int NT, int CPL>
__device__ void dp_rows_affine(const G& g, int2* HF, const uint32_t V, const uint8_t* s, const uint32_t L, const MArgs& a, Shared& sh, int* s_wtot,
                               uint32_t* bi_out, uint32_t* bj_out) {
    constexpr int NEG2 = -(1 << 30);
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    const uint32_t W = L + 1, j0 = t * CPL;
    const int32_t m = a.m, n = a.n, go = a.g, ge = a.e;
    const int type = a.type;
    uint32_t sq[(CPL + 15) / 16];
#pragma unroll
    for (int q = 0; q < (CPL + 15) / 16; q++) sq[q] = 0;
#pragma unroll
    for (int k = 0; k < CPL; k++) { const uint32_t j = j0 + k; if (j >= 1 && j <= L) sq[k >> 4] |= (uint32_t)s[j - 1] << (2 * (k & 15)); }
#pragma unroll
    for (int k = 0; k < CPL; k++) { const uint32_t j = j0 + k; if (j <= L) HF[j] = make_int2(type == MT_NW && j ? go + ((int32_t)j - 1) * ge : 0, NEG); }
    __syncthreads();
    int32_t bv = type == MT_SW ? 0 : NEG;
    uint32_t bi = 0, bj = 0;
    uint32_t meta = g.row_meta[0], off = g.row_pred_off[0];
    for (uint32_t i = 1; i <= V; i++) {
        const uint32_t cmeta = meta, coff = off;
        if (i < V) { meta = g.row_meta[i]; off = g.row_pred_off[i]; }
        const uint32_t np = cmeta >> META_NP, code = cmeta & 3u;
        const bool sink = (cmeta & 4u) != 0;
        int32_t x[CPL], f[CPL];
#pragma unroll
        for (int k = 0; k < CPL; k++) { x[k] = NEG; f[k] = NEG; }
        const uint32_t npp = np ? np : 1u;
        for (uint32_t p = 0; p < npp; p++) {
            const uint32_t prow = np ? g.pred_rank[coff + p] + 1u : 0u;
            const int2* hp = HF + (size_t)prow * W;
            int32_t left = j0 >= 1 && j0 <= W ? hp[j0 - 1].x : NEG;
#pragma unroll
            for (int k = 0; k < CPL; k++) {
                const uint32_t j = j0 + k;
                if (j <= L) {
                    const int2 v = hp[j];
                    const int32_t sg = ((sq[k >> 4] >> (2 * (k & 15))) & 3u) == code ? m : n;
                    x[k] = max(x[k], left + sg);
                    f[k] = max(f[k], max(v.x + go, v.y + ge));
                    left = v.x;
                }
            }
        }
        if (type != MT_NW && j0 == 0) { x[0] = 0; f[0] = NEG; }   // column 0 of kSW / kOV: H = 0, F = -inf (kNW: H[r][0] = F[r][0], which the fold gave)
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
        int2* row = HF + (size_t)i * W;
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
        __syncthreads();
    }
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

// the affine traceback: a walk with a state (H, F or E); thread 0. E of the current cell is carried in ev: state E is entered where
// H == E, and E[i][j-1] = E[i][j] - e wherever E[i][j] != H[i][j-1] + g. Same output layout as traceback().
__device__ uint32_t traceback_affine(G& g, const int2* HF, const uint8_t* s, const uint32_t L, uint32_t i, uint32_t j, const MArgs& a) {
    const uint32_t W = L + 1;
    uint32_t na = 0;
    bool anypos = false;
    int st = 0;   // 0 H, 1 F, 2 E
    int32_t ev = 0;
    for (;;) {
        const int2 c = HF[(size_t)i * W + j];
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
                    if (c.x == HF[(size_t)prow * W + j - 1].x + sg) {
                        g.aln_node[na] = (int32_t)g.rank2node[i - 1]; g.aln_pos[na] = (int32_t)(j - 1); na++;
                        anypos = true; i = prow; j--; ok = true;
                    }
                }
            }
            if (!ok) { if (i != 0 && c.x == c.y) st = 1; else { st = 2; ev = c.x; } }
        } else if (st == 1) {
            bool ok = false;
            for (uint32_t p = 0; p < npp && !ok; p++) {
                const uint32_t prow = np ? g.pred_rank[off + p] + 1u : 0u;
                const int2 v = HF[(size_t)prow * W + j];
                const bool open = c.y == v.x + a.g;
                if (open || c.y == v.y + a.e) {
                    g.aln_node[na] = (int32_t)g.rank2node[i - 1]; g.aln_pos[na] = -1; na++;
                    i = prow; st = open ? 0 : 1; ok = true;
                }
            }
            if (!ok) break;   // (cannot happen on a consistent matrix)
        } else {
            if (j == 0) break;   // (cannot happen on a consistent matrix)
            g.aln_node[na] = -1; g.aln_pos[na] = (int32_t)(j - 1); na++;
            anypos = true;
            if (ev == HF[(size_t)i * W + j - 1].x + a.g) st = 0; else ev -= a.e;
            j--;
        }
    }
    return anypos ? na : 0u;
}

// ---- convex gaps (DESIGN.md "General POA path", "Convex gaps"): a gap of k bases scores max(g + (k-1) e, q + (k-1) c); first piece a.g / a.e,
// second piece a.q / a.c, each with open <= extend <= 0, q <= g ----
// A cell of the matrix is (H, F, O), 12 bytes: F and O are the vertical gap under the first and the second piece. Neither E nor Q is stored.
//
// DP row: per predecessor, H[p][j-1] + sigma goes into the diagonal candidate, max(H[p][j] + g, F[p][j] + e) into F and max(H[p][j] + q,
// O[p][j] + c) into O. With X[k] = max(diagonal, F, O) of column k (kSW: clamped at 0; column 0: H[r][0]) and w(d) = max(g + (d-1) e,
// q + (d-1) c), the recurrences unroll to H[j] = max(X[j], max over k < j of H[k] + w(j-k)), and w(a) + w(b) <= w(a+b) (each piece opens no
// cheaper than it extends, and q <= g; DESIGN.md has the cases), so a term that passes through another gap on its way never beats the direct
// one: H[j] = max(X[j], E'[j], Q'[j]) with E'[j] = g + (j-1) e + max over k < j of (X[k] - k e) and Q'[j] = q + (j-1) c + max over k < j of
// (X[k] - k c), two exclusive prefix maxima over the same X. E' and Q' can lie below the literal E and Q (a gap that changes its piece on the
// way); their maximum with X cannot, and only H is kept. The scans share the barrier; the in-lane prefixes are rebuilt in the store loop
// instead of kept in registers.
struct Cell3 { int32_t x, y, z; };   // H, F, O

template <int NT, int CPL>
__device__ void dp_rows_convex(const G& g, Cell3* HFO, const uint32_t V, const uint8_t* s, const uint32_t L, const MArgs& a, Shared& sh, int* s_wtot,
                               uint32_t* bi_out, uint32_t* bj_out) {
    constexpr int NEG2 = -(1 << 30);
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    const uint32_t W = L + 1, j0 = t * CPL;
    const int32_t m = a.m, n = a.n, go = a.g, ge = a.e, qo = a.q, qe = a.c;
    const int type = a.type;
    uint32_t sq[(CPL + 15) / 16];
#pragma unroll
    for (int q = 0; q < (CPL + 15) / 16; q++) sq[q] = 0;
#pragma unroll
    for (int k = 0; k < CPL; k++) { const uint32_t j = j0 + k; if (j >= 1 && j <= L) sq[k >> 4] |= (uint32_t)s[j - 1] << (2 * (k & 15)); }
#pragma unroll
    for (int k = 0; k < CPL; k++) {
        const uint32_t j = j0 + k;
        if (j <= L) HFO[j] = Cell3{type == MT_NW && j ? max(go + ((int32_t)j - 1) * ge, qo + ((int32_t)j - 1) * qe) : 0, NEG, NEG};
    }
    __syncthreads();
    int32_t bv = type == MT_SW ? 0 : NEG;
    uint32_t bi = 0, bj = 0;
    uint32_t meta = g.row_meta[0], off = g.row_pred_off[0];
    for (uint32_t i = 1; i <= V; i++) {
        const uint32_t cmeta = meta, coff = off;
        if (i < V) { meta = g.row_meta[i]; off = g.row_pred_off[i]; }
        const uint32_t np = cmeta >> META_NP, code = cmeta & 3u;
        const bool sink = (cmeta & 4u) != 0;
        int32_t x[CPL], f[CPL], o[CPL];
#pragma unroll
        for (int k = 0; k < CPL; k++) { x[k] = NEG; f[k] = NEG; o[k] = NEG; }
        const uint32_t npp = np ? np : 1u;
        for (uint32_t p = 0; p < npp; p++) {
            const uint32_t prow = np ? g.pred_rank[coff + p] + 1u : 0u;
            const Cell3* hp = HFO + (size_t)prow * W;
            int32_t left = j0 >= 1 && j0 <= W ? hp[j0 - 1].x : NEG;
#pragma unroll
            for (int k = 0; k < CPL; k++) {
                const uint32_t j = j0 + k;
                if (j <= L) {
                    const Cell3 v = hp[j];
                    const int32_t sg = ((sq[k >> 4] >> (2 * (k & 15))) & 3u) == code ? m : n;
                    x[k] = max(x[k], left + sg);
                    f[k] = max(f[k], max(v.x + go, v.y + ge));
                    o[k] = max(o[k], max(v.x + qo, v.z + qe));
                    left = v.x;
                }
            }
        }
        if (type != MT_NW && j0 == 0) { x[0] = 0; f[0] = NEG; o[0] = NEG; }   // column 0 of kSW / kOV: H = 0, F = O = -inf (kNW: H[r][0] = max(F, O), which the fold gave)
        // X, and per piece the lane's maximum of X[k] - j e
        int32_t ya = NEG2, za = NEG2;
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
        Cell3* row = HFO + (size_t)i * W;
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
        __syncthreads();
    }
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

// the convex traceback: a walk with a state (H, F or O); thread 0. A horizontal gap is resolved by its length: the smallest k with
// H[i][j] == H[i][j-k] + w(k), w(k) = max(g + (k-1) e, q + (k-1) c) kept incrementally, gives k pairs and leaves the walk in state H.
// Same output layout as traceback().
__device__ uint32_t traceback_convex(G& g, const Cell3* HFO, const uint8_t* s, const uint32_t L, uint32_t i, uint32_t j, const MArgs& a) {
    const uint32_t W = L + 1;
    uint32_t na = 0;
    bool anypos = false;
    int st = 0;   // 0 H, 1 F, 2 O
    for (;;) {
        const Cell3 c = HFO[(size_t)i * W + j];
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
                    if (c.x == HFO[(size_t)prow * W + j - 1].x + sg) {
                        g.aln_node[na] = (int32_t)g.rank2node[i - 1]; g.aln_pos[na] = (int32_t)(j - 1); na++;
                        anypos = true; i = prow; j--; ok = true;
                    }
                }
            }
            if (ok) continue;
            if (i != 0 && c.x == c.y) { st = 1; continue; }
            if (i != 0 && c.x == c.z) { st = 2; continue; }
            uint32_t k = 1;
            int32_t w1 = a.g, w2 = a.q;
            for (; k <= j; k++, w1 += a.e, w2 += a.c)
                if (c.x == HFO[(size_t)i * W + j - k].x + max(w1, w2)) break;
            if (k > j) break;   // (cannot happen on a consistent matrix)
            for (uint32_t d = 1; d <= k; d++) { g.aln_node[na] = -1; g.aln_pos[na] = (int32_t)(j - d); na++; }
            anypos = true;
            j -= k;
        } else {
            const int32_t cur = st == 1 ? c.y : c.z, open_s = st == 1 ? a.g : a.q, ext_s = st == 1 ? a.e : a.c;
            bool ok = false;
            for (uint32_t p = 0; p < npp && !ok; p++) {
                const uint32_t prow = np ? g.pred_rank[off + p] + 1u : 0u;
                const Cell3 v = HFO[(size_t)prow * W + j];
                const bool open = cur == v.x + open_s;
                if (open || cur == (st == 1 ? v.y : v.z) + ext_s) {
                    g.aln_node[na] = (int32_t)g.rank2node[i - 1]; g.aln_pos[na] = -1; na++;
                    i = prow; if (open) st = 0; ok = true;
                }
            }
            if (!ok) break;   // (cannot happen on a consistent matrix)
        }
    }
    return anypos ? na : 0u;
}
