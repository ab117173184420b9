// poa_modes_band.inl - the banded row loop and traceback of the general POA path (kernels/poa_modes.hip; DESIGN.md section 11, "Banded alignment"),
// siblings of dp_rows and traceback (poa_modes_dp.inl), included after them. One wavefront of 64 lanes x 16 columns holds a row's window of
// B = 2w + 1 <= 1023 columns: lane t owns the columns lo_i + 16 t + k of row i, so the row's prefix maxima are wave scans and no row waits at a
// block-wide barrier of several waves. H is stored as (V + 1) x B cells, a cell at its column minus its row's first one; per row lo, m (the
// smallest column of its best reachable cell) and best stand in three word arrays behind H. The model blocks between "combine the accumulators"
// and the stores are dp_rows' own, statement for statement, at NT = 64.
//
// Minus infinity: the kernel leaves the values derived from NEG in place (the host's 2^28 bound keeps every one of them at or below
// UNREACHABLE and every real value above it) and asks `> UNREACHABLE` where the rules say "reachable": the row maximum, the end-cell
// candidates and every compare of the traceback.

constexpr int32_t UNREACHABLE = -(1 << 28);
constexpr int BAND_NT = 64, BAND_CPL = 16;
constexpr uint32_t BAND_SEQ_WORDS = 2049;   // 32 767 bases + position 0, 16 per word, and the word the last window's second read takes

// the band of one slot: the half-width and the window of the set's current attempt, the three per-row arrays
struct BandRows { uint32_t *lo, *m; int32_t* best; uint32_t w, B; };

template <int GM> __device__ __forceinline__ Cell<GM> neg_cell();
template <> __device__ __forceinline__ int32_t neg_cell<GM_LINEAR>() { return NEG; }
template <> __device__ __forceinline__ int2 neg_cell<GM_AFFINE>() { return make_int2(NEG, NEG); }
template <> __device__ __forceinline__ Cell3 neg_cell<GM_CONVEX>() { return Cell3{NEG, NEG, NEG}; }

// the wave's maximum of v (v >= -2^30), in every lane
__device__ __forceinline__ int wave_max_all(int v) { return __builtin_amdgcn_readlane(wave_scan_max(v), 63); }

// DP of sequence s[0, L) against the V rows inside the rows' windows; returns through *bi / *bj the end cell (bi = 0: none) and as its value
// whether the alignment missed its band (kNW and kOV without a reachable candidate; kSW without a cell above 0 is the empty alignment).
template <int GM>
__device__ bool dp_rows_band(const G& g, Cell<GM>* H, const BandRows& br, const uint32_t V, const uint8_t* s, const uint32_t L, const MArgs& a, Shared& sh,
                             uint32_t* bi_out, uint32_t* bj_out) {
    constexpr int CPL = BAND_CPL;
    constexpr int NEG2 = -(1 << 30);   // identity of the scans (below every real and every NEG-derived value)
    // position j holds s[j - 1] in 2 bits (position 0 is no base). In LDS and not read through L2: a lane's 16 letters move by a column from
    // row to row, so every row needs them again at another bit offset - two LDS words and a 64-bit shift here, 16 byte loads there
    __shared__ uint32_t s_seq[BAND_SEQ_WORDS];
    const uint32_t t = threadIdx.x;
    const uint32_t B = br.B, w = br.w;
    const int32_t m = a.m, n = a.n, go = a.g, ge = a.e, qo = a.q, qe = a.c;
    const int type = a.type;
    const uint32_t n_words = (L >> 4) + 2;   // <= BAND_SEQ_WORDS: L <= 32 767
    for (uint32_t q = t; q < n_words; q += BAND_NT) {
        uint32_t v = 0;
#pragma unroll
        for (int k = 0; k < 16; k++) { const uint32_t j = q * 16 + k; if (j >= 1 && j <= L) v |= (uint32_t)s[j - 1] << (2 * k); }
        s_seq[q] = v;
    }
    const uint32_t lo_max = L + 1 > B ? L + 1 - B : 0u;
    {   // row 0: its window starts at column 0; 0, under kNW a gap of j bases; F = O = -inf. Its best cell is column 0 in every mode
        const uint32_t hi = min(L, B - 1);
#pragma unroll
        for (int k = 0; k < CPL; k++) {
            const uint32_t j = t * CPL + k;
            if (j <= hi) {
                if constexpr (GM == GM_LINEAR) H[j] = type == MT_NW ? (int32_t)j * go : 0;
                else if constexpr (GM == GM_AFFINE) H[j] = make_int2(type == MT_NW && j ? go + ((int32_t)j - 1) * ge : 0, NEG);
                else H[j] = Cell3{type == MT_NW && j ? max(go + ((int32_t)j - 1) * ge, qo + ((int32_t)j - 1) * qe) : 0, NEG, NEG};
            }
        }
        if (t == 0) { br.lo[0] = 0; br.m[0] = 0; br.best[0] = 0; }
    }
    __syncthreads();
    int32_t bv = type == MT_SW ? 0 : UNREACHABLE;   // (a candidate above it is reachable)
    uint32_t bi = 0, bj = 0;
    uint32_t meta = g.row_meta[0], off = g.row_pred_off[0];
    for (uint32_t i = 1; i <= V; i++) {
        const uint32_t cmeta = meta, coff = off;
        if (i < V) { meta = g.row_meta[i]; off = g.row_pred_off[i]; }   // the next row's record, while this one runs
        const uint32_t np = cmeta >> META_NP, code = cmeta & 3u;
        const bool sink = (cmeta & 4u) != 0;
        const uint32_t npp = np ? np : 1u;
        // the window: its centre is one past the best cell's column of the predecessor with the largest best, the first among equals
        int32_t pb = 0;
        uint32_t pm = 0;
        for (uint32_t p = 0; p < npp; p++) {
            const uint32_t prow = np ? g.pred_rank[coff + p] + 1u : 0u;
            const int32_t b = br.best[prow];
            if (p == 0 || b > pb) { pb = b; pm = br.m[prow]; }
        }
        const uint32_t centre = min(pm + 1u, L);
        const uint32_t lo = min(centre > w ? centre - w : 0u, lo_max), hi = min(L, lo + B - 1);
        const uint32_t j0 = lo + t * CPL;
        uint32_t sq = 0;   // s[j - 1] of the lane's columns, 2 bits each
        if (j0 <= L) sq = (uint32_t)((((unsigned long long)s_seq[(j0 >> 4) + 1] << 32) | s_seq[j0 >> 4]) >> (2 * (j0 & 15u)));
        // per column: x the diagonal candidate (linear: and the vertical one), f / o the vertical gap under the first / the second piece
        int32_t x[CPL], f[GM >= GM_AFFINE ? CPL : 1], o[GM == GM_CONVEX ? CPL : 1];
#pragma unroll
        for (int k = 0; k < CPL; k++) {
            x[k] = NEG;
            if constexpr (GM >= GM_AFFINE) f[k] = NEG;
            if constexpr (GM == GM_CONVEX) o[k] = NEG;
        }
        for (uint32_t p = 0; p < npp; p++) {
            const uint32_t prow = np ? g.pred_rank[coff + p] + 1u : 0u;
            const Cell<GM>* hp = H + (size_t)prow * B;
            const uint32_t d = j0 - br.lo[prow];   // the lane's first column in the predecessor's window (wraps when it lies before it: >= B then)
            int32_t left = j0 >= 1 && d - 1u < B ? h_of(hp[d - 1u]) : NEG;
#pragma unroll
            for (int k = 0; k < CPL; k++) {
                const uint32_t j = j0 + k;
                if (j <= hi) {
                    const Cell<GM> v = d + k < B ? hp[d + k] : neg_cell<GM>();   // (j <= L and d + k < B: inside the predecessor's window)
                    const int32_t sg = ((sq >> (2 * k)) & 3u) == code ? m : n;
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
        // column 0 of kSW / kOV: H = 0, F = O = -inf
        if (type != MT_NW && j0 == 0) {
            x[0] = 0;
            if constexpr (GM >= GM_AFFINE) f[0] = NEG;
            if constexpr (GM == GM_CONVEX) o[0] = NEG;
        }
        int32_t rb = UNREACHABLE;   // the lane's best reachable cell of the row and its first column
        uint32_t rj = 0;
        Cell<GM>* row = H + (size_t)i * B + t * CPL;
        if constexpr (GM == GM_LINEAR) {
#pragma unroll
            for (int k = 0; k < CPL; k++) { x[k] -= (int32_t)(j0 + k) * go; if (k) x[k] = max(x[k], x[k - 1]); }
            const int incl = wave_scan_max(x[CPL - 1]);
            const int carry = wave_shift_up1(incl, NEG2);
#pragma unroll
            for (int k = 0; k < CPL; k++) {
                const uint32_t j = j0 + k;
                int32_t h = max(x[k], carry) + (int32_t)j * go;
                if (type == MT_SW) h = max(h, 0);
                if (j <= hi) {
                    row[k] = h;
                    if (h > rb) { rb = h; rj = j; }
                    const bool cand = j >= 1 && (type == MT_SW || (type == MT_NW ? sink && j == L : sink || j == L));
                    if (cand && h > bv) { bv = h; bi = i; bj = j; }
                }
            }
        } else if constexpr (GM == GM_AFFINE) {
#pragma unroll
            for (int k = 0; k < CPL; k++) { x[k] = max(x[k], f[k]); if (type == MT_SW) x[k] = max(x[k], 0); }
            int32_t y[CPL];
#pragma unroll
            for (int k = 0; k < CPL; k++) { y[k] = x[k] - (int32_t)(j0 + k) * ge; if (k) y[k] = max(y[k], y[k - 1]); }
            const int incl = wave_scan_max(y[CPL - 1]);
            const int carry = wave_shift_up1(incl, NEG2);
#pragma unroll
            for (int k = 0; k < CPL; k++) {
                const uint32_t j = j0 + k;
                const int32_t ex = k ? max(carry, y[k - 1]) : carry;
                const int32_t h = max(x[k], ex + go + ((int32_t)j - 1) * ge);
                if (j <= hi) {
                    row[k] = make_int2(h, f[k]);
                    if (h > rb) { rb = h; rj = j; }
                    const bool cand = j >= 1 && (type == MT_SW || (type == MT_NW ? sink && j == L : sink || j == L));
                    if (cand && h > bv) { bv = h; bi = i; bj = j; }
                }
            }
        } else {
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
#pragma unroll
            for (int k = 0; k < CPL; k++) {
                const uint32_t j = j0 + k;
                const int32_t h = max(x[k], max(run1 + go + ((int32_t)j - 1) * ge, run2 + qo + ((int32_t)j - 1) * qe));
                run1 = max(run1, x[k] - (int32_t)j * ge);
                run2 = max(run2, x[k] - (int32_t)j * qe);
                if (j <= hi) {
                    row[k] = Cell3{h, f[k], o[k]};
                    if (h > rb) { rb = h; rj = j; }
                    const bool cand = j >= 1 && (type == MT_SW || (type == MT_NW ? sink && j == L : sink || j == L));
                    if (cand && h > bv) { bv = h; bi = i; bj = j; }
                }
            }
        }
        // the row's best reachable cell, the first column among equals: two wave reductions
        const int32_t best = wave_max_all(rb);
        const uint32_t first = (uint32_t)-wave_max_all(rb == best ? -(int32_t)rj : NEG2);
        if (t == 0) {
            const bool any = best > UNREACHABLE;
            br.lo[i] = lo; br.m[i] = any ? first : centre; br.best[i] = any ? best : NEG;
        }
        __syncthreads();   // the row and its record are visible to every lane before a later row reads them (one wavefront: no wave waits for another)
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
    return key == ~0ull && type != MT_SW;
}

// The traceback from (i, j) through the rows' windows; thread 0. dp traceback's walks (poa_modes_dp.inl: the literal compare walk for linear gaps, the
// walk with a state for the two gapped models) with every read of H going through the window of its row: a cell outside it is minus infinity, and
// an unreachable neighbour never matches. Leaves the pairs REVERSED in aln_node / aln_pos and returns their number, 0 when no pair holds a position.
template <int GM>
__device__ uint32_t traceback_band(G& g, const Cell<GM>* H, const BandRows& br, const uint8_t* s, const uint32_t L, uint32_t i, uint32_t j, const MArgs& a) {
    const uint32_t B = br.B;
    // (j - 1 at j = 0 wraps: no column of a window)
    auto cell = [&](uint32_t r, uint32_t c) { const uint32_t d = c - br.lo[r]; return c <= L && d < B ? H[(size_t)r * B + d] : neg_cell<GM>(); };
    auto inside = [&](uint32_t r, uint32_t c) { return c <= L && c - br.lo[r] < B; };
    uint32_t na = 0;
    bool anypos = false;
    if constexpr (GM == GM_LINEAR) {
        for (;;) {
            const int32_t h = cell(i, j);
            if (a.type == MT_SW ? h == 0 : a.type == MT_NW ? (i == 0 && j == 0) : (i == 0 || j == 0)) break;
            uint32_t pi = i, pj = j, np = 0, off = 0, code = 0;
            bool ok = false;
            if (i != 0) { const uint32_t meta = g.row_meta[i - 1]; np = meta >> META_NP; off = g.row_pred_off[i - 1]; code = meta & 3u; }
            const uint32_t npp = np ? np : 1u;
            if (i != 0 && j != 0) {
                const int32_t sg = s[j - 1] == code ? a.m : a.n;
                for (uint32_t p = 0; p < npp && !ok; p++) {
                    const uint32_t prow = np ? g.pred_rank[off + p] + 1u : 0u;
                    const int32_t v = cell(prow, j - 1);
                    if (v > UNREACHABLE && h == v + sg) { pi = prow; pj = j - 1; ok = true; }
                }
            }
            if (!ok && i != 0)
                for (uint32_t p = 0; p < npp && !ok; p++) {
                    const uint32_t prow = np ? g.pred_rank[off + p] + 1u : 0u;
                    const int32_t v = cell(prow, j);
                    if (v > UNREACHABLE && h == v + a.g) { pi = prow; pj = j; ok = true; }
                }
            if (!ok) { if (j == 0 || !inside(i, j - 1)) break; pj = j - 1; }   // horizontal (the break cannot happen on a consistent matrix)
            g.aln_node[na] = pi != i ? (int32_t)g.rank2node[i - 1] : -1;
            g.aln_pos[na] = pj != j ? (int32_t)(j - 1) : -1;
            anypos = anypos || pj != j;
            na++;
            i = pi; j = pj;
        }
    } else {
        int st = 0;       // 0 H, 1 F, 2 O (convex), 3 E (affine)
        int32_t ev = 0;   // state E: E of the current cell
        for (;;) {
            const Cell<GM> c = cell(i, j);
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
                        const int32_t v = cell(prow, j - 1).x;
                        if (v > UNREACHABLE && c.x == v + sg) {
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
                    bool hit = false;
                    for (; k <= j && inside(i, j - k); k++, w1 += a.e, w2 += a.c) {
                        const int32_t v = cell(i, j - k).x;
                        if (v > UNREACHABLE && c.x == v + max(w1, w2)) { hit = true; break; }
                    }
                    if (!hit) break;   // (cannot happen on a consistent matrix)
                    for (uint32_t d = 1; d <= k; d++) { g.aln_node[na] = -1; g.aln_pos[na] = (int32_t)(j - d); na++; }
                    anypos = true;
                    j -= k;
                }
            } else if (GM == GM_CONVEX || st == 1) {
                int32_t cur = c.y;
                if constexpr (GM == GM_CONVEX) cur = st == 1 ? c.y : c.z;
                const int32_t open_s = GM == GM_AFFINE || st == 1 ? a.g : a.q, ext_s = GM == GM_AFFINE || st == 1 ? a.e : a.c;
                bool ok = false;
                for (uint32_t p = 0; p < npp && !ok; p++) {
                    const uint32_t prow = np ? g.pred_rank[off + p] + 1u : 0u;
                    const Cell<GM> v = cell(prow, j);
                    const bool open = v.x > UNREACHABLE && cur == v.x + open_s;
                    int32_t vg = v.y;
                    if constexpr (GM == GM_CONVEX) vg = st == 1 ? v.y : v.z;
                    if (open || (vg > UNREACHABLE && cur == vg + ext_s)) {
                        g.aln_node[na] = (int32_t)g.rank2node[i - 1]; g.aln_pos[na] = -1; na++;
                        i = prow; if (open) st = 0; ok = true;
                    }
                }
                if (!ok) break;   // (cannot happen on a consistent matrix)
            } else {   // state E (affine only): one base to the left
                if (j == 0 || !inside(i, j - 1)) break;   // (cannot happen on a consistent matrix)
                g.aln_node[na] = -1; g.aln_pos[na] = (int32_t)(j - 1); na++;
                anypos = true;
                const int32_t v = cell(i, j - 1).x;
                if (v > UNREACHABLE && ev == v + a.g) st = 0; else ev -= a.e;
                j--;
            }
        }
    }
    return anypos ? na : 0u;
}
