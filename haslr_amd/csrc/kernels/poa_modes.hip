// poa_modes.hip — the general POA path: spoa's linear-gap engine in its three alignment modes (kSW local, kNW global, kOV overlap) for
// caller-given sequence sets (hx_poa_sequences_mode; DESIGN.md "General POA path" has the semantics and the mapping), and the affine-gap
// engine in the same modes (hx_poa_sequences_affine; k_poa_affine below: same mapping, a cell is the pair (H, F), its own instance table).
//
// It is a kernel family of its own beside the tuned global-only k_poa (kernels/poa.hip), which depends on kNW throughout (de-ramped keys
// with tie bits, score-bound pruning, sink lists, end-node ties decided on closures, multi-member pipelines). What the modes share with
// kNW - spoa's add_alignment, its topological sort, the heaviest bundle with branch completion - is poa_graph.inl, included here as it is.
//
// Mapping: one workgroup per set; persistent workgroups pull set indices off a device counter; each owns one slot of the workspace (graph
// pools sized for the set's total length, then the int32 score matrix H). For every sequence, in order:
//   * DP, one row per node in spoa's rank order: a lane owns CPL contiguous columns in registers; the predecessor rows' diagonal and vertical
//     candidates are folded in in-edge order; the horizontal recurrence is a prefix maximum of H[j] - j g (in-lane, then a DPP wave scan and
//     a scan of the wave totals); kSW clamps at 0 after the scan (exact: a clamped 0 only ever propagates g < 0). The end cell is the first
//     maximum in row-major order over the mode's candidate cells (per-lane first maxima, then the smallest (row, column) among the best).
//   * traceback: spoa's literal compare walk over H (first matching predecessor: diagonal, then vertical, then horizontal), thread 0
//   * graph update (add_alignment), spoa's topological sort (thread 0), rank-ordered predecessor rows (all lanes)
// and at the end the heaviest bundle with branch completion by the first wavefront. A set whose next alignment needs more of H than its slot
// holds stops with a status; the host reruns it in a larger slot.
//
// The multiple sequence alignment of a set (hx_poa_msa; DESIGN.md "MSA output") comes from the same workgroup under a template flag: it keeps
// the node of every base that add_alignment reports, turns nodes into columns after the last sort, and a second, grid-wide kernel
// (k_msa_rows) writes the row text once the host knows the sizes.
//
// Per-base weights and consensus coverage (hx_poa_weighted; DESIGN.md "Base weights and coverage") are one more template flag on top of the
// MSA one: after add_alignment all lanes add w[i-1] + w[i] - 2 to the edge between the nodes of bases i-1 and i (add_alignment gave it 2), so
// the heaviest bundle sees spoa's weighted edges; two grid-wide kernels (k_cov_hist, k_cov_gather) count the bases per column and letter and
// pick the counts at the consensus bases' columns.
#include <algorithm>
#include <chrono>
#include <numeric>

#include "kernels.h"
#include "poa_modes.h"

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "kernels/poa_modes.hip is written for gfx950 (CDNA4)"
#endif

namespace hxk {

namespace {

#include "poa_graph.inl"    // the graph of a set, spoa's topological order, heaviest bundle

enum { MT_SW = 0, MT_NW = 1, MT_OV = 2 };
enum { MS_OK = 0, MS_H_OVERFLOW = 1, MS_GRAPH_OVERFLOW = 2 };
constexpr uint32_t MAX_SET_BASES = (1u << 21) - 2;   // node ids are packed in 21 bits (+1) in the node records of poa_graph.inl

struct MSet { uint64_t seq_begin, sum_len, cns_off; uint32_t nseq, lmax; };

struct MArgs {
    const MSet* sets; const uint32_t* order; uint32_t n_items; uint32_t* counter;
    const uint8_t* codes; const uint64_t* soff;
    uint8_t* ws; uint64_t slot_bytes;
    int32_t m, n, g, type;
    char* cns; uint32_t *cns_len, *status, *vseen; unsigned long long* cells;
    int32_t e;   // affine instances only: gap extend (g is gap open)
    // MSA instances only: per base of the call (global offset) its node, rewritten to its column when the set is done; columns per set;
    // column of every consensus base beside cns (null: not asked for)
    uint32_t *base_col, *n_cols, *cns_col;
    const uint8_t* wts;   // weighted instances only: the weight of every base of the call (1..255), beside codes
};

// one row of the MSA text: its columns (rising) start at cols[src], its letters at codes[src] (a sequence) or cns[src] (the consensus row)
struct MRow { uint64_t src, dst; uint32_t len, ncols, is_cns, pad; };

__host__ __device__ inline uint64_t al256(uint64_t x) { return (x + 255) & ~255ull; }

// the graph pools of a set at the start of its slot: at most one node per base (vcap = total length), one edge per base and sequence.
// Returns their bytes; fills g / path / colref when base is not null. The host sizes slots with the same function.
__host__ __device__ inline uint64_t carve_pools(uint8_t* base, uint64_t T, uint32_t nseq, uint32_t lmax, G* g, uint32_t** path, uint32_t** colref) {
    const uint64_t vc = T + 1, ec = T + nseq + 1, ac = T + lmax + 2, sc = 4 * vc + ec + 64;
    uint64_t off = 0;
    auto take = [&](uint64_t bytes) -> uint8_t* { uint8_t* p = base ? base + off : nullptr; off += al256(bytes); return p; };
    G t{};
    t.code = take(vc); t.n_aligned = take(vc); t.mark = take(vc); t.check = take(vc);
    t.aligned = (uint32_t*)take(12 * vc);
    t.in_head = (uint32_t*)take(4 * vc); t.in_tail = (uint32_t*)take(4 * vc); t.out_head = (uint32_t*)take(4 * vc); t.out_tail = (uint32_t*)take(4 * vc);
    t.rank2node = (uint32_t*)take(4 * vc); t.node2rank = (uint32_t*)take(4 * vc); t.stack = (uint32_t*)take(4 * sc);
    t.score = (int32_t*)take(4 * vc); t.pred = (int32_t*)take(4 * vc);
    t.row_meta = (uint32_t*)take(4 * vc); t.row_pred_off = (uint32_t*)take(4 * vc + 4);
    t.pred_rank = (uint32_t*)take(4 * ec); t.pred_w = (int32_t*)take(4 * ec);
    t.nrec = (uint4*)take(16 * vc); t.nrec2 = (uint4*)take(16 * vc);
    t.e_from = (uint32_t*)take(4 * ec); t.e_to = (uint32_t*)take(4 * ec); t.e_next_in = (uint32_t*)take(4 * ec); t.e_next_out = (uint32_t*)take(4 * ec);
    t.e_w = (int32_t*)take(4 * ec);
    t.aln_node = (int32_t*)take(4 * ac); t.aln_pos = (int32_t*)take(4 * ac);
    uint32_t* p = (uint32_t*)take(4 * (uint64_t)(lmax + 1));
    uint32_t* c = (uint32_t*)take(4 * (uint64_t)(lmax + 1));
    t.vcap = (uint32_t)T; t.ecap = (uint32_t)(T + nseq);
    if (g) { *g = t; *path = p; *colref = c; }
    return off;
}

// block-wide exclusive sum of v (every thread calls it; s_scan holds NT / 64 words); returns the prefix, *total the sum
template <int NT>
__device__ __forceinline__ uint32_t block_excl_sum(uint32_t v, uint32_t* s_scan, uint32_t* total) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t incl = wave_scan_add(v);
    if (lane == 63) s_scan[w] = incl;
    __syncthreads();
    uint32_t pre = 0, tot = 0;
    for (uint32_t q = 0; q < NT / 64; q++) { const uint32_t x = s_scan[q]; pre += q < w ? x : 0u; tot += x; }
    __syncthreads();
    *total = tot;
    return pre + incl - v;
}

// spoa's rank order after an add (serial DFS, thread 0) and the rows the DP and the heaviest bundle read: per rank the node's base, sink
// bit and in-degree (row_meta), the ranks and weights of its in-edge sources in in-edge order (row_pred_off / pred_rank / pred_w)
template <int NT>
__device__ void order_rows(G& g, const uint32_t V, uint32_t* s_scan) {
    const uint32_t t = threadIdx.x;
    for (uint32_t i = t; i < V; i += NT) { g.mark[i] = 0; g.check[i] = 1; }
    __syncthreads();
    if (t == 0) toposort(g, V, g.rank2node);
    __syncthreads();
    for (uint32_t r = t; r < V; r += NT) g.node2rank[g.rank2node[r]] = r;
    __syncthreads();
    uint32_t carry = 0;
    for (uint32_t b = 0; b < V; b += NT) {
        const uint32_t r = b + t;
        uint32_t np = 0;
        if (r < V) {
            const uint32_t n = g.rank2node[r];
            for (uint32_t e = g.in_head[n]; e != NONE; e = g.e_next_in[e]) np++;
            g.row_meta[r] = (uint32_t)g.code[n] | (g.out_head[n] == NONE ? 4u : 0u) | (np << META_NP);
        }
        uint32_t tot;
        const uint32_t pre = block_excl_sum<NT>(np, s_scan, &tot);
        if (r < V) {
            uint32_t o = carry + pre;
            g.row_pred_off[r] = o;
            for (uint32_t e = g.in_head[g.rank2node[r]]; e != NONE; e = g.e_next_in[e], o++) { g.pred_rank[o] = g.node2rank[g.e_from[e]]; g.pred_w[o] = g.e_w[e]; }
        }
        carry += tot;
    }
    if (t == 0) g.row_pred_off[V] = carry;
    __syncthreads();
}

struct Shared { uint32_t item, V, E, fail; int best; unsigned long long key; };

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

// ---- MSA output (DESIGN.md "General POA path", "MSA output") ----
// The columns of spoa's generate_multiple_sequence_alignment on the final rank order (order_rows leaves aligned nodes contiguous): rank r
// opens a column iff none of its node's aligned nodes has a smaller rank, and the column of a rank is the number of openers up to it, less
// one. colr (by rank) receives them; returns the number of columns. All lanes.
template <int NT>
__device__ uint32_t msa_columns(const G& g, const uint32_t V, uint32_t* colr, uint32_t* s_scan) {
    const uint32_t t = threadIdx.x;
    uint32_t carry = 0;
    for (uint32_t b = 0; b < V; b += NT) {
        const uint32_t r = b + t;
        uint32_t opens = 0;
        if (r < V) {
            const uint32_t n = g.rank2node[r], na = g.n_aligned[n];
            opens = 1;
            for (uint32_t k = 0; k < na; k++) if (g.node2rank[g.aligned[3 * n + k]] < r) opens = 0;
        }
        uint32_t tot;
        const uint32_t pre = block_excl_sum<NT>(opens, s_scan, &tot);
        if (r < V) colr[r] = carry + pre + opens - 1u;   // (rank 0 always opens: never below 0)
        carry += tot;
    }
    __syncthreads();
    return carry;
}

// consensus_wave of poa_graph.inl (k_poa uses that one, so it stays as it is) that also hands back the rank the walk back starts from:
// the ranks of the consensus nodes are that rank and its chain of g.pred
__device__ uint32_t consensus_wave_end(G& g, const uint32_t V, char* out, uint32_t* end_rank) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t best, nbest;
    bundle_pass(g, V, 0, false, -1, best, nbest);
    if (best == NONE) best = g.node2rank[0];
    for (uint32_t round = 0; !(g.row_meta[best] & 4u) && round <= V; round++) {
        const uint32_t n0 = g.rank2node[best];
        if (lane == 0)
            for (uint32_t e = g.out_head[n0]; e != NONE; e = g.e_next_out[e])
                for (uint32_t oe = g.in_head[g.e_to[e]]; oe != NONE; oe = g.e_next_in[oe])
                    if (g.e_from[oe] != n0) g.score[g.node2rank[g.e_from[oe]]] = -1;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        uint32_t nb;
        bundle_pass(g, V, best + 1, true, 0, nb, nbest);
        best = nb == NONE ? g.node2rank[0] : nb;
    }
    *end_rank = best;
    return bundle_backtrack(g, best, out);
}

// the columns of the len consensus bases, by the first wavefront: bundle_backtrack's walk (64 ranks around the walk fetched at once, the
// walk inside them on v_readlane) with the rank's column in place of its base; back to front in rev, then turned round by all lanes
__device__ void consensus_columns(const G& g, const uint32_t end_rank, const uint32_t len, const uint32_t* colr, uint32_t* rev, uint32_t* out) {
    const uint32_t lane = threadIdx.x & 63u;
    const int32_t* pr_r = g.pred;
    int32_t r = __builtin_amdgcn_readfirstlane((int)end_rank);
    uint32_t k = 0;
    int acc = 0;
    while (r != -1 && k < len) {
        const uint32_t cb = (uint32_t)r & ~63u, idx = min(cb + lane, (uint32_t)r);
        const int p = pr_r[idx], c = (int)colr[idx];
        while (r >= (int32_t)cb && k < len) {
            const int l = r - (int32_t)cb;
            const int cl = __builtin_amdgcn_readlane(c, l);
            acc = lane == (k & 63u) ? cl : acc;
            k++;
            if ((k & 63u) == 0) rev[k - 64 + lane] = (uint32_t)acc;
            r = __builtin_amdgcn_readlane(p, l);
        }
    }
    if (lane < (k & 63u)) rev[(k & ~63u) + lane] = (uint32_t)acc;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    for (uint32_t q = lane; q < k; q += 64) out[q] = rev[k - 1 - q];
}

// The row text of one call, grid-wide: a wavefront takes 64 consecutive bases of one row. Columns rise strictly along a row, so lane i
// writes the gaps between the previous base's column and its own, then its base: one nearly contiguous span per wavefront, every byte of
// the output written exactly once (no fill pass). The gaps before a row's first base and after its last one can be long: the whole
// wavefront writes those. A row without bases (an empty sequence) is one chunk that writes ncols gaps.
__global__ __launch_bounds__(256) void k_msa_rows(const MRow* rows, const uint2* chunks, const uint32_t n_chunks, const uint32_t* base_col, const uint8_t* codes,
                                                  const uint32_t* cns_col, const char* cns, char* out) {
    const uint32_t w = (blockIdx.x * 256u + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (w >= n_chunks) return;
    const uint2 ch = chunks[w];
    const MRow R = rows[ch.x];
    const uint32_t* col = (R.is_cns ? cns_col : base_col) + R.src;
    char* row = out + R.dst;
    const uint32_t i = ch.y + lane;
    if (i < R.len) {
        const uint32_t c = col[i];
        const uint32_t from = i ? col[i - 1] + 1u : c;   // (the gaps before the first base: below, by all lanes)
        if (c < R.ncols && from <= c) {                   // (always true for the columns run_set leaves: the guard keeps a store inside the row)
            for (uint32_t q = from; q < c; q++) row[q] = '-';
            row[c] = R.is_cns ? cns[R.src + i] : "ACGT"[codes[R.src + i] & 3];
        }
    }
    if (ch.y == 0 && R.len) { const uint32_t c0 = min(col[0], R.ncols); for (uint32_t q = lane; q < c0; q += 64) row[q] = '-'; }
    if (ch.y + 64 >= R.len) {
        const uint32_t after = R.len ? col[R.len - 1] + 1u : 0u;
        for (uint32_t q = after + lane; q < R.ncols; q += 64) row[q] = '-';
    }
}

// ---- base weights and coverage (DESIGN.md "General POA path", "Base weights and coverage") ----
// spoa's weighted add_alignment, applied beside the unit-weight one: the sequence walks the edge path[i-1] -> path[i] for every pair of
// consecutive bases (prefix chain, aligned part, suffix chain alike) and add_alignment has given each of them 2; what is missing to spoa's
// w[i-1] + w[i] is added here, by all lanes. The nodes of one sequence are distinct (its columns rise strictly), so no two lanes meet on an
// edge. The edge is looked up in the out-list of path[i-1], as add_edge does.
template <int NT>
__device__ void weigh_path(G& g, const uint32_t* path, const uint8_t* w, const uint32_t L) {
    for (uint32_t i = threadIdx.x + 1; i < L; i += NT) {
        const int32_t extra = (int32_t)w[i - 1] + (int32_t)w[i] - 2;
        if (extra == 0) continue;
        const uint32_t to = path[i];
        for (uint32_t e = g.out_head[path[i - 1]]; e != NONE; e = g.e_next_out[e])
            if (g.e_to[e] == to) { g.e_w[e] += extra; break; }
    }
}

// one sequence of >= 2 bases (k_cov_hist: src = its first base, hoff = the first column of its set among all columns of the call) or one
// consensus (k_cov_gather: src = its place beside the device's consensus text, dst = its place in the output)
struct CRow { uint64_t src, dst, hoff; uint32_t len, ncols; };

// The number of bases per column (stride 1) or per column and letter (stride 4) of one call, grid-wide: a wavefront takes 64 consecutive
// bases of one sequence. Columns rise strictly along a sequence, so the lanes of a wavefront never meet on a counter; different sequences
// of a set do, hence the atomic.
__global__ __launch_bounds__(256) void k_cov_hist(const CRow* rows, const uint2* chunks, const uint32_t n_chunks, const uint32_t* base_col, const uint8_t* codes,
                                                  const uint32_t stride, uint32_t* hist) {
    const uint32_t w = (blockIdx.x * 256u + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (w >= n_chunks) return;
    const uint2 ch = chunks[w];
    const CRow R = rows[ch.x];
    const uint32_t i = ch.y + lane;
    if (i >= R.len) return;
    const uint32_t c = base_col[R.src + i];
    if (c >= R.ncols) return;   // (never true for the columns run_set leaves: the guard keeps the add inside the set's counters)
    atomicAdd(&hist[(R.hoff + c) * stride + (stride == 4 ? (uint32_t)(codes[R.src + i] & 3) : 0u)], 1u);
}

// coverage (and the four letter counts) of every consensus base: the counters of its column. A wavefront takes 64 consecutive bases of
// one consensus; cov / prof are in the output's layout (consensus strings back to back).
__global__ __launch_bounds__(256) void k_cov_gather(const CRow* rows, const uint2* chunks, const uint32_t n_chunks, const uint32_t* cns_col, const uint32_t* hist,
                                                    const uint32_t stride, uint32_t* cov, uint32_t* prof) {
    const uint32_t w = (blockIdx.x * 256u + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (w >= n_chunks) return;
    const uint2 ch = chunks[w];
    const CRow R = rows[ch.x];
    const uint32_t i = ch.y + lane;
    if (i >= R.len) return;
    const uint32_t c = cns_col[R.src + i];
    uint32_t n[4] = {0, 0, 0, 0};
    if (c < R.ncols) {
        const uint32_t* h = hist + (R.hoff + c) * stride;
        n[0] = h[0];
        if (stride == 4) { n[1] = h[1]; n[2] = h[2]; n[3] = h[3]; }
    }
    cov[R.dst + i] = n[0] + n[1] + n[2] + n[3];
    if (prof) { uint32_t* p = prof + 4 * (R.dst + i); p[0] = n[0]; p[1] = n[1]; p[2] = n[2]; p[3] = n[3]; }
}

template <int NT, int CPL, bool AFF = false, bool MSA = false, bool WTS = false>
__device__ void run_set(const MArgs& a, const uint32_t set, uint8_t* slot, Shared& sh, int* s_wtot, uint32_t* s_scan) {
    const uint32_t t = threadIdx.x;
    const MSet S = a.sets[set];
    G g; uint32_t *path, *colref;
    const uint64_t pools = carve_pools(slot, S.sum_len, S.nseq, S.lmax, &g, &path, &colref);
    if (pools > a.slot_bytes) { if (t == 0) a.status[set] = MS_GRAPH_OVERFLOW; return; }
    int32_t* H = (int32_t*)(slot + pools);
    const uint64_t hcap = (a.slot_bytes - pools) / (AFF ? 8 : 4);   // cells the slot holds (affine: an (H, F) pair each)
    uint32_t V = 0, E = 0, non_empty = 0;
    unsigned long long cells = 0;
    for (uint32_t k = 0; k < S.nseq; k++) {
        const uint64_t b = a.soff[S.seq_begin + k];
        const uint32_t L = (uint32_t)(a.soff[S.seq_begin + k + 1] - b);
        if (L == 0) continue;
        const uint8_t* s = a.codes + b;
        non_empty++;
        uint32_t na = 0;
        if (V) {
            if ((uint64_t)(V + 1) * (L + 1) > hcap) { if (t == 0) { a.status[set] = MS_H_OVERFLOW; a.vseen[set] = V; } return; }
            cells += (unsigned long long)V * L;
            uint32_t bi, bj;
            if (AFF) {
                dp_rows_affine<NT, CPL>(g, (int2*)H, V, s, L, a, sh, s_wtot, &bi, &bj);
                if (t == 0 && bi) na = traceback_affine(g, (const int2*)H, s, L, bi, bj, a);
            } else {
                dp_rows<NT, CPL>(g, H, V, s, L, a, sh, s_wtot, &bi, &bj);
                if (t == 0 && bi) na = traceback(g, H, s, L, bi, bj, a);
            }
        }
        if (t == 0) {
            uint32_t v = V, e = E;
            const bool ok = add_alignment(g, v, e, na, s, L, path, colref);
            sh.V = v; sh.E = e; sh.fail = !ok;
        }
        __syncthreads();
        V = sh.V; E = sh.E;
        if (sh.fail) { if (t == 0) a.status[set] = MS_GRAPH_OVERFLOW; return; }
        if (MSA) for (uint32_t i = t; i < L; i += NT) a.base_col[b + i] = path[i];   // (node ids never change: a rerun set rewrites its part)
        if (WTS) weigh_path<NT>(g, path, a.wts + b, L);   // (order_rows reads e_w behind its barriers)
        order_rows<NT>(g, V, s_scan);
    }
    if (MSA) {
        // columns by rank into the DFS stack's pool (free after the last sort), then every base of the set from its node to its column
        uint32_t* colr = g.stack;
        const uint32_t ncols = msa_columns<NT>(g, V, colr, s_scan);
        const uint64_t b0 = a.soff[S.seq_begin];
        for (uint64_t i = t; i < S.sum_len; i += NT) a.base_col[b0 + i] = colr[g.node2rank[a.base_col[b0 + i]]];
        if (t < 64) {
            uint32_t len = 0, end_rank = 0;
            if (non_empty) {
                len = consensus_wave_end(g, V, a.cns + S.cns_off, &end_rank);
                if (a.cns_col) consensus_columns(g, end_rank, len, colr, (uint32_t*)g.aln_pos, a.cns_col + S.cns_off);
            }
            if (t == 0) { a.cns_len[set] = len; a.n_cols[set] = ncols; a.cells[set] = cells; a.status[set] = MS_OK; }
        }
    } else if (t < 64) {
        const uint32_t len = non_empty ? consensus_wave(g, V, a.cns + S.cns_off) : 0u;
        if (t == 0) { a.cns_len[set] = len; a.cells[set] = cells; a.status[set] = MS_OK; }
    }
    __syncthreads();   // the slot is free for the next set
}

template <int NT, int CPL, bool MSA = false, bool WTS = false>
__global__ __launch_bounds__(NT) void k_poa_modes(MArgs a) {
    __shared__ Shared sh;
    __shared__ int s_wtot[NT / 64];
    __shared__ uint32_t s_scan[NT / 64];
    uint8_t* slot = a.ws + (size_t)blockIdx.x * a.slot_bytes;
    for (;;) {
        if (threadIdx.x == 0) sh.item = atomicAdd(a.counter, 1u);
        __syncthreads();
        const uint32_t q = sh.item;
        __syncthreads();
        if (q >= a.n_items) return;
        run_set<NT, CPL, false, MSA, WTS>(a, a.order[q], slot, sh, s_wtot, s_scan);
    }
}

template <int NT, int CPL, bool MSA = false, bool WTS = false>
__global__ __launch_bounds__(NT) void k_poa_affine(MArgs a) {
    __shared__ Shared sh;
    __shared__ int s_wtot[NT / 64];
    __shared__ uint32_t s_scan[NT / 64];
    uint8_t* slot = a.ws + (size_t)blockIdx.x * a.slot_bytes;
    for (;;) {
        if (threadIdx.x == 0) sh.item = atomicAdd(a.counter, 1u);
        __syncthreads();
        const uint32_t q = sh.item;
        __syncthreads();
        if (q >= a.n_items) return;
        run_set<NT, CPL, true, MSA, WTS>(a, a.order[q], slot, sh, s_wtot, s_scan);
    }
}

// the instances: workgroup lanes x columns per lane; a set goes to the first whose NT x CPL columns hold its longest sequence + 1.
// Each has a twin that also records the MSA (a template flag: a consensus-only call runs the code it ran before the MSA existed), and a
// second twin that records the MSA and applies base weights (hx_poa_weighted with weights; coverage needs the node of every base anyway).
struct Inst { int nt, cpl; const void* fn; const void* fn_msa; const void* fn_w; };
const Inst kInst[] = {
    {64, 16, (const void*)k_poa_modes<64, 16>, (const void*)k_poa_modes<64, 16, true>, (const void*)k_poa_modes<64, 16, true, true>},
    {256, 16, (const void*)k_poa_modes<256, 16>, (const void*)k_poa_modes<256, 16, true>, (const void*)k_poa_modes<256, 16, true, true>},
    {256, 32, (const void*)k_poa_modes<256, 32>, (const void*)k_poa_modes<256, 32, true>, (const void*)k_poa_modes<256, 32, true, true>},
    {1024, 32, (const void*)k_poa_modes<1024, 32>, (const void*)k_poa_modes<1024, 32, true>, (const void*)k_poa_modes<1024, 32, true, true>},
};
constexpr int N_INST = sizeof(kInst) / sizeof(kInst[0]);
constexpr uint32_t MAX_LEN = 1024 * 32 - 1;
// the affine instances keep two accumulators per column (diagonal and F): 16 columns per lane throughout, more lanes instead
const Inst kInstAffine[N_INST] = {
    {64, 16, (const void*)k_poa_affine<64, 16>, (const void*)k_poa_affine<64, 16, true>, (const void*)k_poa_affine<64, 16, true, true>},
    {256, 16, (const void*)k_poa_affine<256, 16>, (const void*)k_poa_affine<256, 16, true>, (const void*)k_poa_affine<256, 16, true, true>},
    {512, 16, (const void*)k_poa_affine<512, 16>, (const void*)k_poa_affine<512, 16, true>, (const void*)k_poa_affine<512, 16, true, true>},
    {1024, 16, (const void*)k_poa_affine<1024, 16>, (const void*)k_poa_affine<1024, 16, true>, (const void*)k_poa_affine<1024, 16, true, true>},
};
constexpr uint32_t MAX_LEN_AFFINE = 1024 * 16 - 1;

template <class T> struct Buf {   // device buffer of one call
    T* p = nullptr;
    hipError_t alloc(size_t n) { return hipMalloc((void**)&p, std::max<size_t>(n, 1) * sizeof(T)); }
    ~Buf() { if (p) (void)hipFree(p); }
};

}  // namespace

#define MCHK(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) { err = std::string(#expr) + ": " + hipGetErrorString(e_); return -1; } } while (0)

int poa_modes_run(hipStream_t s, PoaModesWs& ws, const PoaModesArgs& a, PoaModesOut& o, std::string& err) {
    const uint32_t ns = a.n_sets;
    const bool aff = a.affine != 0;
    const Inst* const inst = aff ? kInstAffine : kInst;
    const uint32_t max_len = aff ? MAX_LEN_AFFINE : MAX_LEN;
    const uint64_t cell_bytes = aff ? 8 : 4;   // affine: an (H, F) pair per cell
    const bool msa = a.msa != 0;
    const bool wtd = a.weighted != 0;                        // hx_poa_weighted: the node of every base is kept, as for the MSA
    const bool cols = msa || wtd;
    const bool want_cov = wtd && (a.want_coverage || a.want_profile);
    const std::string who = wtd ? "hx_poa_weighted" : msa ? "hx_poa_msa" : aff ? "hx_poa_sequences_affine" : "hx_poa_sequences_mode";
    const uint64_t nseq = a.set_off[ns], nb = a.seq_off[nseq];
    std::vector<MSet> sets(ns);
    std::vector<uint64_t> cns_off((size_t)ns + 1, 0);
    o = PoaModesOut();
    for (uint32_t i = 0; i < ns; i++) {
        MSet& S = sets[i];
        S.seq_begin = a.set_off[i]; S.nseq = (uint32_t)(a.set_off[i + 1] - a.set_off[i]); S.sum_len = 0; S.lmax = 0;
        for (uint64_t k = a.set_off[i]; k < a.set_off[i + 1]; k++) {
            const uint64_t L = a.seq_off[k + 1] - a.seq_off[k];
            if (L > max_len) { err = who + ": set " + std::to_string(i) + " holds a sequence of " + std::to_string(L) + " bases, longer than " + std::to_string(max_len) + (aff ? " (the longest the general POA path takes with affine gaps)" : " (the longest the general POA path takes)"); return -1; }
            S.sum_len += L; S.lmax = std::max(S.lmax, (uint32_t)L);
            o.seq_bases += L; o.n_aligned += L != 0;
        }
        if (S.sum_len > MAX_SET_BASES) { err = who + ": set " + std::to_string(i) + " holds " + std::to_string(S.sum_len) + " bases in all, more than the " + std::to_string(MAX_SET_BASES) + " nodes a graph can have"; return -1; }
        S.cns_off = cns_off[i]; cns_off[i + 1] = cns_off[i] + S.sum_len;   // (a consensus has at most one base per node)
    }
    std::vector<uint8_t> codes(std::max<uint64_t>(1, nb));
    for (uint64_t k = 0; k < nb; k++) { const char c = a.bases[k]; codes[k] = c == 'C' || c == 'c' ? 1 : c == 'G' || c == 'g' ? 2 : c == 'T' || c == 't' ? 3 : 0; }
    int dev = 0, n_cu = 0;
    MCHK(hipGetDevice(&dev));
    MCHK(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev));
    Buf<MSet> d_sets; Buf<uint8_t> d_codes; Buf<uint64_t> d_soff; Buf<uint32_t> d_order, d_counter, d_status, d_vseen, d_cns_len; Buf<unsigned long long> d_cells; Buf<char> d_cns;
    MCHK(d_sets.alloc(ns)); MCHK(d_codes.alloc(codes.size())); MCHK(d_soff.alloc(nseq + 1)); MCHK(d_order.alloc(ns)); MCHK(d_counter.alloc(N_INST));
    MCHK(d_status.alloc(ns)); MCHK(d_vseen.alloc(ns)); MCHK(d_cns_len.alloc(ns)); MCHK(d_cells.alloc(ns)); MCHK(d_cns.alloc(cns_off[ns]));
    MCHK(hipMemcpyAsync(d_sets.p, sets.data(), ns * sizeof(MSet), hipMemcpyHostToDevice, s));
    MCHK(hipMemcpyAsync(d_codes.p, codes.data(), codes.size(), hipMemcpyHostToDevice, s));
    MCHK(hipMemcpyAsync(d_soff.p, a.seq_off, (nseq + 1) * 8, hipMemcpyHostToDevice, s));
    MCHK(hipMemsetAsync(d_cns_len.p, 0, std::max<size_t>(1, ns) * 4, s));
    MCHK(hipMemsetAsync(d_cells.p, 0, std::max<size_t>(1, ns) * 8, s));
    Buf<uint32_t> d_base_col, d_n_cols, d_cns_col;   // MSA and weighted calls only
    if (cols) {
        MCHK(d_base_col.alloc(nb)); MCHK(d_n_cols.alloc(ns));
        MCHK(hipMemsetAsync(d_n_cols.p, 0, std::max<size_t>(1, ns) * 4, s));
        if (msa ? a.include_consensus != 0 : want_cov) MCHK(d_cns_col.alloc(cns_off[ns]));
    }
    Buf<uint8_t> d_wts;                              // weighted calls with weights only: a byte per base
    if (wtd && a.weights) {
        MCHK(d_wts.alloc(nb));
        MCHK(hipMemcpyAsync(d_wts.p, a.weights, nb, hipMemcpyHostToDevice, s));
    }
    auto fn_of = [&](int k) { return d_wts.p ? inst[k].fn_w : cols ? inst[k].fn_msa : inst[k].fn; };

    // H is sized from an estimate of the graph's final size (noisy copies add about a tenth of their length each); a set that outgrows its
    // slot comes back and is rerun with twice the room (or the room for what it had when it stopped, doubled), the worst case at most
    std::vector<uint64_t> vest(ns);
    std::vector<uint32_t> todo;
    for (uint32_t i = 0; i < ns; i++) { vest[i] = std::min<uint64_t>(sets[i].sum_len, sets[i].lmax + sets[i].sum_len / 8 + 64); if (sets[i].sum_len) todo.push_back(i); }
    auto need = [&](uint32_t i) { const MSet& S = sets[i]; return carve_pools(nullptr, S.sum_len, S.nseq, S.lmax, nullptr, nullptr, nullptr) + al256((vest[i] + 1) * (uint64_t)(S.lmax + 1) * cell_bytes); };
    auto inst_of = [&](uint32_t i) { int k = 0; while ((uint64_t)inst[k].nt * inst[k].cpl < (uint64_t)sets[i].lmax + 1) k++; return k; };
    uint64_t budget;
    {
        size_t fr = 0, tot = 0;
        MCHK(hipMemGetInfo(&fr, &tot));
        budget = a.workspace_gb > 0 ? (uint64_t)(a.workspace_gb * 1e9) : (uint64_t)((double)(fr + ws.cap) * 0.4);
    }
    hipEvent_t e0, e1;
    MCHK(hipEventCreate(&e0)); MCHK(hipEventCreate(&e1));
    struct EvGuard { hipEvent_t a, b; ~EvGuard() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); } } evg{e0, e1};
    std::vector<uint32_t> status(ns), vseen(ns);
    for (bool first = true; !todo.empty(); first = false) {
        // plan the round: per instance, its sets costliest first, one slot size (the largest need), as many slots as are resident and fit the budget
        std::vector<std::vector<uint32_t>> by(N_INST);
        for (uint32_t i : todo) by[inst_of(i)].push_back(i);
        std::vector<uint64_t> slot(N_INST, 0), base(N_INST, 0);
        std::vector<uint32_t> nslots(N_INST, 0);
        std::vector<uint32_t> order;
        uint64_t total = 0;
        for (int k = 0; k < N_INST; k++) {
            auto& v = by[k];
            if (v.empty()) continue;
            std::stable_sort(v.begin(), v.end(), [&](uint32_t x, uint32_t y) { return sets[x].sum_len * sets[x].lmax > sets[y].sum_len * sets[y].lmax; });
            uint64_t sb = 0, pmax = 0;
            uint32_t big = v[0];
            for (uint32_t i : v) {
                const uint64_t nd = need(i);
                if (nd > sb) { sb = nd; big = i; }
                pmax = std::max(pmax, carve_pools(nullptr, sets[i].sum_len, sets[i].nseq, sets[i].lmax, nullptr, nullptr, nullptr));
            }
            if (first && a.slot_kb_cap) sb = std::max(pmax, std::min<uint64_t>(sb, (uint64_t)a.slot_kb_cap << 10));   // (test switch: forces the overflow and rerun)
            sb = al256(sb);
            int occ = 0;
            MCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn_of(k), inst[k].nt, 0));
            const uint64_t resident = (uint64_t)std::max(1, occ) * (uint64_t)n_cu;
            const uint64_t fit = budget / sb;
            if (fit == 0) { err = who + ": set " + std::to_string(big) + " needs " + std::to_string(sb) + " bytes of workspace, more than the budget of " + std::to_string(budget) + " (option poa_workspace_gb)"; return -1; }
            slot[k] = sb; nslots[k] = (uint32_t)std::min<uint64_t>({(uint64_t)v.size(), resident, fit});
            base[k] = order.size();
            order.insert(order.end(), v.begin(), v.end());
            total = std::max(total, nslots[k] * sb);   // (the instances run one after the other on the stream: they share the workspace)
        }
        if (total > ws.cap) {
            MCHK(hipStreamSynchronize(s));
            ws.release();
            const hipError_t e = hipMalloc(&ws.p, total);
            if (e != hipSuccess) { ws.p = nullptr; err = who + ": the workspace of " + std::to_string(total) + " bytes could not be allocated: " + hipGetErrorString(e); return -1; }
            ws.cap = total;
        }
        MCHK(hipMemcpyAsync(d_order.p, order.data(), order.size() * 4, hipMemcpyHostToDevice, s));
        MCHK(hipMemsetAsync(d_counter.p, 0, N_INST * 4, s));
        MCHK(hipMemsetAsync(d_status.p, 0xff, std::max<size_t>(1, ns) * 4, s));
        MCHK(hipEventRecord(e0, s));
        for (int k = 0; k < N_INST; k++) {
            if (by[k].empty()) continue;
            MArgs q{d_sets.p, d_order.p + base[k], (uint32_t)by[k].size(), d_counter.p + k, d_codes.p, d_soff.p, (uint8_t*)ws.p, slot[k],
                    a.match, a.mismatch, a.gap, a.type, d_cns.p, d_cns_len.p, d_status.p, d_vseen.p, d_cells.p, a.gap_extend,
                    d_base_col.p, d_n_cols.p, d_cns_col.p, d_wts.p};
            void* kargs[] = {&q};
            MCHK(hipLaunchKernel(fn_of(k), dim3(nslots[k]), dim3((uint32_t)inst[k].nt), kargs, 0, s));
            o.launches++;
            if (a.debug) fprintf(stderr, "[hx] POA modes%s: %zu sets on %u workgroups of %d lanes x %d columns, slots of %.1f MB\n", aff ? " (affine)" : "", by[k].size(), nslots[k], inst[k].nt, inst[k].cpl, slot[k] / 1e6);
        }
        MCHK(hipEventRecord(e1, s));
        MCHK(hipEventSynchronize(e1));
        float ms = 0;
        MCHK(hipEventElapsedTime(&ms, e0, e1));
        o.kernel_ms += ms;
        MCHK(hipMemcpy(status.data(), d_status.p, ns * 4, hipMemcpyDeviceToHost));
        MCHK(hipMemcpy(vseen.data(), d_vseen.p, ns * 4, hipMemcpyDeviceToHost));
        std::vector<uint32_t> next;
        for (uint32_t i : todo) {
            if (status[i] == MS_OK) continue;
            const bool capped = first && a.slot_kb_cap;   // (a capped slot can be short of even the worst case)
            if (status[i] != MS_H_OVERFLOW || (vest[i] >= sets[i].sum_len && !capped)) { err = who + ": set " + std::to_string(i) + " failed on the device (status " + std::to_string((int)status[i]) + ")"; return -1; }
            vest[i] = std::min<uint64_t>(sets[i].sum_len, std::max<uint64_t>(2 * vest[i], 2 * (uint64_t)vseen[i] + 64));
            next.push_back(i);
            o.retried++;
        }
        todo.swap(next);
    }
    std::vector<uint32_t> len(ns);
    std::vector<unsigned long long> cells(ns);
    std::vector<char> cns(std::max<uint64_t>(1, cns_off[ns]));
    MCHK(hipMemcpy(len.data(), d_cns_len.p, ns * 4, hipMemcpyDeviceToHost));
    MCHK(hipMemcpy(cells.data(), d_cells.p, ns * 8, hipMemcpyDeviceToHost));
    MCHK(hipMemcpy(cns.data(), d_cns.p, cns_off[ns], hipMemcpyDeviceToHost));
    o.cns_off.assign((size_t)ns + 1, 0);
    for (uint32_t i = 0; i < ns; i++) {
        o.cns.append(cns.data() + cns_off[i], len[i]);
        o.cns_off[i + 1] = o.cns.size();
        o.cells += cells[i];
    }
    if (want_cov) {
        // coverage and profile: now that the columns of every set are known, one counter per column (four with the profile: one per
        // letter) for the whole call, filled from the bases of the sequences of >= 2 bases (k_cov_hist), then read at the columns of the
        // consensus bases (k_cov_gather). Built here, after the last round: a set that was rerun is counted once.
        const uint32_t stride = a.want_profile ? 4u : 1u;
        std::vector<uint32_t> ncols(ns);
        MCHK(hipMemcpy(ncols.data(), d_n_cols.p, ns * 4, hipMemcpyDeviceToHost));
        std::vector<CRow> rows, crows;
        std::vector<uint2> chunks, cchunks;
        uint64_t hoff = 0, hist_bases = 0;
        for (uint32_t i = 0; i < ns; i++) {
            for (uint64_t k = a.set_off[i]; k < a.set_off[i + 1]; k++) {
                const uint32_t L = (uint32_t)(a.seq_off[k + 1] - a.seq_off[k]);
                if (L < 2) continue;   // (spoa counts the sequence labels of a node's edges: a sequence of one base has none)
                for (uint32_t f = 0; f < L; f += 64) chunks.push_back(make_uint2((uint32_t)rows.size(), f));
                rows.push_back(CRow{a.seq_off[k], 0, hoff, L, ncols[i]});
                hist_bases += L;
            }
            if (len[i]) {
                for (uint32_t f = 0; f < len[i]; f += 64) cchunks.push_back(make_uint2((uint32_t)crows.size(), f));
                crows.push_back(CRow{cns_off[i], o.cns_off[i], hoff, len[i], ncols[i]});
            }
            hoff += ncols[i];
        }
        if (rows.size() >= 0xffffffffULL || crows.size() >= 0xffffffffULL || chunks.size() >= 0xffffffffULL / 64 || cchunks.size() >= 0xffffffffULL / 64) { err = who + ": too many sequences"; return -1; }
        const uint64_t nc = o.cns.size();
        o.cov.assign(nc, 0);
        if (a.want_profile) o.prof.assign(4 * nc, 0);
        if (nc) {
            Buf<CRow> d_rows, d_crows; Buf<uint2> d_chunks, d_cchunks; Buf<uint32_t> d_hist, d_cov, d_prof;
            MCHK(d_rows.alloc(rows.size())); MCHK(d_crows.alloc(crows.size())); MCHK(d_chunks.alloc(chunks.size())); MCHK(d_cchunks.alloc(cchunks.size()));
            MCHK(d_hist.alloc(hoff * stride)); MCHK(d_cov.alloc(nc));
            if (a.want_profile) MCHK(d_prof.alloc(4 * nc));
            MCHK(hipMemcpyAsync(d_rows.p, rows.data(), rows.size() * sizeof(CRow), hipMemcpyHostToDevice, s));
            MCHK(hipMemcpyAsync(d_crows.p, crows.data(), crows.size() * sizeof(CRow), hipMemcpyHostToDevice, s));
            MCHK(hipMemcpyAsync(d_chunks.p, chunks.data(), chunks.size() * sizeof(uint2), hipMemcpyHostToDevice, s));
            MCHK(hipMemcpyAsync(d_cchunks.p, cchunks.data(), cchunks.size() * sizeof(uint2), hipMemcpyHostToDevice, s));
            MCHK(hipEventRecord(e0, s));
            MCHK(hipMemsetAsync(d_hist.p, 0, std::max<uint64_t>(1, hoff * stride) * 4, s));
            if (!chunks.empty()) {
                k_cov_hist<<<(uint32_t)((chunks.size() + 3) / 4), 256, 0, s>>>(d_rows.p, d_chunks.p, (uint32_t)chunks.size(), d_base_col.p, d_codes.p, stride, d_hist.p);
                MCHK(hipGetLastError());
                o.launches++;
            }
            k_cov_gather<<<(uint32_t)((cchunks.size() + 3) / 4), 256, 0, s>>>(d_crows.p, d_cchunks.p, (uint32_t)cchunks.size(), d_cns_col.p, d_hist.p, stride, d_cov.p, d_prof.p);
            MCHK(hipGetLastError());
            MCHK(hipEventRecord(e1, s));
            MCHK(hipEventSynchronize(e1));
            float cov_ms = 0;
            MCHK(hipEventElapsedTime(&cov_ms, e0, e1));
            o.cov_ms = cov_ms; o.kernel_ms += cov_ms; o.launches++;
            // what the two kernels and the clearing of the counters must move: a column (and a letter) read per counted base, the
            // counters written twice and read once where a consensus base stands, a column read and the counts written per consensus base
            o.cov_moved_bytes = hist_bases * (4 + (stride == 4 ? 1 : 0)) + 2 * hoff * stride * 4 + nc * (4 + 4 * stride + 4 + (a.want_profile ? 16 : 0));
            MCHK(hipMemcpy(o.cov.data(), d_cov.p, nc * 4, hipMemcpyDeviceToHost));
            if (a.want_profile) MCHK(hipMemcpy(o.prof.data(), d_prof.p, 4 * nc * 4, hipMemcpyDeviceToHost));
        }
    }
    if (!msa) return 0;

    // the MSA text: now that the columns of every set are known, the rows' places (set i = rows x n_cols bytes, row-major), one descriptor per
    // row and one work item per 64 bases of a row for k_msa_rows
    o.msa_cols.assign(ns, 0);
    MCHK(hipMemcpy(o.msa_cols.data(), d_n_cols.p, ns * 4, hipMemcpyDeviceToHost));
    o.msa_rows.assign(ns, 0);
    o.msa_off.assign((size_t)ns + 1, 0);
    std::vector<MRow> rows;
    std::vector<uint2> chunks;
    auto add_row = [&](uint64_t src, uint64_t dst, uint32_t n, uint32_t ncols, uint32_t is_cns) {
        const uint32_t r = (uint32_t)rows.size();
        rows.push_back(MRow{src, dst, n, ncols, is_cns, 0});
        for (uint32_t f = 0; f == 0 || f < n; f += 64) chunks.push_back(make_uint2(r, f));
    };
    for (uint32_t i = 0; i < ns; i++) {
        const uint32_t nc = o.msa_cols[i];
        uint64_t dst = o.msa_off[i];
        if (nc) {   // (no column: no non-empty sequence, nothing to write)
            for (uint64_t k = a.set_off[i]; k < a.set_off[i + 1]; k++, dst += nc) add_row(a.seq_off[k], dst, (uint32_t)(a.seq_off[k + 1] - a.seq_off[k]), nc, 0);
            if (a.include_consensus) { add_row(cns_off[i], dst, len[i], nc, 1); dst += nc; }
        }
        o.msa_rows[i] = sets[i].nseq + (a.include_consensus ? 1u : 0u);
        o.msa_off[i + 1] = o.msa_off[i] + (uint64_t)o.msa_rows[i] * nc;
    }
    if (rows.size() >= 0xffffffffULL || chunks.size() >= 0xffffffffULL / 64) { err = who + ": too many rows"; return -1; }
    const uint64_t out_bytes = o.msa_off[ns];
    o.msa.resize(out_bytes);
    if (out_bytes == 0) return 0;
    Buf<MRow> d_rows; Buf<uint2> d_chunks; Buf<char> d_out;
    MCHK(d_rows.alloc(rows.size())); MCHK(d_chunks.alloc(chunks.size()));
    {
        const hipError_t e = d_out.alloc(out_bytes);
        if (e != hipSuccess) { err = who + ": the " + std::to_string(out_bytes) + " bytes of the alignment text could not be allocated on the device: " + hipGetErrorString(e); return -1; }
    }
    MCHK(hipMemcpyAsync(d_rows.p, rows.data(), rows.size() * sizeof(MRow), hipMemcpyHostToDevice, s));
    MCHK(hipMemcpyAsync(d_chunks.p, chunks.data(), chunks.size() * sizeof(uint2), hipMemcpyHostToDevice, s));
    MCHK(hipEventRecord(e0, s));
    k_msa_rows<<<(uint32_t)((chunks.size() + 3) / 4), 256, 0, s>>>(d_rows.p, d_chunks.p, (uint32_t)chunks.size(), d_base_col.p, d_codes.p, d_cns_col.p, d_cns.p, d_out.p);
    MCHK(hipGetLastError());
    MCHK(hipEventRecord(e1, s));
    MCHK(hipEventSynchronize(e1));
    float rows_ms = 0;
    MCHK(hipEventElapsedTime(&rows_ms, e0, e1));
    o.msa_rows_ms = rows_ms; o.kernel_ms += rows_ms; o.launches++;
    o.msa_moved_bytes = out_bytes + 4 * (nb + (a.include_consensus ? o.cns.size() : 0));
    MCHK(hipMemcpy(&o.msa[0], d_out.p, out_bytes, hipMemcpyDeviceToHost));
    return 0;
}

}  // namespace hxk
