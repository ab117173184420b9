// poa_modes.hip — the general POA path: spoa's linear-gap engine in its three alignment modes (kSW local, kNW global, kOV overlap) for
// caller-given sequence sets (hx_poa_sequences_mode; DESIGN.md "General POA path" has the semantics and the mapping), and the affine-gap
// engine in the same modes (hx_poa_sequences_affine: same mapping, a cell is the pair (H, F), its own row of the instance table), and the
// two-piece affine ("convex") gap model (hx_poa_sequences_convex: a cell is (H, F, O), 12 bytes, a third row of the table). All of it is
// one kernel template, k_poa_general<NT, CPL, GM, MSA, WTS, GRAPH, STRAND>, GM the gap model.
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
//
// The graph itself and the alignments (hx_poa_graph; DESIGN.md "Graph and alignment output") are a third flag on top of the weighted one: after
// every traceback the workgroup copies the alignment's pairs and the end cell's score into the call's alignment pool, after the last sort it
// writes the set's nodes (code, rank, column), its edges in creation order and the nodes of the consensus, and base_col stays node ids. A
// grid-wide kernel (k_graph_gather) moves all of it into dense arrays once the host knows the sizes. The pool is the one array sized from an
// estimate: a set whose alignments outgrow its share finishes, reports what it needed, and is rerun once with exactly that room.
//
// Strand-ambiguous sets (hx_poa_strand; DESIGN.md "Strand-ambiguous sets") are a fourth flag, over the weighted variant: every sequence after
// a set's first is aligned to the graph reverse-complemented and as given, the orientation with the higher end-cell score is added (ties
// forward; when the reverse complement wins, its DP runs once more so that its H is the one the traceback walks), and everything
// downstream reads the codes and weights as they were added (codes_used / wts_used).
//
// Layout: the DP and traceback of the three gap models are poa_modes_dp.inl, the columns, row text, coverage and the graph output's helpers
// and gather poa_modes_out.inl; this file keeps the work of one set (run_set), the kernel, the instance table and the host driver
// (poa_modes_run, in named stages).
#include <algorithm>
#include <chrono>
#include <memory>
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
enum { GM_LINEAR = 0, GM_AFFINE = 1, GM_CONVEX = 2 };   // PoaModesArgs::gap_model
enum { MS_OK = 0, MS_H_OVERFLOW = 1, MS_GRAPH_OVERFLOW = 2, MS_ALN_OVERFLOW = 3 };   // (3: done, but its alignments outgrew their share of the pool)
constexpr uint32_t MAX_SET_BASES = (1u << 21) - 2;   // node ids are packed in 21 bits (+1) in the node records of poa_graph.inl

struct MSet { uint64_t seq_begin, sum_len, cns_off; uint32_t nseq, lmax; };

// What the graph instances (hx_poa_graph) write beside the consensus. The alignment pool holds the (node, position) pairs of every
// alignment of a set, back to front as the traceback leaves them, one alignment after the other from the set's share on (aln_at, aln_room
// pairs); a set stores nothing beyond its share and reports in aln_need what all of its alignments hold. Per sequence of the call: the
// pairs of its alignment and the score of its end cell. The node and edge arrays need no estimate: a set has at most one node per base and
// one edge per base and sequence, so its nodes start at its first base's global offset and its edges at that offset plus its first
// sequence's index.
struct GraphOutArgs {
    int32_t *aln_node, *aln_pos; const uint64_t* aln_at; const uint32_t* aln_room; uint32_t* aln_need;
    uint32_t* aln_cnt; int32_t* aln_score;
    uint8_t* node_code; uint32_t *node_rank, *node_col, *n_nodes;
    uint32_t *edge_from, *edge_to; int32_t* edge_w; uint32_t* n_edges;
    uint32_t* cns_node;   // beside cns
};

// What the strand instances (hx_poa_strand) read and write beside the rest: every sequence reverse-complemented at its own offset (codes_rc,
// and wts_rc: base i of rc(s) carries the weight of base L-1-i of s), the orientation that was added (codes_used / wts_used: what
// add_alignment, weigh_path and the row, coverage and profile kernels read), and per sequence of the call the choice and the two end-cell
// scores; per set the sequences whose reverse complement won (each cost a third DP pass).
struct StrandArgs {
    const uint8_t *codes_rc, *wts_rc; uint8_t *codes_used, *wts_used;
    uint8_t* reversed; int32_t *score_fwd, *score_rev; uint32_t* third;
};

struct MArgs {
    const MSet* sets; const uint32_t* order; uint32_t n_items; uint32_t* counter;
    const uint8_t* codes; const uint64_t* soff;
    uint8_t* ws; uint64_t slot_bytes;
    int32_t m, n, g, type;
    char* cns; uint32_t *cns_len, *status, *vseen; unsigned long long* cells;
    int32_t e;   // affine and convex instances only: gap extend (g is gap open)
    // MSA instances only: per base of the call (global offset) its node, rewritten to its column when the set is done; columns per set;
    // column of every consensus base beside cns (null: not asked for)
    uint32_t *base_col, *n_cols, *cns_col;
    const uint8_t* wts;   // weighted instances only: the weight of every base of the call (1..255), beside codes
    int32_t q, c;         // convex instances only: gap open and gap extend of the second piece
    GraphOutArgs go;      // graph instances only (poa_modes_out.inl)
    StrandArgs sa;        // strand instances only
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

struct Shared { uint32_t item, V, E, fail; int best; uint32_t na /* graph instances: the pairs the traceback left */; unsigned long long key; };

#include "poa_modes_dp.inl"     // DP and traceback, linear, affine and convex gaps
#include "poa_modes_out.inl"    // MSA columns and row text, base weights, coverage, graph and alignment output

template <int NT, int CPL, int GM, bool MSA, bool WTS, bool GRAPH, bool STRAND>
__device__ void run_set(const MArgs& a, const uint32_t set, uint8_t* slot, Shared& sh, int* s_wtot, uint32_t* s_scan) {
    const uint32_t t = threadIdx.x;
    const MSet S = a.sets[set];
    G g; uint32_t *path, *colref;
    const uint64_t pools = carve_pools(slot, S.sum_len, S.nseq, S.lmax, &g, &path, &colref);
    if (pools > a.slot_bytes) { if (t == 0) a.status[set] = MS_GRAPH_OVERFLOW; return; }
    Cell<GM>* H = (Cell<GM>*)(slot + pools);
    const uint64_t hcap = (a.slot_bytes - pools) / sizeof(Cell<GM>);   // cells the slot holds
    uint32_t V = 0, E = 0, non_empty = 0;
    unsigned long long cells = 0;
    uint64_t aln_used = 0;   // graph instances: the pairs of the set's alignments so far
    uint32_t third = 0;      // strand instances: the sequences whose reverse complement won
    for (uint32_t k = 0; k < S.nseq; k++) {
        const uint64_t b = a.soff[S.seq_begin + k];
        const uint32_t L = (uint32_t)(a.soff[S.seq_begin + k + 1] - b);
        if (L == 0) continue;
        const uint8_t* s = a.codes + b;
        non_empty++;
        uint32_t na = 0;
        if (V) {
            if ((uint64_t)(V + 1) * (L + 1) > hcap) { if (t == 0) { a.status[set] = MS_H_OVERFLOW; a.vseen[set] = V; } return; }
            cells += (unsigned long long)V * L * (STRAND ? 2u : 1u);   // (strand instances: the algorithm's cells, both orientations)
            uint32_t bi, bj;
            if (GRAPH) mark_pairs<NT>(g, V);   // (dp_rows' barriers lie between this and the traceback)
            if constexpr (STRAND) {
                // Both orientations against the graph as it stands, the reverse complement first: when the forward one wins or ties, its
                // H is the one in the slot; when the reverse complement wins, a third pass computes its H again. One call site, so that
                // dp_rows is inlined once, as in the other instances. Every lane reads the scores from sh.best behind dp_rows' last
                // barrier (the next write to it lies behind the barriers of the next pass), so the choice is the same value in every lane.
                const uint8_t* rc = a.sa.codes_rc + b;
                int32_t score_r = 0, score_f = 0;
                bool rev = false;
#pragma unroll 1
                for (int pass = 0; pass < 3; pass++) {
                    if (pass == 2 && !rev) break;
                    dp_rows<NT, CPL, GM>(g, H, V, pass == 1 ? s : rc, L, a, sh, s_wtot, &bi, &bj);
                    if (pass == 0) score_r = sh.best;
                    if (pass == 1) { score_f = sh.best; rev = score_r > score_f; }   // (ties go forward)
                }
                third += rev;
                keep_strand<NT>(a, b, L, S.seq_begin + k, rev, score_f, score_r);
                s = a.sa.codes_used + b;
            } else dp_rows<NT, CPL, GM>(g, H, V, s, L, a, sh, s_wtot, &bi, &bj);
            if (t == 0 && bi) na = traceback<GM>(g, H, s, L, bi, bj, a);
            if (GRAPH && t == 0) sh.na = bi ? keep_score(g, V, na, sh.best, a.go.aln_score + S.seq_begin + k) : 0u;   // (sh.best: dp_rows' end-cell score)
        } else if constexpr (STRAND) {   // the first non-empty sequence goes in forward, without a DP: both scores 0
            keep_strand<NT>(a, b, L, S.seq_begin + k, false, 0, 0);
            s = a.sa.codes_used + b;
        }
        if (t == 0) {
            uint32_t v = V, e = E;
            const bool ok = add_alignment(g, v, e, na, s, L, path, colref);
            sh.V = v; sh.E = e; sh.fail = !ok;
        }
        __syncthreads();
        if (GRAPH && V) aln_used += keep_pairs<NT>(g, sh.na, a.go, set, S.seq_begin + k, aln_used);   // (V: the graph before the add)
        V = sh.V; E = sh.E;
        if (sh.fail) { if (t == 0) a.status[set] = MS_GRAPH_OVERFLOW; return; }
        if (MSA) for (uint32_t i = t; i < L; i += NT) a.base_col[b + i] = path[i];   // (node ids never change: a rerun set rewrites its part)
        if (WTS) weigh_path<NT>(g, path, (STRAND ? a.sa.wts_used : a.wts) + b, L);   // (order_rows reads e_w behind its barriers)
        order_rows<NT>(g, V, s_scan);
    }
    if (MSA) {
        // columns by rank into the DFS stack's pool (free after the last sort), then every base of the set from its node to its column
        uint32_t* colr = g.stack;
        const uint32_t ncols = msa_columns<NT>(g, V, colr, s_scan);
        const uint64_t b0 = a.soff[S.seq_begin];
        // (a graph instance keeps base_col as node ids: there the column travels with the node)
        if (GRAPH) keep_graph<NT>(g, V, E, colr, a.go, set, b0, b0 + S.seq_begin);
        else for (uint64_t i = t; i < S.sum_len; i += NT) a.base_col[b0 + i] = colr[g.node2rank[a.base_col[b0 + i]]];
        if (t < 64) {
            uint32_t len = 0, end_rank = 0;
            if (non_empty) {
                len = consensus_wave_end(g, V, a.cns + S.cns_off, &end_rank);
                if (a.cns_col) consensus_columns(g, end_rank, len, colr, (uint32_t*)g.aln_pos, a.cns_col + S.cns_off);
                if (GRAPH) consensus_columns(g, end_rank, len, g.rank2node, (uint32_t*)g.aln_pos, a.go.cns_node + S.cns_off);   // (the same walk, the rank's node in place of its column)
            }
            if (t == 0) {
                a.cns_len[set] = len; a.n_cols[set] = ncols; a.cells[set] = cells; a.status[set] = MS_OK;
                if (STRAND) a.sa.third[set] = third;
                if (GRAPH) { a.go.aln_need[set] = (uint32_t)min(aln_used, (uint64_t)0xffffffffu); if (aln_used > a.go.aln_room[set]) a.status[set] = MS_ALN_OVERFLOW; }
            }
        }
    } else if (t < 64) {
        const uint32_t len = non_empty ? consensus_wave(g, V, a.cns + S.cns_off) : 0u;
        if (t == 0) { a.cns_len[set] = len; a.cells[set] = cells; a.status[set] = MS_OK; }
    }
    __syncthreads();   // the slot is free for the next set
}

template <int NT, int CPL, int GM, bool MSA, bool WTS, bool GRAPH = false, bool STRAND = false>
__global__ __launch_bounds__(NT) void k_poa_general(MArgs a) {
    __shared__ Shared sh;
    __shared__ int s_wtot[(GM == GM_CONVEX ? 2 : 1) * (NT / 64)];   // per wave the total of its row scan (convex: of its two)
    __shared__ uint32_t s_scan[NT / 64];
    uint8_t* slot = a.ws + (size_t)blockIdx.x * a.slot_bytes;
    for (;;) {
        if (threadIdx.x == 0) sh.item = atomicAdd(a.counter, 1u);
        __syncthreads();
        const uint32_t q = sh.item;
        __syncthreads();
        if (q >= a.n_items) return;
        run_set<NT, CPL, GM, MSA, WTS, GRAPH, STRAND>(a, a.order[q], slot, sh, s_wtot, s_scan);
    }
}

// the instances: workgroup lanes x columns per lane; a set goes to the first whose NT x CPL columns hold its longest sequence + 1.
// Each comes in three variants: the consensus alone (a consensus-only call runs the code it ran before the MSA existed), with the node of
// every base kept (the MSA; coverage needs it too), with base weights applied on top of that (hx_poa_weighted with weights), and with the
// graph and the alignments written out on top of that (hx_poa_graph; without weights it runs on weights of 1, which add nothing to an edge).
// A fifth variant, over the weighted one, aligns every sequence in both orientations and adds the better one (hx_poa_strand).
struct Inst { int nt, cpl; const void* variant[5]; };
#define HX_INST(GM, NT, CPL) {NT, CPL, {(const void*)k_poa_general<NT, CPL, GM, false, false>, (const void*)k_poa_general<NT, CPL, GM, true, false>, (const void*)k_poa_general<NT, CPL, GM, true, true>, \
                                        (const void*)k_poa_general<NT, CPL, GM, true, true, true>, (const void*)k_poa_general<NT, CPL, GM, true, true, false, true>}}
constexpr int N_INST = 4;
// by gap model (GM_LINEAR, GM_AFFINE, GM_CONVEX). The affine instances keep two accumulators per column (diagonal and F): 16 columns per
// lane throughout, more lanes instead. The convex ones keep three (diagonal, F and O) and stop at 512 lanes, two waves per SIMD with up to
// 256 registers each: 1024 lanes would have 128 and spill the row (DESIGN.md "Convex gaps")
const Inst kInst[3][N_INST] = {
    {HX_INST(GM_LINEAR, 64, 16), HX_INST(GM_LINEAR, 256, 16), HX_INST(GM_LINEAR, 256, 32), HX_INST(GM_LINEAR, 1024, 32)},
    {HX_INST(GM_AFFINE, 64, 16), HX_INST(GM_AFFINE, 256, 16), HX_INST(GM_AFFINE, 512, 16), HX_INST(GM_AFFINE, 1024, 16)},
    {HX_INST(GM_CONVEX, 64, 16), HX_INST(GM_CONVEX, 128, 16), HX_INST(GM_CONVEX, 256, 16), HX_INST(GM_CONVEX, 512, 16)},
};
#undef HX_INST
constexpr uint32_t MAX_LEN[3] = {1024 * 32 - 1, 1024 * 16 - 1, 512 * 16 - 1};
constexpr uint64_t CELL_BYTES[3] = {4, 8, 12};   // of a cell of H by gap model: what the kernels take as sizeof(Cell<GM>)
static_assert(CELL_BYTES[GM_LINEAR] == sizeof(Cell<GM_LINEAR>) && CELL_BYTES[GM_AFFINE] == sizeof(Cell<GM_AFFINE>) && CELL_BYTES[GM_CONVEX] == sizeof(Cell<GM_CONVEX>), "CELL_BYTES against the cell types of poa_modes_dp.inl");
inline const void* fn(const Inst& inst, bool cols, bool weighted, bool graph, bool strand) { return inst.variant[strand ? 4 : graph ? 3 : weighted ? 2 : cols ? 1 : 0]; }

template <class T> struct Buf {   // device buffer of one call
    T* p = nullptr;
    hipError_t alloc(size_t n) { return hipMalloc((void**)&p, std::max<size_t>(n, 1) * sizeof(T)); }
    ~Buf() { if (p) (void)hipFree(p); }
};

// the work list of a grid-wide row kernel (k_msa_rows, k_cov_hist, k_cov_gather): one descriptor per row and one chunk (row, first element)
// per 64 elements of it, one wavefront each. A row without elements still gets its one chunk (the MSA row of an empty sequence).
template <class Row> struct RowList {
    std::vector<Row> rows; std::vector<uint2> chunks;
    Buf<Row> d_rows; Buf<uint2> d_chunks;
    void add(const Row& r, uint32_t n) {
        for (uint32_t f = 0; f == 0 || f < n; f += 64) chunks.push_back(make_uint2((uint32_t)rows.size(), f));
        rows.push_back(r);
    }
    bool too_many() const { return rows.size() >= 0xffffffffULL || chunks.size() >= 0xffffffffULL / 64; }
    uint32_t n_chunks() const { return (uint32_t)chunks.size(); }
    uint32_t blocks() const { return (uint32_t)((chunks.size() + 3) / 4); }   // of 256 lanes
    hipError_t upload(hipStream_t s) {
        hipError_t e = d_rows.alloc(rows.size());
        if (e == hipSuccess) e = d_chunks.alloc(chunks.size());
        if (e == hipSuccess) e = hipMemcpyAsync(d_rows.p, rows.data(), rows.size() * sizeof(Row), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(d_chunks.p, chunks.data(), chunks.size() * sizeof(uint2), hipMemcpyHostToDevice, s);
        return e;
    }
};

#define MCHK(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) { err = std::string(#expr) + ": " + hipGetErrorString(e_); return -1; } } while (0)

// one call of poa_modes_run: what its stages share. Every stage returns 0, or -1 with the reason in err.
struct Run {
    hipStream_t s; PoaModesWs& ws; const PoaModesArgs& a; PoaModesOut& o; std::string& err;
    const std::string who = a.who;
    const uint32_t ns = a.n_sets;
    const int gm = a.gap_model;                             // GM_LINEAR, GM_AFFINE or GM_CONVEX (the entry points set nothing else)
    const bool msa = a.msa != 0;
    const bool wtd = a.weighted != 0;                        // hx_poa_weighted: the node of every base is kept, as for the MSA
    const bool graph = a.graph != 0;                         // hx_poa_graph: the node of every base stays a node, the graph and the alignments are written out
    const bool strand = a.strand != 0;                       // hx_poa_strand: every sequence in both orientations; MSA text, coverage and profile as asked
    const bool cols = msa || wtd || graph || strand;
    const bool want_cov = (wtd || strand) && (a.want_coverage || a.want_profile);
    const Inst* const inst = kInst[gm];
    const uint64_t cell_bytes = CELL_BYTES[gm];
    const uint64_t nseq = a.set_off[ns], nb = a.seq_off[nseq];
    std::vector<MSet> sets = std::vector<MSet>(ns);
    std::vector<uint64_t> cns_off = std::vector<uint64_t>((size_t)ns + 1, 0);
    std::vector<uint8_t> codes;      // the bases as 0..3 (kept to the end of the call: they are uploaded asynchronously)
    std::vector<uint8_t> codes_rc, wts_rc;   // strand calls: every sequence reverse-complemented at its own offset, its weights reversed with it
    std::vector<uint64_t> vest;      // per set: the estimate of its graph's final size that its H is sized from
    std::vector<uint32_t> todo;      // the sets of the next round
    std::vector<uint32_t> len;       // per set: the length of its consensus (after consensus())
    int n_cu = 0;
    uint64_t budget = 0;
    Buf<MSet> d_sets; Buf<uint8_t> d_codes; Buf<uint64_t> d_soff; Buf<uint32_t> d_order, d_counter, d_status, d_vseen, d_cns_len; Buf<unsigned long long> d_cells; Buf<char> d_cns;
    Buf<uint32_t> d_base_col, d_n_cols, d_cns_col;   // MSA and weighted calls only
    Buf<uint8_t> d_wts;                              // weighted calls with weights only: a byte per base (graph and strand calls: always, 1 without weights)
    // strand calls only: what StrandArgs points to
    Buf<uint8_t> d_codes_rc, d_wts_rc, d_codes_used, d_wts_used, d_reversed; Buf<int32_t> d_score_fwd, d_score_rev; Buf<uint32_t> d_third;
    // graph calls only: what GraphOutArgs points to. The alignment pool is one allocation per round (a rerun set's share lies in a later
    // round's pool; pool_of / aln_at tell where a set's pairs are after the last round it ran in)
    struct Pool { Buf<int32_t> node, pos; };
    std::vector<std::unique_ptr<Pool>> pools;
    std::vector<uint32_t> pool_of, aln_room, aln_rerun;   // per set: the round of its share, the share in pairs, 1 once it was rerun for want of room
    std::vector<uint64_t> aln_at;
    Buf<uint64_t> d_aln_at; Buf<uint32_t> d_aln_room, d_aln_need, d_aln_cnt, d_n_nodes, d_n_edges, d_node_rank, d_node_col, d_edge_from, d_edge_to, d_cns_node;
    Buf<int32_t> d_aln_score, d_edge_w; Buf<uint8_t> d_node_code;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~Run() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }

    const void* fn_of(int k) const { return fn(inst[k], cols, d_wts.p != nullptr, graph, strand); }
    const uint8_t* codes_as_added() const { return strand ? d_codes_used.p : d_codes.p; }   // what the row, coverage and profile kernels read
    uint64_t pools_of(uint32_t i) const { const MSet& S = sets[i]; return carve_pools(nullptr, S.sum_len, S.nseq, S.lmax, nullptr, nullptr, nullptr); }

    // runs f (0 = ok) between two events, waits for it, and adds the milliseconds it took on the device to *ms
    template <class F> int timed(float* ms, F f) {
        MCHK(hipEventRecord(e0, s));
        if (f()) return -1;
        MCHK(hipEventRecord(e1, s));
        MCHK(hipEventSynchronize(e1));
        float t = 0;
        MCHK(hipEventElapsedTime(&t, e0, e1));
        *ms += t;
        return 0;
    }

    // ---- the sets checked and described, the call's inputs on the device, the memory budget
    int prepare() {
        const uint32_t max_len = MAX_LEN[gm];
        o = PoaModesOut();
        for (uint32_t i = 0; i < ns; i++) {
            MSet& S = sets[i];
            S.seq_begin = a.set_off[i]; S.nseq = (uint32_t)(a.set_off[i + 1] - a.set_off[i]); S.sum_len = 0; S.lmax = 0;
            for (uint64_t k = a.set_off[i]; k < a.set_off[i + 1]; k++) {
                const uint64_t L = a.seq_off[k + 1] - a.seq_off[k];
                if (L > max_len) { err = who + ": set " + std::to_string(i) + " holds a sequence of " + std::to_string(L) + " bases, longer than " + std::to_string(max_len) + (gm == GM_CONVEX ? " (the longest the general POA path takes with convex gaps)" : gm == GM_AFFINE ? " (the longest the general POA path takes with affine gaps)" : " (the longest the general POA path takes)"); return -1; }
                S.sum_len += L; S.lmax = std::max(S.lmax, (uint32_t)L);
                o.seq_bases += L; o.n_aligned += L != 0;
            }
            if (S.sum_len > MAX_SET_BASES) { err = who + ": set " + std::to_string(i) + " holds " + std::to_string(S.sum_len) + " bases in all, more than the " + std::to_string(MAX_SET_BASES) + " nodes a graph can have"; return -1; }
            S.cns_off = cns_off[i]; cns_off[i + 1] = cns_off[i] + S.sum_len;   // (a consensus has at most one base per node)
        }
        codes.resize(std::max<uint64_t>(1, nb));
        for (uint64_t k = 0; k < nb; k++) { const char c = a.bases[k]; codes[k] = c == 'C' || c == 'c' ? 1 : c == 'G' || c == 'g' ? 2 : c == 'T' || c == 't' ? 3 : 0; }
        int dev = 0;
        MCHK(hipGetDevice(&dev));
        MCHK(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev));
        MCHK(d_sets.alloc(ns)); MCHK(d_codes.alloc(codes.size())); MCHK(d_soff.alloc(nseq + 1)); MCHK(d_order.alloc(ns)); MCHK(d_counter.alloc(N_INST));
        MCHK(d_status.alloc(ns)); MCHK(d_vseen.alloc(ns)); MCHK(d_cns_len.alloc(ns)); MCHK(d_cells.alloc(ns)); MCHK(d_cns.alloc(cns_off[ns]));
        MCHK(hipMemcpyAsync(d_sets.p, sets.data(), ns * sizeof(MSet), hipMemcpyHostToDevice, s));
        MCHK(hipMemcpyAsync(d_codes.p, codes.data(), codes.size(), hipMemcpyHostToDevice, s));
        MCHK(hipMemcpyAsync(d_soff.p, a.seq_off, (nseq + 1) * 8, hipMemcpyHostToDevice, s));
        MCHK(hipMemsetAsync(d_cns_len.p, 0, std::max<size_t>(1, ns) * 4, s));
        MCHK(hipMemsetAsync(d_cells.p, 0, std::max<size_t>(1, ns) * 8, s));
        if (cols) {
            MCHK(d_base_col.alloc(nb)); MCHK(d_n_cols.alloc(ns));
            MCHK(hipMemsetAsync(d_n_cols.p, 0, std::max<size_t>(1, ns) * 4, s));
            if ((msa && a.include_consensus) || want_cov) MCHK(d_cns_col.alloc(cns_off[ns]));
        }
        if ((wtd || graph || strand) && a.weights) {
            MCHK(d_wts.alloc(nb));
            MCHK(hipMemcpyAsync(d_wts.p, a.weights, nb, hipMemcpyHostToDevice, s));
        }
        if ((graph || strand) && !a.weights) { MCHK(d_wts.alloc(nb)); MCHK(hipMemsetAsync(d_wts.p, 1, std::max<uint64_t>(1, nb), s)); }
        if (strand) {
            codes_rc.resize(codes.size());
            if (a.weights) wts_rc.resize(codes.size());
            for (uint64_t k = 0; k < nseq; k++) {
                const uint64_t b = a.seq_off[k], L = a.seq_off[k + 1] - b;
                for (uint64_t i = 0; i < L; i++) { codes_rc[b + i] = (uint8_t)(3 - codes[b + L - 1 - i]); if (a.weights) wts_rc[b + i] = a.weights[b + L - 1 - i]; }
            }
            MCHK(d_codes_rc.alloc(nb)); MCHK(d_codes_used.alloc(nb)); MCHK(d_wts_used.alloc(nb));
            MCHK(d_reversed.alloc(nseq)); MCHK(d_score_fwd.alloc(nseq)); MCHK(d_score_rev.alloc(nseq)); MCHK(d_third.alloc(ns));
            MCHK(hipMemcpyAsync(d_codes_rc.p, codes_rc.data(), nb, hipMemcpyHostToDevice, s));
            if (a.weights) { MCHK(d_wts_rc.alloc(nb)); MCHK(hipMemcpyAsync(d_wts_rc.p, wts_rc.data(), nb, hipMemcpyHostToDevice, s)); }   // (without weights: d_wts, all 1, is its own reverse)
            // (an empty sequence and a set's first non-empty one keep flag 0 and scores 0; a set without a base writes no count)
            MCHK(hipMemsetAsync(d_reversed.p, 0, std::max<uint64_t>(1, nseq), s)); MCHK(hipMemsetAsync(d_score_fwd.p, 0, std::max<uint64_t>(1, nseq) * 4, s));
            MCHK(hipMemsetAsync(d_score_rev.p, 0, std::max<uint64_t>(1, nseq) * 4, s)); MCHK(hipMemsetAsync(d_third.p, 0, std::max<size_t>(1, ns) * 4, s));
        }
        if (graph) {
            const uint64_t ne = nb + nseq;   // (a set's edges start at its first base's offset plus its first sequence's index)
            MCHK(d_aln_at.alloc(ns)); MCHK(d_aln_room.alloc(ns)); MCHK(d_aln_need.alloc(ns)); MCHK(d_aln_cnt.alloc(nseq)); MCHK(d_aln_score.alloc(nseq));
            MCHK(d_n_nodes.alloc(ns)); MCHK(d_n_edges.alloc(ns)); MCHK(d_node_code.alloc(nb)); MCHK(d_node_rank.alloc(nb)); MCHK(d_node_col.alloc(nb));
            MCHK(d_edge_from.alloc(ne)); MCHK(d_edge_to.alloc(ne)); MCHK(d_edge_w.alloc(ne)); MCHK(d_cns_node.alloc(cns_off[ns]));
            // (a sequence that meets no DP writes neither: its alignment is empty, its score 0; a set without a base writes no counts)
            MCHK(hipMemsetAsync(d_aln_cnt.p, 0, std::max<uint64_t>(1, nseq) * 4, s)); MCHK(hipMemsetAsync(d_aln_score.p, 0, std::max<uint64_t>(1, nseq) * 4, s));
            MCHK(hipMemsetAsync(d_n_nodes.p, 0, std::max<size_t>(1, ns) * 4, s)); MCHK(hipMemsetAsync(d_n_edges.p, 0, std::max<size_t>(1, ns) * 4, s));
            // The share of the alignment pool a set gets in its first round. The alignment of a sequence of L bases holds one pair per base
            // and one per graph node the walk passes without a base; under kNW the walk spans the graph from a source to a sink, which for
            // copies of one template is about the longest sequence. So: max(L, longest) pairs, an eighth more for the nodes passed without
            // a base (the copy's deletions against that path: 3 % in the error models of the tests and the bench tool, a quarter of that
            // room), and 16 for short sequences, per sequence after the first non-empty one (DESIGN.md "Graph and alignment output" has
            // the reasoning and the measured reruns)
            pool_of.assign(ns, 0); aln_room.assign(ns, 0); aln_rerun.assign(ns, 0); aln_at.assign(ns, 0);
            for (uint32_t i = 0; i < ns; i++) {
                uint64_t est = 0;
                bool seen = false;
                for (uint64_t k = a.set_off[i]; k < a.set_off[i + 1]; k++) {
                    const uint64_t L = a.seq_off[k + 1] - a.seq_off[k];
                    if (L == 0) continue;
                    if (seen) { const uint64_t span = std::max<uint64_t>(L, sets[i].lmax); est += span + span / 8 + 16; }
                    seen = true;
                }
                aln_room[i] = (uint32_t)std::min<uint64_t>(est, 0xfffffffeu);
                if (a.aln_cap) aln_room[i] = std::min(aln_room[i], a.aln_cap);   // (test switch: forces the overflow and the rerun with the exact room)
            }
        }
        // H is sized from an estimate of the graph's final size (noisy copies add about a tenth of their length each); a set that outgrows its
        // slot comes back and is rerun with twice the room (or the room for what it had when it stopped, doubled), the worst case at most
        vest.resize(ns);
        for (uint32_t i = 0; i < ns; i++) { vest[i] = std::min<uint64_t>(sets[i].sum_len, sets[i].lmax + sets[i].sum_len / 8 + 64); if (sets[i].sum_len) todo.push_back(i); }
        size_t fr = 0, tot = 0;
        MCHK(hipMemGetInfo(&fr, &tot));
        budget = a.workspace_gb > 0 ? (uint64_t)(a.workspace_gb * 1e9) : (uint64_t)((double)(fr + ws.cap) * 0.4);
        MCHK(hipEventCreate(&e0)); MCHK(hipEventCreate(&e1));
        return 0;
    }

    // ---- one round over todo: plan, launch, collect; the sets that outgrew their slot are todo again
    int round(const bool first) {
        auto need = [&](uint32_t i) { return pools_of(i) + al256((vest[i] + 1) * (uint64_t)(sets[i].lmax + 1) * cell_bytes); };
        auto inst_of = [&](uint32_t i) { int k = 0; while ((uint64_t)inst[k].nt * inst[k].cpl < (uint64_t)sets[i].lmax + 1) k++; return k; };
        // the plan: per instance, its sets costliest first, one slot size (the largest need), as many slots as are resident and fit the budget
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
                pmax = std::max(pmax, pools_of(i));
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
        GraphOutArgs go{};
        if (graph) {   // this round's pool: the shares of its sets side by side
            pools.emplace_back(new Pool);
            uint64_t at = 0;
            for (uint32_t i : todo) { pool_of[i] = (uint32_t)pools.size() - 1; aln_at[i] = at; at += aln_room[i]; }
            Pool& P = *pools.back();
            {
                hipError_t e = P.node.alloc(at);
                if (e == hipSuccess) e = P.pos.alloc(at);
                if (e != hipSuccess) { err = who + ": the alignment pool of " + std::to_string(at) + " pairs could not be allocated on the device: " + hipGetErrorString(e); return -1; }
            }
            MCHK(hipMemcpyAsync(d_aln_at.p, aln_at.data(), ns * 8, hipMemcpyHostToDevice, s));
            MCHK(hipMemcpyAsync(d_aln_room.p, aln_room.data(), ns * 4, hipMemcpyHostToDevice, s));
            go = GraphOutArgs{P.node.p, P.pos.p, d_aln_at.p, d_aln_room.p, d_aln_need.p, d_aln_cnt.p, d_aln_score.p, d_node_code.p, d_node_rank.p, d_node_col.p, d_n_nodes.p,
                              d_edge_from.p, d_edge_to.p, d_edge_w.p, d_n_edges.p, d_cns_node.p};
        }
        MCHK(hipMemcpyAsync(d_order.p, order.data(), order.size() * 4, hipMemcpyHostToDevice, s));
        MCHK(hipMemsetAsync(d_counter.p, 0, N_INST * 4, s));
        MCHK(hipMemsetAsync(d_status.p, 0xff, std::max<size_t>(1, ns) * 4, s));
        float ms = 0;
        if (timed(&ms, [&] {
                for (int k = 0; k < N_INST; k++) {
                    if (by[k].empty()) continue;
                    MArgs q{d_sets.p, d_order.p + base[k], (uint32_t)by[k].size(), d_counter.p + k, d_codes.p, d_soff.p, (uint8_t*)ws.p, slot[k],
                            a.match, a.mismatch, a.gap, a.type, d_cns.p, d_cns_len.p, d_status.p, d_vseen.p, d_cells.p, a.gap_extend,
                            d_base_col.p, d_n_cols.p, d_cns_col.p, d_wts.p, a.gap_open2, a.gap_extend2, go,
                            StrandArgs{d_codes_rc.p, d_wts_rc.p ? d_wts_rc.p : d_wts.p, d_codes_used.p, d_wts_used.p, d_reversed.p, d_score_fwd.p, d_score_rev.p, d_third.p}};
                    void* kargs[] = {&q};
                    MCHK(hipLaunchKernel(fn_of(k), dim3(nslots[k]), dim3((uint32_t)inst[k].nt), kargs, 0, s));
                    o.launches++;
                    if (a.debug) fprintf(stderr, "[hx] POA modes%s: %zu sets on %u workgroups of %d lanes x %d columns, slots of %.1f MB\n", gm == GM_CONVEX ? " (convex)" : gm == GM_AFFINE ? " (affine)" : "", by[k].size(), nslots[k], inst[k].nt, inst[k].cpl, slot[k] / 1e6);
                }
                return 0;
            })) return -1;
        o.kernel_ms += ms;
        std::vector<uint32_t> status(ns), vseen(ns);
        MCHK(hipMemcpy(status.data(), d_status.p, ns * 4, hipMemcpyDeviceToHost));
        MCHK(hipMemcpy(vseen.data(), d_vseen.p, ns * 4, hipMemcpyDeviceToHost));
        std::vector<uint32_t> next, pairs;   // (pairs: what the alignments of a set hold in all)
        if (graph) { pairs.resize(ns); MCHK(hipMemcpy(pairs.data(), d_aln_need.p, ns * 4, hipMemcpyDeviceToHost)); }
        for (uint32_t i : todo) {
            if (status[i] == MS_OK) continue;
            if (graph && status[i] == MS_ALN_OVERFLOW) {   // done, but for its alignments: once more, with exactly the room they need
                if (aln_rerun[i] || pairs[i] == 0xffffffffu) { err = who + ": set " + std::to_string(i) + " failed on the device (its alignments hold " + std::to_string(pairs[i]) + " pairs, its share of the pool " + std::to_string(aln_room[i]) + ")"; return -1; }
                aln_rerun[i] = 1; aln_room[i] = pairs[i];
                next.push_back(i);
                o.aln_retried++;
                continue;
            }
            const bool capped = first && a.slot_kb_cap;   // (a capped slot can be short of even the worst case)
            if (status[i] != MS_H_OVERFLOW || (vest[i] >= sets[i].sum_len && !capped)) { err = who + ": set " + std::to_string(i) + " failed on the device (status " + std::to_string((int)status[i]) + ")"; return -1; }
            vest[i] = std::min<uint64_t>(sets[i].sum_len, std::max<uint64_t>(2 * vest[i], 2 * (uint64_t)vseen[i] + 64));
            next.push_back(i);
            o.retried++;
        }
        todo.swap(next);
        return 0;
    }

    // ---- the consensus strings and the cell counts, after the last round
    int consensus() {
        len.resize(ns);
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
        if (strand) {   // (a set that was rerun rewrote its own part)
            std::vector<uint32_t> third(ns);
            o.reversed.assign(nseq, 0); o.score_fwd.assign(nseq, 0); o.score_rev.assign(nseq, 0);
            MCHK(hipMemcpy(third.data(), d_third.p, ns * 4, hipMemcpyDeviceToHost));
            if (nseq) { MCHK(hipMemcpy(o.reversed.data(), d_reversed.p, nseq, hipMemcpyDeviceToHost)); MCHK(hipMemcpy(o.score_fwd.data(), d_score_fwd.p, nseq * 4, hipMemcpyDeviceToHost)); MCHK(hipMemcpy(o.score_rev.data(), d_score_rev.p, nseq * 4, hipMemcpyDeviceToHost)); }
            for (uint32_t i = 0; i < ns; i++) o.third_passes += third[i];
        }
        return 0;
    }

    // ---- coverage and profile: now that the columns of every set are known, one counter per column (four with the profile: one per
    // letter) for the whole call, filled from the bases of the sequences of >= 2 bases (k_cov_hist), then read at the columns of the
    // consensus bases (k_cov_gather). Built here, after the last round: a set that was rerun is counted once.
    int coverage() {
        const uint32_t stride = a.want_profile ? 4u : 1u;
        std::vector<uint32_t> ncols(ns);
        MCHK(hipMemcpy(ncols.data(), d_n_cols.p, ns * 4, hipMemcpyDeviceToHost));
        RowList<CRow> seqs, cnss;
        uint64_t hoff = 0, hist_bases = 0;
        for (uint32_t i = 0; i < ns; i++) {
            for (uint64_t k = a.set_off[i]; k < a.set_off[i + 1]; k++) {
                const uint32_t L = (uint32_t)(a.seq_off[k + 1] - a.seq_off[k]);
                if (L < 2) continue;   // (spoa counts the sequence labels of a node's edges: a sequence of one base has none)
                seqs.add(CRow{a.seq_off[k], 0, hoff, L, ncols[i]}, L);
                hist_bases += L;
            }
            if (len[i]) cnss.add(CRow{cns_off[i], o.cns_off[i], hoff, len[i], ncols[i]}, len[i]);
            hoff += ncols[i];
        }
        if (seqs.too_many() || cnss.too_many()) { err = who + ": too many sequences"; return -1; }
        const uint64_t nc = o.cns.size();
        o.cov.assign(nc, 0);
        if (a.want_profile) o.prof.assign(4 * nc, 0);
        if (!nc) return 0;
        Buf<uint32_t> d_hist, d_cov, d_prof;
        MCHK(seqs.upload(s)); MCHK(cnss.upload(s));
        MCHK(d_hist.alloc(hoff * stride)); MCHK(d_cov.alloc(nc));
        if (a.want_profile) MCHK(d_prof.alloc(4 * nc));
        float cov_ms = 0;
        if (timed(&cov_ms, [&] {
                MCHK(hipMemsetAsync(d_hist.p, 0, std::max<uint64_t>(1, hoff * stride) * 4, s));
                if (seqs.n_chunks()) {
                    k_cov_hist<<<seqs.blocks(), 256, 0, s>>>(seqs.d_rows.p, seqs.d_chunks.p, seqs.n_chunks(), d_base_col.p, codes_as_added(), stride, d_hist.p);
                    MCHK(hipGetLastError());
                    o.launches++;
                }
                k_cov_gather<<<cnss.blocks(), 256, 0, s>>>(cnss.d_rows.p, cnss.d_chunks.p, cnss.n_chunks(), d_cns_col.p, d_hist.p, stride, d_cov.p, d_prof.p);
                MCHK(hipGetLastError());
                return 0;
            })) return -1;
        o.cov_ms = cov_ms; o.kernel_ms += cov_ms; o.launches++;
        // what the two kernels and the clearing of the counters must move: a column (and a letter) read per counted base, the
        // counters written twice and read once where a consensus base stands, a column read and the counts written per consensus base
        o.cov_moved_bytes = hist_bases * (4 + (stride == 4 ? 1 : 0)) + 2 * hoff * stride * 4 + nc * (4 + 4 * stride + 4 + (a.want_profile ? 16 : 0));
        MCHK(hipMemcpy(o.cov.data(), d_cov.p, nc * 4, hipMemcpyDeviceToHost));
        if (a.want_profile) MCHK(hipMemcpy(o.prof.data(), d_prof.p, 4 * nc * 4, hipMemcpyDeviceToHost));
        return 0;
    }

    // ---- the graph and the alignments: now that the host knows the nodes, edges and pairs of every set, one grid-wide kernel moves them
    // from the worst-case places run_set wrote them to into dense arrays, set after set (codes become letters, an alignment's pairs are
    // turned into forward order), and only those are downloaded. Built here, after the last round: a set that was rerun is taken from
    // the round it finished in, once.
    int graph_out() {
        std::vector<uint32_t> nv(ns), ne(ns), cnt(nseq);
        o.aln_score.assign(nseq, 0);
        MCHK(hipMemcpy(nv.data(), d_n_nodes.p, ns * 4, hipMemcpyDeviceToHost));
        MCHK(hipMemcpy(ne.data(), d_n_edges.p, ns * 4, hipMemcpyDeviceToHost));
        MCHK(hipMemcpy(cnt.data(), d_aln_cnt.p, nseq * 4, hipMemcpyDeviceToHost));
        MCHK(hipMemcpy(o.aln_score.data(), d_aln_score.p, nseq * 4, hipMemcpyDeviceToHost));
        o.node_off.assign((size_t)ns + 1, 0); o.edge_off.assign((size_t)ns + 1, 0); o.aln_off.assign((size_t)nseq + 1, 0);
        RowList<GRow> rows;
        for (uint32_t i = 0; i < ns; i++) {
            const uint64_t b0 = a.seq_off[a.set_off[i]];
            o.node_off[i + 1] = o.node_off[i] + nv[i]; o.edge_off[i + 1] = o.edge_off[i] + ne[i];
            if (nv[i]) rows.add(GRow{nullptr, nullptr, b0, o.node_off[i], nv[i], GR_NODES}, nv[i]);
            if (ne[i]) rows.add(GRow{nullptr, nullptr, b0 + a.set_off[i], o.edge_off[i], ne[i], GR_EDGES}, ne[i]);
            if (len[i]) rows.add(GRow{nullptr, nullptr, cns_off[i], o.cns_off[i], len[i], GR_CNS}, len[i]);
            uint64_t at = sets[i].sum_len ? aln_at[i] : 0;
            for (uint64_t k = a.set_off[i]; k < a.set_off[i + 1]; k++) {
                o.aln_off[k + 1] = o.aln_off[k] + cnt[k];
                if (cnt[k]) { const Pool& P = *pools[pool_of[i]]; rows.add(GRow{P.node.p, P.pos.p, at, o.aln_off[k], cnt[k], GR_ALN}, cnt[k]); }
                at += cnt[k];
            }
            if (sets[i].sum_len && at - aln_at[i] > aln_room[i]) { err = who + ": internal error (the alignments of set " + std::to_string(i) + " outgrew their share of the pool)"; return -1; }
        }
        if (rows.too_many()) { err = who + ": too many sequences"; return -1; }
        const uint64_t NV = o.node_off[ns], NE = o.edge_off[ns], NC = o.cns.size(), NP = o.aln_off[nseq];
        o.node_base.resize(NV); o.node_rank.resize(NV); o.node_col.resize(NV);
        o.edge_from.resize(NE); o.edge_to.resize(NE); o.edge_w.resize(NE);
        o.cns_node.resize(NC); o.aln_node.resize(NP); o.aln_pos.resize(NP);
        o.base_node.resize(nb);
        if (nb) MCHK(hipMemcpy(o.base_node.data(), d_base_col.p, nb * 4, hipMemcpyDeviceToHost));   // (dense as it is: the layout of the call's bases)
        if (rows.n_chunks() == 0) return 0;
        Buf<char> o_base; Buf<uint32_t> o_rank, o_col, o_from, o_to, o_cns; Buf<int32_t> o_w, o_an, o_ap;
        MCHK(o_base.alloc(NV)); MCHK(o_rank.alloc(NV)); MCHK(o_col.alloc(NV)); MCHK(o_from.alloc(NE)); MCHK(o_to.alloc(NE)); MCHK(o_w.alloc(NE));
        MCHK(o_cns.alloc(NC)); MCHK(o_an.alloc(NP)); MCHK(o_ap.alloc(NP));
        MCHK(rows.upload(s));
        const GatherArgs ga{d_node_code.p, d_node_rank.p, d_node_col.p, d_edge_from.p, d_edge_to.p, d_edge_w.p, d_cns_node.p,
                            o_base.p, o_rank.p, o_col.p, o_from.p, o_to.p, o_w.p, o_cns.p, o_an.p, o_ap.p};
        float ms = 0;
        if (timed(&ms, [&] {
                k_graph_gather<<<rows.blocks(), 256, 0, s>>>(rows.d_rows.p, rows.d_chunks.p, rows.n_chunks(), ga);
                MCHK(hipGetLastError());
                return 0;
            })) return -1;
        o.gather_ms = ms; o.kernel_ms += ms; o.launches++;
        o.gather_moved_bytes = 2 * (9 * NV + 12 * NE + 4 * NC + 8 * NP);   // every element read once and written once
        if (NV) { MCHK(hipMemcpy(&o.node_base[0], o_base.p, NV, hipMemcpyDeviceToHost)); MCHK(hipMemcpy(o.node_rank.data(), o_rank.p, NV * 4, hipMemcpyDeviceToHost)); MCHK(hipMemcpy(o.node_col.data(), o_col.p, NV * 4, hipMemcpyDeviceToHost)); }
        if (NE) { MCHK(hipMemcpy(o.edge_from.data(), o_from.p, NE * 4, hipMemcpyDeviceToHost)); MCHK(hipMemcpy(o.edge_to.data(), o_to.p, NE * 4, hipMemcpyDeviceToHost)); MCHK(hipMemcpy(o.edge_w.data(), o_w.p, NE * 4, hipMemcpyDeviceToHost)); }
        if (NC) MCHK(hipMemcpy(o.cns_node.data(), o_cns.p, NC * 4, hipMemcpyDeviceToHost));
        if (NP) { MCHK(hipMemcpy(o.aln_node.data(), o_an.p, NP * 4, hipMemcpyDeviceToHost)); MCHK(hipMemcpy(o.aln_pos.data(), o_ap.p, NP * 4, hipMemcpyDeviceToHost)); }
        return 0;
    }

    // ---- the MSA text: now that the columns of every set are known, the rows' places (set i = rows x n_cols bytes, row-major) and the
    // work list of k_msa_rows
    int msa_text() {
        o.msa_cols.assign(ns, 0);
        MCHK(hipMemcpy(o.msa_cols.data(), d_n_cols.p, ns * 4, hipMemcpyDeviceToHost));
        o.msa_rows.assign(ns, 0);
        o.msa_off.assign((size_t)ns + 1, 0);
        RowList<MRow> rows;
        for (uint32_t i = 0; i < ns; i++) {
            const uint32_t nc = o.msa_cols[i];
            uint64_t dst = o.msa_off[i];
            if (nc) {   // (no column: no non-empty sequence, nothing to write)
                for (uint64_t k = a.set_off[i]; k < a.set_off[i + 1]; k++, dst += nc) { const uint32_t L = (uint32_t)(a.seq_off[k + 1] - a.seq_off[k]); rows.add(MRow{a.seq_off[k], dst, L, nc, 0, 0}, L); }
                if (a.include_consensus) rows.add(MRow{cns_off[i], dst, len[i], nc, 1, 0}, len[i]);
            }
            o.msa_rows[i] = sets[i].nseq + (a.include_consensus ? 1u : 0u);
            o.msa_off[i + 1] = o.msa_off[i] + (uint64_t)o.msa_rows[i] * nc;
        }
        if (rows.too_many()) { err = who + ": too many rows"; return -1; }
        const uint64_t out_bytes = o.msa_off[ns];
        o.msa.resize(out_bytes);
        if (out_bytes == 0) return 0;
        Buf<char> d_out;
        {
            const hipError_t e = d_out.alloc(out_bytes);
            if (e != hipSuccess) { err = who + ": the " + std::to_string(out_bytes) + " bytes of the alignment text could not be allocated on the device: " + hipGetErrorString(e); return -1; }
        }
        MCHK(rows.upload(s));
        float rows_ms = 0;
        if (timed(&rows_ms, [&] {
                k_msa_rows<<<rows.blocks(), 256, 0, s>>>(rows.d_rows.p, rows.d_chunks.p, rows.n_chunks(), d_base_col.p, codes_as_added(), d_cns_col.p, d_cns.p, d_out.p);
                MCHK(hipGetLastError());
                return 0;
            })) return -1;
        o.msa_rows_ms = rows_ms; o.kernel_ms += rows_ms; o.launches++;
        o.msa_moved_bytes = out_bytes + 4 * (nb + (a.include_consensus ? o.cns.size() : 0));
        MCHK(hipMemcpy(&o.msa[0], d_out.p, out_bytes, hipMemcpyDeviceToHost));
        return 0;
    }
};

}  // namespace

int poa_modes_run(hipStream_t s, PoaModesWs& ws, const PoaModesArgs& a, PoaModesOut& o, std::string& err) {
    Run r{s, ws, a, o, err};
    if (r.prepare()) return -1;
    for (bool first = true; !r.todo.empty(); first = false)
        if (r.round(first)) return -1;
    if (r.consensus()) return -1;
    if (r.want_cov && r.coverage()) return -1;
    if (r.graph) return r.graph_out();
    return r.msa ? r.msa_text() : 0;
}

}  // namespace hxk
