// poa_modes.hip — the general POA path: spoa's linear-gap engine in its three alignment modes (kSW local, kNW global, kOV overlap) for
// caller-given sequence sets (hx_poa_sequences_mode; DESIGN.md "General POA path" has the semantics and the mapping), and the affine-gap
// engine in the same modes (hx_poa_sequences_affine: same mapping, a cell is the pair (H, F), its own row of the instance table), and the
// two-piece affine ("convex") gap model (hx_poa_sequences_convex: a cell is (H, F, O), 12 bytes, a third row of the table). All of it is
// one kernel template, k_poa_general<NT, CPL, GM, MSA, WTS, GRAPH, STRAND, BAND, LABELS>, GM the gap model (and k_poa_phase, the same loop
// over run_set with its PHASE flag set).
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
// Adaptive banded alignment (hx_poa_banded; DESIGN.md "Banded alignment") is a flag of its own, BAND, over the three variants that keep no
// per-alignment pair pool: one shape per gap model, one wavefront of 64 lanes x 16 columns, whose row loop and traceback (dp_rows_band,
// traceback_band) read and write H through per-row windows of 2 w + 1 columns. An alignment without a reachable end cell stops its set
// with MS_BAND_MISS; the host runs the set again in twice the band, at last in the full-matrix instances above.
//
// Per-label consensus (hx_poa_labelled; DESIGN.md "Per-label consensus") is one more flag, LABELS, over the weighted variant of every
// shape: the graph is built as ever, and behind the last sort the workgroup runs once per label over the view of that label - the edges
// its own sequences walk, weighed by them alone (label_views: a per-edge weight array, the rank-ordered rows without the absent edges, the
// heaviest bundle with a branch completion that stays inside the view) - and writes one consensus and its columns per label.
//
// Two-haplotype consensus (hx_poa_phased; DESIGN.md "Two-haplotype consensus") is one more flag of run_set, PHASE, over LABELS (kernel k_poa_phase): between msa_columns and
// label_views the workgroup derives the label of every sequence of its set itself (phase_reads: the heterozygous columns, a seed site,
// at most eight voting rounds, a verdict) and label_views reads those labels as it reads a caller's, with two labels.
//
// Layout: the DP and traceback of the three gap models are poa_modes_dp.inl, their banded siblings poa_modes_band.inl, the columns, row text, coverage and the graph output's helpers
// and gather and the per-label views poa_modes_out.inl, the pools of a set poa_modes_pools.inl; this file keeps the work of one set (run_set), the kernel, the
// kernel table and the device half of the host driver (poa_modes_run, in named stages: buffers, uploads, launches, downloads). Every
// integer decision of those stages - limits, instance, slot sizes, shares of the alignment pool, the retry rule, the work lists and
// offsets of the outputs - is poa_modes_plan.h / .hip, which makes no HIP call and is tested without a GPU.
#include <algorithm>
#include <memory>

#include "kernels.h"
#include "poa_modes_plan.h"

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "kernels/poa_modes.hip is written for gfx950 (CDNA4)"
#endif

namespace hxk {

namespace {

#include "poa_graph.inl"    // the graph of a set, spoa's topological order, heaviest bundle

#include "poa_modes_pools.inl"   // al256, carve_pools: the graph pools of a set at the start of its slot

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

// What the phase instances (hx_poa_phased) read and write beside the rest: the haplotype of every sequence of the call (the array the
// label code then reads as labels), per set its haplotypes, rounds and sites, and the sites themselves from the set's first base's
// global offset on (site_inf: a1 | a2 << 4 | (phase + 1) << 8); the two thresholds of the site rule.
struct PhaseArgs { uint8_t* hap; uint32_t *n_haps, *rounds, *n_sites, *site_col, *site_inf; uint32_t min_count, min_pct; };

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
    const uint32_t* band_w;   // band instances only: per set the half-width of its current attempt
    // label instances only: the label of every sequence of the call (0 .. n_labels - 1, or 255: none). A set has n_labels consensus
    // places of sum_len bases each from its cns_off on, and cns_len holds n_labels lengths per set
    const uint8_t* labels; uint32_t n_labels;
    PhaseArgs ph;         // phase instances only (labels is ph.hap, n_labels 2)
};

// one row of the MSA text: its columns (rising) start at cols[src], its letters at codes[src] (a sequence) or cns[src] (the consensus row)
struct MRow { uint64_t src, dst; uint32_t len, ncols, is_cns, pad; };

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

struct Shared { uint32_t item, V, E, fail; int best; uint32_t na /* graph instances: the pairs the traceback left; label instances: the smallest node id of a view */; unsigned long long key; };

#include "poa_modes_dp.inl"     // DP and traceback, linear, affine and convex gaps
#include "poa_modes_band.inl"   // the banded row loop and traceback: one wavefront per window
#include "poa_modes_out.inl"    // MSA columns and row text, base weights, coverage, graph and alignment output

template <int NT, int CPL, int GM, bool MSA, bool WTS, bool GRAPH, bool STRAND, bool BAND, bool LABELS, bool PHASE>
__device__ void run_set(const MArgs& a, const uint32_t set, uint8_t* slot, Shared& sh, int* s_wtot, uint32_t* s_scan) {
    const uint32_t t = threadIdx.x;
    const MSet S = a.sets[set];
    G g; uint32_t *path, *colref;
    uint64_t pools = carve_pools(slot, S.sum_len, S.nseq, S.lmax, &g, &path, &colref);
    const uint64_t phase_at = pools;   // phase instances: the phase pool lies behind the graph pools (the plan's slot_pools_bytes)
    if constexpr (PHASE) pools += carve_phase(nullptr, S.sum_len, S.nseq, nullptr);
    if (pools > a.slot_bytes) { if (t == 0) a.status[set] = MS_GRAPH_OVERFLOW; return; }
    Cell<GM>* H = (Cell<GM>*)(slot + pools);
    const uint64_t hcap = (a.slot_bytes - pools) / sizeof(Cell<GM>);   // cells the slot holds
    // band instances: H is rcap rows of B cells, and behind it the rows' three word arrays (lo, m, best)
    BandRows br{};
    uint64_t rcap = 0;
    if constexpr (BAND) {
        static_assert(NT == BAND_NT && CPL == BAND_CPL && !GRAPH && !STRAND, "the band instances are one wavefront of 64 lanes x 16 columns, without graph output and strands");
        br.w = a.band_w[set]; br.B = 2 * br.w + 1;
        rcap = (a.slot_bytes - pools) / ((uint64_t)br.B * sizeof(Cell<GM>) + 12);
        br.lo = (uint32_t*)(slot + pools + rcap * br.B * sizeof(Cell<GM>)); br.m = br.lo + rcap; br.best = (int32_t*)(br.m + rcap);
    }
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
        if constexpr (BAND) {
            if (V) {
                if ((uint64_t)V + 1 > rcap) { if (t == 0) { a.status[set] = MS_H_OVERFLOW; a.vseen[set] = V; } return; }
                cells += (unsigned long long)V * min(br.B, L + 1);
                uint32_t bi, bj;
                // (a miss is the same value in every lane: dp_rows_band reads it behind its last barrier)
                if (dp_rows_band<GM>(g, H, br, V, s, L, a, sh, &bi, &bj)) { if (t == 0) a.status[set] = MS_BAND_MISS; return; }
                if (t == 0 && bi) na = traceback_band<GM>(g, H, br, s, L, bi, bj, a);
            }
        } else if (V) {
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
        if constexpr (LABELS) {
            static_assert(WTS && !GRAPH && !STRAND && !BAND, "the label instances are weighted ones, without graph output, strands and band");
            if constexpr (PHASE) {   // (writes the labels label_views reads; the pool's pointers are made here, so that none of them lives through the DP)
                PhasePool pp;
                carve_phase(slot + phase_at, S.sum_len, S.nseq, &pp);
                phase_reads<NT>(g, a, S, set, ncols, colr, pp, s_scan);
            }
            label_views<NT>(g, a, S, set, V, E, colr, sh, s_scan);   // (reads base_col as node ids)
        }
        // (a graph instance keeps base_col as node ids: there the column travels with the node)
        if (GRAPH) keep_graph<NT>(g, V, E, colr, a.go, set, b0, b0 + S.seq_begin);
        else for (uint64_t i = t; i < S.sum_len; i += NT) a.base_col[b0 + i] = colr[g.node2rank[a.base_col[b0 + i]]];
        if (LABELS) {   // (label_views has written the consensus places)
            if (t == 0) { a.n_cols[set] = ncols; a.cells[set] = cells; a.status[set] = MS_OK; }
        } else if (t < 64) {
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

template <int NT, int CPL, int GM, bool MSA, bool WTS, bool GRAPH = false, bool STRAND = false, bool BAND = false, bool LABELS = false>
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
        run_set<NT, CPL, GM, MSA, WTS, GRAPH, STRAND, BAND, LABELS, false>(a, a.order[q], slot, sh, s_wtot, s_scan);
    }
}

// The waves per SIMD a phase instance is compiled for: its label neighbour's (DESIGN.md "Two-haplotype consensus", resources). Left to
// itself the compiler gives the phase instances of 256 x 32 columns and of the small convex shapes a handful of registers more than 256,
// which halves their occupancy. The rule is written for the shapes of HX_POA_INSTANCES_LINEAR / _AFFINE / _CONVEX (poa_modes_plan.h) as
// they stand: 1 024 lanes are four waves per SIMD by themselves, the linear shapes of 16 columns per lane have three, every other shape
// two. The assertions below fail when those lists change; the rule and the table in DESIGN.md are then to be made again from a compile
// of the label instances with -Rpass-analysis=kernel-resource-usage.
constexpr int waves_per_simd(int nt, int cpl, int gm) { return nt == 1024 ? 4 : gm == GM_LINEAR && cpl == 16 ? 3 : 2; }
static_assert(INST_SHAPE[GM_LINEAR][0].nt == 64 && INST_SHAPE[GM_LINEAR][0].cpl == 16 && INST_SHAPE[GM_LINEAR][1].nt == 256 && INST_SHAPE[GM_LINEAR][1].cpl == 16 &&
              INST_SHAPE[GM_LINEAR][2].nt == 256 && INST_SHAPE[GM_LINEAR][2].cpl == 32 && INST_SHAPE[GM_LINEAR][3].nt == 1024 && INST_SHAPE[GM_AFFINE][2].nt == 512 &&
              INST_SHAPE[GM_AFFINE][3].nt == 1024 && INST_SHAPE[GM_CONVEX][1].nt == 128 && INST_SHAPE[GM_CONVEX][3].nt == 512 && N_INST == 4,
              "waves_per_simd() was made for these instance shapes");

// The phase instances (hx_poa_phased): k_poa_general's loop over run_set with LABELS and PHASE, as a kernel of their own, so that the
// occupancy attribute stands on them alone and the declaration of k_poa_general stays as it was.
template <int NT, int CPL, int GM>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(waves_per_simd(NT, CPL, GM)))) void k_poa_phase(MArgs a) {
    __shared__ Shared sh;
    __shared__ int s_wtot[(GM == GM_CONVEX ? 2 : 1) * (NT / 64)];
    __shared__ uint32_t s_scan[NT / 64];
    uint8_t* slot = a.ws + (size_t)blockIdx.x * a.slot_bytes;
    for (;;) {
        if (threadIdx.x == 0) sh.item = atomicAdd(a.counter, 1u);
        __syncthreads();
        const uint32_t q = sh.item;
        __syncthreads();
        if (q >= a.n_items) return;
        run_set<NT, CPL, GM, true, true, false, false, false, true, true>(a, a.order[q], slot, sh, s_wtot, s_scan);
    }
}

// the kernels of the instances (their shapes: INST_SHAPE, poa_modes_plan.h, from the same list). Each comes in three variants: the
// consensus alone (a consensus-only call runs the code it ran before the MSA existed), with the node of every base kept (the MSA; coverage
// needs it too), with base weights applied on top of that (hx_poa_weighted with weights), and with the graph and the alignments written out
// on top of that (hx_poa_graph; without weights it runs on weights of 1, which add nothing to an edge). A fifth variant, over the weighted
// one, aligns every sequence in both orientations and adds the better one (hx_poa_strand).
struct Inst { const void* variant[5]; };
#define HX_INST(GM, NT, CPL) {{(const void*)k_poa_general<NT, CPL, GM, false, false>, (const void*)k_poa_general<NT, CPL, GM, true, false>, (const void*)k_poa_general<NT, CPL, GM, true, true>, \
                               (const void*)k_poa_general<NT, CPL, GM, true, true, true>, (const void*)k_poa_general<NT, CPL, GM, true, true, false, true>}}
const Inst kInst[3][N_INST] = {{HX_POA_INSTANCES_LINEAR(HX_INST)}, {HX_POA_INSTANCES_AFFINE(HX_INST)}, {HX_POA_INSTANCES_CONVEX(HX_INST)}};
#undef HX_INST
static_assert(CELL_BYTES[GM_LINEAR] == sizeof(Cell<GM_LINEAR>) && CELL_BYTES[GM_AFFINE] == sizeof(Cell<GM_AFFINE>) && CELL_BYTES[GM_CONVEX] == sizeof(Cell<GM_CONVEX>), "CELL_BYTES against the cell types of poa_modes_dp.inl");
static_assert(GR_NODES == ROW_NODES && GR_EDGES == ROW_EDGES && GR_CNS == ROW_CNS && GR_ALN == ROW_ALN, "the plan's row kinds against k_graph_gather's");
// the band instances (BAND_INST, poa_modes_plan.h): one shape per gap model, in the three variants that keep no per-alignment pair pool
#define HX_BAND(GM) {{(const void*)k_poa_general<BAND_NT, BAND_CPL, GM, false, false, false, false, true>, (const void*)k_poa_general<BAND_NT, BAND_CPL, GM, true, false, false, false, true>, \
                      (const void*)k_poa_general<BAND_NT, BAND_CPL, GM, true, true, false, false, true>, nullptr, nullptr}}
const Inst kBand[3] = {HX_BAND(GM_LINEAR), HX_BAND(GM_AFFINE), HX_BAND(GM_CONVEX)};
#undef HX_BAND
static_assert(BAND_SHAPE.nt == BAND_NT && BAND_SHAPE.cpl == BAND_CPL && 2 * MAX_BAND + 1 <= BAND_NT * BAND_CPL, "the plan's band shape against the kernels'");
static_assert(MAX_LEN[GM_LINEAR] + 1 <= (BAND_SEQ_WORDS - 1) * 16, "the staged sequence of the band instances against the longest sequence");
// the label instances (hx_poa_labelled; DESIGN.md "Per-label consensus"): the weighted variant of every shape with the per-label views behind its last sort
#define HX_LABEL(GM, NT, CPL) (const void*)k_poa_general<NT, CPL, GM, true, true, false, false, false, true>
const void* const kLabel[3][N_INST] = {{HX_POA_INSTANCES_LINEAR(HX_LABEL)}, {HX_POA_INSTANCES_AFFINE(HX_LABEL)}, {HX_POA_INSTANCES_CONVEX(HX_LABEL)}};
#undef HX_LABEL
// the phase instances (hx_poa_phased; DESIGN.md "Two-haplotype consensus"): the label instance of every shape with the phasing of the set's reads in front of its views
#define HX_PHASE(GM, NT, CPL) (const void*)k_poa_phase<NT, CPL, GM>
const void* const kPhase[3][N_INST] = {{HX_POA_INSTANCES_LINEAR(HX_PHASE)}, {HX_POA_INSTANCES_AFFINE(HX_PHASE)}, {HX_POA_INSTANCES_CONVEX(HX_PHASE)}};
#undef HX_PHASE
inline const void* fn(const Inst& inst, bool cols, bool weighted, bool graph, bool strand) { return inst.variant[strand ? 4 : graph ? 3 : weighted ? 2 : cols ? 1 : 0]; }

template <class T> struct Buf {   // device buffer of one call
    T* p = nullptr;
    hipError_t alloc(size_t n) { return hipMalloc((void**)&p, std::max<size_t>(n, 1) * sizeof(T)); }
    hipError_t fill(int byte, size_t n, hipStream_t s) { return hipMemsetAsync(p, byte, std::max<size_t>(n, 1) * sizeof(T), s); }   // every byte of the n elements
    hipError_t download(T* to, size_t n) const { return hipMemcpy(to, p, n * sizeof(T), hipMemcpyDeviceToHost); }
    ~Buf() { if (p) (void)hipFree(p); }
};

// the device half of a work list (RowPlan, poa_modes_plan.h): the plan's rows as the kernel's descriptors, and the chunks
template <class Row> struct RowList {
    std::vector<Row> rows;
    Buf<Row> d_rows; Buf<uint2> d_chunks;
    template <class P, class F> hipError_t upload(const RowPlan<P>& plan, hipStream_t s, F to_row) {
        for (const P& r : plan.rows) rows.push_back(to_row(r));
        hipError_t e = d_rows.alloc(rows.size());
        if (e == hipSuccess) e = d_chunks.alloc(plan.chunks.size());
        if (e == hipSuccess) e = hipMemcpyAsync(d_rows.p, rows.data(), rows.size() * sizeof(Row), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(d_chunks.p, plan.chunks.data(), plan.chunks.size() * sizeof(uint2), hipMemcpyHostToDevice, s);
        return e;
    }
};

#define MCHK(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) { err = std::string(#expr) + ": " + hipGetErrorString(e_); return -1; } } while (0)

// one call of poa_modes_run: what its stages share. Every stage returns 0, or -1 with the reason in err. The arithmetic of every stage is
// the plan's (c, st: poa_modes_plan.h); this keeps the buffers, the uploads, the launches and the downloads.
struct Run {
    hipStream_t s; PoaModesWs& ws; const PoaModesArgs& a; PoaModesOut& o; std::string& err;
    ModesCall c; ModesState st;
    std::vector<uint32_t> len;       // per set: the length of its consensus (after consensus())
    int n_cu = 0;
    uint64_t budget = 0;
    Buf<MSet> d_sets; Buf<uint8_t> d_codes; Buf<uint64_t> d_soff; Buf<uint32_t> d_order, d_counter, d_status, d_vseen, d_cns_len; Buf<unsigned long long> d_cells; Buf<char> d_cns;
    Buf<uint32_t> d_base_col, d_n_cols, d_cns_col;   // MSA and weighted calls only
    Buf<uint8_t> d_labels;                           // labelled calls only: a label per sequence (phased calls: written by the kernel)
    Buf<uint32_t> d_n_haps, d_rounds, d_n_sites, d_site_col, d_site_inf;   // phased calls only: what PhaseArgs points to
    Buf<uint32_t> d_band;                            // banded calls only: per set the half-width of its current attempt
    Buf<uint8_t> d_wts;                              // weighted calls with weights only: a byte per base (graph and strand calls: always, 1 without weights)
    // strand calls only: what StrandArgs points to
    Buf<uint8_t> d_codes_rc, d_wts_rc, d_codes_used, d_wts_used, d_reversed; Buf<int32_t> d_score_fwd, d_score_rev; Buf<uint32_t> d_third;
    // graph calls only: what GraphOutArgs points to. The alignment pool is one allocation per round (st.pool_of names it)
    struct Pool { Buf<int32_t> node, pos; };
    std::vector<std::unique_ptr<Pool>> pools;
    Buf<uint64_t> d_aln_at; Buf<uint32_t> d_aln_room, d_aln_need, d_aln_cnt, d_n_nodes, d_n_edges, d_node_rank, d_node_col, d_edge_from, d_edge_to, d_cns_node;
    Buf<int32_t> d_aln_score, d_edge_w; Buf<uint8_t> d_node_code;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~Run() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }

    const void* fn_of(int k) const { return c.phase ? kPhase[c.gm][k] : c.labels ? kLabel[c.gm][k] : fn(k == BAND_INST ? kBand[c.gm] : kInst[c.gm][k], c.cols, d_wts.p != nullptr, c.graph, c.strand); }
    const uint8_t* codes_as_added() const { return c.strand ? d_codes_used.p : d_codes.p; }   // what the row, coverage and profile kernels read

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

    // ---- the sets checked and described (the plan's describe), the call's inputs on the device, the memory budget
    int prepare() {
        o = PoaModesOut();
        const int bad = describe(a, c, st, err);
        o.seq_bases = c.seq_bases; o.n_aligned = c.n_aligned;
        if (bad) return -1;
        const uint32_t ns = c.ns;
        const uint64_t nseq = c.nseq, nb = c.nb, ncns = c.cns_off.back(), nlen = (uint64_t)ns * c.nl;
        int dev = 0;
        MCHK(hipGetDevice(&dev));
        MCHK(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev));
        MCHK(d_sets.alloc(ns)); MCHK(d_codes.alloc(c.codes.size())); MCHK(d_soff.alloc(nseq + 1)); MCHK(d_order.alloc(ns)); MCHK(d_counter.alloc(N_SLOTS));
        MCHK(d_status.alloc(ns)); MCHK(d_vseen.alloc(ns)); MCHK(d_cns_len.alloc(nlen)); MCHK(d_cells.alloc(ns)); MCHK(d_cns.alloc(ncns));
        MCHK(hipMemcpyAsync(d_sets.p, c.sets.data(), ns * sizeof(MSet), hipMemcpyHostToDevice, s));
        MCHK(hipMemcpyAsync(d_codes.p, c.codes.data(), c.codes.size(), hipMemcpyHostToDevice, s));   // (the codes live to the end of the call)
        MCHK(hipMemcpyAsync(d_soff.p, a.seq_off, (nseq + 1) * 8, hipMemcpyHostToDevice, s));
        MCHK(d_cns_len.fill(0, nlen, s));
        MCHK(d_cells.fill(0, ns, s));
        if (c.band) MCHK(d_band.alloc(ns));
        if (c.cols) {
            MCHK(d_base_col.alloc(nb)); MCHK(d_n_cols.alloc(ns));
            MCHK(d_n_cols.fill(0, ns, s));
            if ((c.msa && a.include_consensus) || c.want_cov || c.labels) MCHK(d_cns_col.alloc(ncns));
        }
        if ((c.wtd || c.graph || c.strand || c.labels) && a.weights) {
            MCHK(d_wts.alloc(nb));
            MCHK(hipMemcpyAsync(d_wts.p, a.weights, nb, hipMemcpyHostToDevice, s));
        }
        if ((c.graph || c.strand || c.labels) && !a.weights) { MCHK(d_wts.alloc(nb)); MCHK(d_wts.fill(1, nb, s)); }
        if (c.labels && !c.phase) { MCHK(d_labels.alloc(nseq)); MCHK(hipMemcpyAsync(d_labels.p, a.labels, nseq, hipMemcpyHostToDevice, s)); }
        if (c.phase) {   // (a set without a base runs nowhere: its sequences keep 255, its counts 0)
            MCHK(d_labels.alloc(nseq)); MCHK(d_n_haps.alloc(ns)); MCHK(d_rounds.alloc(ns)); MCHK(d_n_sites.alloc(ns)); MCHK(d_site_col.alloc(nb)); MCHK(d_site_inf.alloc(nb));
            MCHK(d_labels.fill(0xff, nseq, s)); MCHK(d_n_haps.fill(0, ns, s)); MCHK(d_rounds.fill(0, ns, s)); MCHK(d_n_sites.fill(0, ns, s));
        }
        if (c.strand) {
            MCHK(d_codes_rc.alloc(nb)); MCHK(d_codes_used.alloc(nb)); MCHK(d_wts_used.alloc(nb));
            MCHK(d_reversed.alloc(nseq)); MCHK(d_score_fwd.alloc(nseq)); MCHK(d_score_rev.alloc(nseq)); MCHK(d_third.alloc(ns));
            MCHK(hipMemcpyAsync(d_codes_rc.p, c.codes_rc.data(), nb, hipMemcpyHostToDevice, s));
            if (a.weights) { MCHK(d_wts_rc.alloc(nb)); MCHK(hipMemcpyAsync(d_wts_rc.p, c.wts_rc.data(), nb, hipMemcpyHostToDevice, s)); }   // (without weights: d_wts, all 1, is its own reverse)
            // (an empty sequence and a set's first non-empty one keep flag 0 and scores 0; a set without a base writes no count)
            MCHK(d_reversed.fill(0, nseq, s)); MCHK(d_score_fwd.fill(0, nseq, s));
            MCHK(d_score_rev.fill(0, nseq, s)); MCHK(d_third.fill(0, ns, s));
        }
        if (c.graph) {
            const uint64_t ne = nb + nseq;   // (a set's edges start at its first base's offset plus its first sequence's index)
            MCHK(d_aln_at.alloc(ns)); MCHK(d_aln_room.alloc(ns)); MCHK(d_aln_need.alloc(ns)); MCHK(d_aln_cnt.alloc(nseq)); MCHK(d_aln_score.alloc(nseq));
            MCHK(d_n_nodes.alloc(ns)); MCHK(d_n_edges.alloc(ns)); MCHK(d_node_code.alloc(nb)); MCHK(d_node_rank.alloc(nb)); MCHK(d_node_col.alloc(nb));
            MCHK(d_edge_from.alloc(ne)); MCHK(d_edge_to.alloc(ne)); MCHK(d_edge_w.alloc(ne)); MCHK(d_cns_node.alloc(ncns));
            // (a sequence that meets no DP writes neither: its alignment is empty, its score 0; a set without a base writes no counts)
            MCHK(d_aln_cnt.fill(0, nseq, s)); MCHK(d_aln_score.fill(0, nseq, s));
            MCHK(d_n_nodes.fill(0, ns, s)); MCHK(d_n_edges.fill(0, ns, s));
        }
        size_t fr = 0, tot = 0;
        MCHK(hipMemGetInfo(&fr, &tot));
        budget = a.workspace_gb > 0 ? (uint64_t)(a.workspace_gb * 1e9) : (uint64_t)((double)(fr + ws.cap) * 0.4);
        MCHK(hipEventCreate(&e0)); MCHK(hipEventCreate(&e1));
        return 0;
    }

    // ---- one round over st.todo: plan (plan_round), launch, collect; the sets that outgrew their slot are todo again (after_round)
    int round(const bool first) {
        const uint32_t ns = c.ns;
        uint64_t resident[N_SLOTS] = {};   // workgroups the device holds, asked for the instances that have sets
        for (int k = 0; k < N_SLOTS; k++) {
            if (std::none_of(st.todo.begin(), st.todo.end(), [&](uint32_t i) { return slot_of(c, st, i) == k; })) continue;
            int occ = 0;
            MCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn_of(k), shape_of(c.gm, k).nt, 0));
            resident[k] = (uint64_t)std::max(1, occ) * (uint64_t)n_cu;
        }
        RoundPlan p;
        if (plan_round(c, st, first, budget, resident, p, err)) return -1;
        if (p.total > ws.cap) {
            MCHK(hipStreamSynchronize(s));
            ws.release();
            const hipError_t e = hipMalloc(&ws.p, p.total);
            if (e != hipSuccess) { ws.p = nullptr; err = c.who + ": the workspace of " + std::to_string(p.total) + " bytes could not be allocated: " + hipGetErrorString(e); return -1; }
            ws.cap = p.total;
        }
        o.workspace_bytes = std::max(o.workspace_bytes, p.total);
        if (c.band) MCHK(hipMemcpyAsync(d_band.p, st.band.data(), ns * 4, hipMemcpyHostToDevice, s));   // (st.band stays as it is until after_round, behind the round's last download)
        GraphOutArgs go{};
        if (c.graph) {   // this round's pool
            pools.emplace_back(new Pool);
            Pool& P = *pools.back();
            {
                hipError_t e = P.node.alloc(p.aln_pairs);
                if (e == hipSuccess) e = P.pos.alloc(p.aln_pairs);
                if (e != hipSuccess) { err = c.who + ": the alignment pool of " + std::to_string(p.aln_pairs) + " pairs could not be allocated on the device: " + hipGetErrorString(e); return -1; }
            }
            MCHK(hipMemcpyAsync(d_aln_at.p, st.aln_at.data(), ns * 8, hipMemcpyHostToDevice, s));
            MCHK(hipMemcpyAsync(d_aln_room.p, st.aln_room.data(), ns * 4, hipMemcpyHostToDevice, s));
            go = GraphOutArgs{P.node.p, P.pos.p, d_aln_at.p, d_aln_room.p, d_aln_need.p, d_aln_cnt.p, d_aln_score.p, d_node_code.p, d_node_rank.p, d_node_col.p, d_n_nodes.p,
                              d_edge_from.p, d_edge_to.p, d_edge_w.p, d_n_edges.p, d_cns_node.p};
        }
        MCHK(hipMemcpyAsync(d_order.p, p.order.data(), p.order.size() * 4, hipMemcpyHostToDevice, s));
        MCHK(d_counter.fill(0, N_SLOTS, s));
        MCHK(d_status.fill(0xff, ns, s));
        float ms = 0;
        if (timed(&ms, [&] {
                for (int k = 0; k < N_SLOTS; k++) {
                    const RoundPlan::PerInst& pk = p.inst[k];
                    if (pk.sets.empty()) continue;
                    MArgs q{d_sets.p, d_order.p + pk.base, (uint32_t)pk.sets.size(), d_counter.p + k, d_codes.p, d_soff.p, (uint8_t*)ws.p, pk.slot,
                            a.match, a.mismatch, a.gap, a.type, d_cns.p, d_cns_len.p, d_status.p, d_vseen.p, d_cells.p, a.gap_extend,
                            d_base_col.p, d_n_cols.p, d_cns_col.p, d_wts.p, a.gap_open2, a.gap_extend2, go,
                            StrandArgs{d_codes_rc.p, d_wts_rc.p ? d_wts_rc.p : d_wts.p, d_codes_used.p, d_wts_used.p, d_reversed.p, d_score_fwd.p, d_score_rev.p, d_third.p}, d_band.p, d_labels.p, c.nl,
                            PhaseArgs{d_labels.p, d_n_haps.p, d_rounds.p, d_n_sites.p, d_site_col.p, d_site_inf.p, a.phase_min_count, a.phase_min_pct}};
                    void* kargs[] = {&q};
                    MCHK(hipLaunchKernel(fn_of(k), dim3(pk.nslots), dim3((uint32_t)shape_of(c.gm, k).nt), kargs, 0, s));
                    o.launches++;
                    if (a.debug) fprintf(stderr, "[hx] POA modes%s: %zu sets on %u workgroups of %d lanes x %d columns, slots of %.1f MB\n", gap_model_label(c.gm), pk.sets.size(), pk.nslots, shape_of(c.gm, k).nt, shape_of(c.gm, k).cpl, pk.slot / 1e6);
                }
                return 0;
            })) return -1;
        o.kernel_ms += ms;
        std::vector<uint32_t> status(ns), vseen(ns), pairs;   // (pairs: what the alignments of a set hold in all)
        MCHK(d_status.download(status.data(), ns));
        MCHK(d_vseen.download(vseen.data(), ns));
        if (c.graph) { pairs.resize(ns); MCHK(d_aln_need.download(pairs.data(), ns)); }
        if (c.band) {   // the half-width a set finished with, before after_round moves the others on
            o.band_used.resize(ns, 0);
            for (uint32_t i : st.todo) if (status[i] == MS_OK) o.band_used[i] = st.band[i];
        }
        const int bad = after_round(c, st, first, status.data(), vseen.data(), pairs.data(), err);
        o.retried = st.retried; o.aln_retried = st.aln_retried; o.band_reruns = st.band_retried;
        return bad;
    }

    // ---- the consensus strings and the cell counts, after the last round
    int consensus() {
        const uint32_t ns = c.ns;
        const uint64_t nseq = c.nseq, nlen = (uint64_t)ns * c.nl, ncns = c.cns_off.back();
        len.resize(nlen);
        std::vector<unsigned long long> cells(ns);
        std::vector<char> cns(std::max<uint64_t>(1, ncns));
        MCHK(d_cns_len.download(len.data(), nlen));
        MCHK(d_cells.download(cells.data(), ns));
        MCHK(d_cns.download(cns.data(), ncns));
        if (c.band) o.band_used.resize(ns, 0);   // (a call without a round: no set has a base)
        o.cns_off.assign((size_t)nlen + 1, 0);
        for (uint64_t j = 0; j < nlen; j++) {
            o.cns.append(cns.data() + c.cns_off[j], len[j]);
            o.cns_off[j + 1] = o.cns.size();
        }
        for (uint32_t i = 0; i < ns; i++) o.cells += cells[i];
        if (c.labels) {   // the columns of the consensus bases, dense like the strings
            std::vector<uint32_t> col(std::max<uint64_t>(1, ncns));
            MCHK(d_cns_col.download(col.data(), ncns));
            for (uint64_t j = 0; j < nlen; j++) o.cns_col.insert(o.cns_col.end(), col.begin() + c.cns_off[j], col.begin() + c.cns_off[j] + len[j]);
        }
        if (c.phase && phase_out()) return -1;
        if (c.strand) {   // (a set that was rerun rewrote its own part)
            std::vector<uint32_t> third(ns);
            o.reversed.assign(nseq, 0); o.score_fwd.assign(nseq, 0); o.score_rev.assign(nseq, 0);
            MCHK(d_third.download(third.data(), ns));
            if (nseq) { MCHK(d_reversed.download(o.reversed.data(), nseq)); MCHK(d_score_fwd.download(o.score_fwd.data(), nseq)); MCHK(d_score_rev.download(o.score_rev.data(), nseq)); }
            for (uint32_t i = 0; i < ns; i++) o.third_passes += third[i];
        }
        return 0;
    }

    // ---- the haplotypes and the sites of a phased call (a set that was rerun rewrote its own part): the sites dense, set after set. The
    // haplotypes are from here on the labels the plan of the coverage reads (c.lab)
    int phase_out() {
        const uint32_t ns = c.ns;
        const uint64_t nseq = c.nseq, nb = c.nb;
        std::vector<uint32_t> n_sites(ns), col(std::max<uint64_t>(1, nb)), inf(std::max<uint64_t>(1, nb));
        o.hap.assign(std::max<uint64_t>(1, nseq), 255); o.n_haps.assign(ns, 1); o.phase_rounds.assign(ns, 0); o.site_off.assign((size_t)ns + 1, 0);
        if (nseq) MCHK(d_labels.download(o.hap.data(), nseq));
        o.hap.resize(nseq);
        if (ns) { MCHK(d_n_haps.download(o.n_haps.data(), ns)); MCHK(d_rounds.download(o.phase_rounds.data(), ns)); MCHK(d_n_sites.download(n_sites.data(), ns)); }
        if (nb) { MCHK(d_site_col.download(col.data(), nb)); MCHK(d_site_inf.download(inf.data(), nb)); }
        for (uint32_t i = 0; i < ns; i++) {
            if (!c.sets[i].sum_len) o.n_haps[i] = 1;   // (no base: one haplotype without a member)
            if (n_sites[i] > c.sets[i].sum_len) { err = c.who + ": internal error (set " + std::to_string(i) + " reports " + std::to_string(n_sites[i]) + " sites on " + std::to_string(c.sets[i].sum_len) + " bases)"; return -1; }
            const uint64_t b0 = a.seq_off[a.set_off[i]];
            for (uint32_t j = 0; j < n_sites[i]; j++) {
                o.site_col.push_back(col[b0 + j]); o.site_a1.push_back((uint8_t)(inf[b0 + j] & 15u)); o.site_a2.push_back((uint8_t)(inf[b0 + j] >> 4 & 15u));
                o.site_phase.push_back((int8_t)((int)(inf[b0 + j] >> 8 & 3u) - 1));
            }
            o.site_off[i + 1] = o.site_col.size();
        }
        c.lab = o.hap.data();
        return 0;
    }

    // ---- coverage and profile: now that the columns of every set are known (plan_coverage). Built here, after the last round: a set
    // that was rerun is counted once.
    int coverage() {
        std::vector<uint32_t> ncols(c.ns);
        MCHK(d_n_cols.download(ncols.data(), c.ns));
        CovPlan p;
        if (plan_coverage(c, ncols, len, o.cns_off, p, err)) return -1;
        const uint64_t nc = p.nc;
        const uint32_t stride = p.stride;
        o.cov.assign(nc, 0);
        if (a.want_profile) o.prof.assign(4 * nc, 0);
        if (!nc) return 0;
        RowList<CRow> seqs, cnss;
        Buf<uint32_t> d_hist, d_cov, d_prof;
        auto to_row = [](const CovRow& r) { return CRow{r.src, r.dst, r.hoff, r.len, r.ncols}; };
        MCHK(seqs.upload(p.seqs, s, to_row)); MCHK(cnss.upload(p.cnss, s, to_row));
        MCHK(d_hist.alloc(p.hist_words)); MCHK(d_cov.alloc(nc));
        if (a.want_profile) MCHK(d_prof.alloc(4 * nc));
        float cov_ms = 0;
        if (timed(&cov_ms, [&] {
                MCHK(d_hist.fill(0, p.hist_words, s));
                if (p.seqs.n_chunks()) {
                    k_cov_hist<<<p.seqs.blocks(), 256, 0, s>>>(seqs.d_rows.p, seqs.d_chunks.p, p.seqs.n_chunks(), d_base_col.p, codes_as_added(), stride, d_hist.p);
                    MCHK(hipGetLastError());
                    o.launches++;
                }
                k_cov_gather<<<p.cnss.blocks(), 256, 0, s>>>(cnss.d_rows.p, cnss.d_chunks.p, p.cnss.n_chunks(), d_cns_col.p, d_hist.p, stride, d_cov.p, d_prof.p);
                MCHK(hipGetLastError());
                return 0;
            })) return -1;
        o.cov_ms = cov_ms; o.kernel_ms += cov_ms; o.launches++;
        o.cov_moved_bytes = p.moved_bytes;
        MCHK(d_cov.download(o.cov.data(), nc));
        if (a.want_profile) MCHK(d_prof.download(o.prof.data(), 4 * nc));
        return 0;
    }

    // ---- the graph and the alignments: now that the host knows the nodes, edges and pairs of every set (plan_graph_out), one grid-wide
    // kernel moves them from the worst-case places run_set wrote them to into dense arrays, set after set (codes become letters, an
    // alignment's pairs are turned into forward order), and only those are downloaded. Built here, after the last round: a set that was
    // rerun is taken from the round it finished in, once.
    int graph_out() {
        const uint32_t ns = c.ns;
        const uint64_t nseq = c.nseq, nb = c.nb;
        std::vector<uint32_t> nv(ns), ne(ns), cnt(nseq);
        o.aln_score.assign(nseq, 0);
        MCHK(d_n_nodes.download(nv.data(), ns));
        MCHK(d_n_edges.download(ne.data(), ns));
        MCHK(d_aln_cnt.download(cnt.data(), nseq));
        MCHK(d_aln_score.download(o.aln_score.data(), nseq));
        GraphPlan p;
        const int bad = plan_graph_out(c, st, nv, ne, cnt, len, o.cns_off, p, err);
        o.node_off = p.node_off; o.edge_off = p.edge_off; o.aln_off = p.aln_off;   // (as far as the plan came, when it failed)
        if (bad) return -1;
        const uint64_t NV = p.NV, NE = p.NE, NC = p.NC, NP = p.NP;
        o.node_base.resize(NV); o.node_rank.resize(NV); o.node_col.resize(NV);
        o.edge_from.resize(NE); o.edge_to.resize(NE); o.edge_w.resize(NE);
        o.cns_node.resize(NC); o.aln_node.resize(NP); o.aln_pos.resize(NP);
        o.base_node.resize(nb);
        if (nb) MCHK(d_base_col.download(o.base_node.data(), nb));   // (dense as it is: the layout of the call's bases)
        if (p.rows.n_chunks() == 0) return 0;
        RowList<GRow> rows;   // (an alignment's row reads the pool of the round its set finished in)
        Buf<char> o_base; Buf<uint32_t> o_rank, o_col, o_from, o_to, o_cns; Buf<int32_t> o_w, o_an, o_ap;
        MCHK(o_base.alloc(NV)); MCHK(o_rank.alloc(NV)); MCHK(o_col.alloc(NV)); MCHK(o_from.alloc(NE)); MCHK(o_to.alloc(NE)); MCHK(o_w.alloc(NE));
        MCHK(o_cns.alloc(NC)); MCHK(o_an.alloc(NP)); MCHK(o_ap.alloc(NP));
        MCHK(rows.upload(p.rows, s, [&](const GraphRow& r) {
            const Pool* P = r.kind == ROW_ALN ? pools[r.round].get() : nullptr;
            return GRow{P ? P->node.p : nullptr, P ? P->pos.p : nullptr, r.src, r.dst, r.len, r.kind};
        }));
        const GatherArgs ga{d_node_code.p, d_node_rank.p, d_node_col.p, d_edge_from.p, d_edge_to.p, d_edge_w.p, d_cns_node.p,
                            o_base.p, o_rank.p, o_col.p, o_from.p, o_to.p, o_w.p, o_cns.p, o_an.p, o_ap.p};
        float ms = 0;
        if (timed(&ms, [&] {
                k_graph_gather<<<p.rows.blocks(), 256, 0, s>>>(rows.d_rows.p, rows.d_chunks.p, p.rows.n_chunks(), ga);
                MCHK(hipGetLastError());
                return 0;
            })) return -1;
        o.gather_ms = ms; o.kernel_ms += ms; o.launches++;
        o.gather_moved_bytes = p.moved_bytes;
        if (NV) { MCHK(o_base.download(&o.node_base[0], NV)); MCHK(o_rank.download(o.node_rank.data(), NV)); MCHK(o_col.download(o.node_col.data(), NV)); }
        if (NE) { MCHK(o_from.download(o.edge_from.data(), NE)); MCHK(o_to.download(o.edge_to.data(), NE)); MCHK(o_w.download(o.edge_w.data(), NE)); }
        if (NC) MCHK(o_cns.download(o.cns_node.data(), NC));
        if (NP) { MCHK(o_an.download(o.aln_node.data(), NP)); MCHK(o_ap.download(o.aln_pos.data(), NP)); }
        return 0;
    }

    // ---- the MSA text: now that the columns of every set are known (plan_msa)
    int msa_text() {
        o.msa_cols.assign(c.ns, 0);
        MCHK(d_n_cols.download(o.msa_cols.data(), c.ns));
        MsaPlan p;
        const int bad = plan_msa(c, o.msa_cols, len, o.cns_off, p, err);
        o.msa_rows = p.msa_rows; o.msa_off = p.msa_off;
        if (bad) return -1;
        const uint64_t out_bytes = p.out_bytes;
        o.msa.resize(out_bytes);
        if (out_bytes == 0) return 0;
        RowList<MRow> rows;
        Buf<char> d_out;
        {
            const hipError_t e = d_out.alloc(out_bytes);
            if (e != hipSuccess) { err = c.who + ": the " + std::to_string(out_bytes) + " bytes of the alignment text could not be allocated on the device: " + hipGetErrorString(e); return -1; }
        }
        MCHK(rows.upload(p.rows, s, [](const MsaRow& r) { return MRow{r.src, r.dst, r.len, r.ncols, r.is_cns, 0}; }));
        float rows_ms = 0;
        if (timed(&rows_ms, [&] {
                k_msa_rows<<<p.rows.blocks(), 256, 0, s>>>(rows.d_rows.p, rows.d_chunks.p, p.rows.n_chunks(), d_base_col.p, codes_as_added(), d_cns_col.p, d_cns.p, d_out.p);
                MCHK(hipGetLastError());
                return 0;
            })) return -1;
        o.msa_rows_ms = rows_ms; o.kernel_ms += rows_ms; o.launches++;
        o.msa_moved_bytes = p.moved_bytes;
        MCHK(d_out.download(&o.msa[0], out_bytes));
        return 0;
    }
};

}  // namespace

int poa_modes_run(hipStream_t s, PoaModesWs& ws, const PoaModesArgs& a, PoaModesOut& o, std::string& err) {
    Run r{s, ws, a, o, err};
    if (r.prepare()) return -1;
    for (bool first = true; !r.st.todo.empty(); first = false)
        if (r.round(first)) return -1;
    if (r.consensus()) return -1;
    if (r.c.want_cov && r.coverage()) return -1;
    if (r.c.graph) return r.graph_out();
    return r.c.msa ? r.msa_text() : 0;
}

}  // namespace hxk
