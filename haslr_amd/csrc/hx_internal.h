// hx_internal.h - what the units of the C-ABI share (hx_api.hip, hx_poa_plan.hip, hx_poa.hip, hx_group.hip): the error helpers, device
// buffers (the column buffers of the chain, edge and coordinate operators generated from the lists of hx_columns.h), the POA workspace arena, the options of a context, the shape of its last consensus call (for hx_poa_report.cpp) and the context itself.
#pragma once
#include <atomic>
#include <thread>
#include <memory>
#include <chrono>
#include <cmath>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>
#include <array>
#include <mutex>

#include "../../include/haslr_hip.h"
#include "host/haslr_host.h"
#include "kernels/kernels.h"
#include "kernels/poa_modes.h"
#include "hx_poa_report.h"
#include "hx_poa_pools.h"
#include "hx_columns.h"

namespace hxi {

extern thread_local std::string g_err;   // what hx_last_error returns (hx_api.hip)
int fail(const std::string& m);          // sets it, returns -1

#define HIPCHK(expr)                                                                                          \
    do {                                                                                                      \
        hipError_t _e = (expr);                                                                               \
        if (_e != hipSuccess) return hxi::fail(std::string(#expr) + ": " + hipGetErrorString(_e));            \
    } while (0)

template <class T>
struct DV {   // device vector (capacity grows, never shrinks)
    T* p = nullptr;
    size_t cap = 0;
    hipError_t reserve(size_t n) {
        if (n <= cap && p) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        hipError_t e = hipMalloc((void**)&p, std::max<size_t>(n, 1) * sizeof(T));
        if (e == hipSuccess) cap = std::max<size_t>(n, 1);
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    ~DV() { release(); }
};

template <class T>
int up(DV<T>& d, const T* h, size_t n) {
    HIPCHK(d.reserve(n));
    if (n) HIPCHK(hipMemcpy(d.p, h, n * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}

// A result array on the host: malloc(max(1, n)), so that an empty result still has a pointer. False when the allocation or the download fails; what
// was allocated stays in `out` for the caller's hx_free_*.
template <class T> bool fetch(T*& out, const T* d, size_t n) {
    out = (T*)malloc(std::max<size_t>(1, n) * sizeof(T));
    return out && (!n || hipMemcpy(out, d, n * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess);
}

// The buffers of a column list (hx_columns.h): one DV per entry under the kernels' name, reserved together, handed to a kernel's struct by member
// name (fill: the struct's other members are the caller's), downloaded into and freed from a public struct by field name.
#define HX_COLUMN_BUFS(Name, LIST) struct Name { \
        LIST(HX_COL_BUF) \
        hipError_t reserve(size_t n) { hipError_t e; LIST(HX_COL_RESERVE) return hipSuccess; } \
        template <class V> void fill(V& v) const { LIST(HX_COL_VIEW) } \
        template <class O> bool download(O* o, size_t n) const { bool ok = true; LIST(HX_COL_FETCH) return ok; } \
        template <class O> static void free_host(O* o) { LIST(HX_COL_FREE) } \
    }
HX_COLUMN_BUFS(ChainCols, HX_CHAIN_COLUMNS); HX_COLUMN_BUFS(DevSideBuf, HX_SIDE_COLUMNS); HX_COLUMN_BUFS(RecCols, HX_REC_COLUMNS);
HX_COLUMN_BUFS(CoordEdgeCols, HX_COORD_EDGE_COLUMNS); HX_COLUMN_BUFS(CoordSuppCols, HX_COORD_SUPP_COLUMNS);
struct HitCols {   // resident raw hits, each uploaded at its own count
    HX_HIT_COLUMNS(HX_COL_BUF)
    int upload(const hx_hits* h, uint64_t n_ops) { const size_t n = h->n; HX_HIT_COLUMNS(HX_COL_UPLOAD) return 0; }
    DevHits view(uint64_t n) const { DevHits v{}; v.n = n; HX_HIT_COLUMNS(HX_COL_VIEW) return v; }
};
struct RecBuf : RecCols {
    DevSideBuf head, tail;
    hipError_t reserve(size_t n) { hipError_t e; if ((e = RecCols::reserve(n)) || (e = head.reserve(n))) return e; return tail.reserve(n); }
    hxk::EdgeRecs view() const { hxk::EdgeRecs v{}; fill(v); head.fill(v.head); tail.fill(v.tail); return v; }
};
struct CoordCols {   // per selected edge, and per support with the host mirrors that hx_poa_batch reads: copies of what was downloaded
    CoordEdgeCols edge;
    CoordSuppCols supp;
    HX_COORD_SUPP_COLUMNS(HX_COL_MIRROR)
    std::vector<uint64_t> h_supp_off;   // n_sel + 1: the scan of the supports kept per edge
    uint32_t n_sel = 0;
    void keep(const hx_coords_out* o, size_t n) { h_supp_off.assign(o->supp_off, o->supp_off + n_sel + 1); HX_COORD_SUPP_COLUMNS(HX_COL_MIRROR_KEEP) }
};

struct Timer {
    hipEvent_t a = nullptr, b = nullptr;
    double ms[4] = {0, 0, 0, 0};
    uint64_t launches[4] = {0, 0, 0, 0};
};

// The POA workspace is ONE device allocation (round 6): an arena that every pool of a batch is carved out of. Forty pools used to be forty synchronous
// hipMalloc calls inside the first consensus call of a context - seconds of a one-shot run at 140 Mb (215 GB), against a 0.5 s hot path. The arena can be
// reserved ahead of the first call (hx_poa_reserve: the CLI does it on a thread of its own while the text inputs are parsed), grows when a batch needs
// more (never shrinks), and is carved anew for every batch: nothing in it outlives a batch. The pools and their list: hx_poa_pools.h.
struct PoaArena {
    uint8_t* p = nullptr;
    size_t cap = 0;
    uint64_t n_alloc = 0;       // device allocations made for it so far
    double alloc_ms = 0;        // ... and the wall time they took
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    hipError_t ensure(size_t bytes) {   // at least `bytes`; the contents are not kept
        if (bytes <= cap && p) return hipSuccess;
        const auto t0 = std::chrono::steady_clock::now();
        release();
        const hipError_t e = hipMalloc((void**)&p, std::max<size_t>(bytes, 256));
        if (e == hipSuccess) cap = std::max<size_t>(bytes, 256); else p = nullptr;
        n_alloc++; alloc_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return e;
    }
    ~PoaArena() { release(); }
};

// ---- tuning and test switches of a context. They used to be HX_* environment variables read inside the library on every call; now they are
// state of the context, set through hx_set_option (include/haslr_hip.h) - by the applications (the CLI and haslr_amd/hip.py copy the HX_*
// variables of their environment in, once, when they create a context) and by the tests. Defaults in the table below; -1 = automatic.
struct HxOptions {
    int debug = 0;                 // progress and statistics of every consensus call on stderr
    int prof = 0;                  // 1 / 2 / 3 / 4: how hx_poa_phase_cycles reads words 6-11 of a build with -DHX_DP_PROF / PROF2 / PROF3 / PROF4 (development: POA_PHASE_FLAVOUR, kernels/poa_phase_words.h)
    double poa_workspace_gb = 0;   // cap of the POA workspace in GB (0: 90 % of the memory that was free at the context's first consensus call)
    int poa_poll_limit = 1 << 24;  // polls before a wave gives up waiting for another member (testing: forces the unshared retry)
    int poa_max_indeg = 16;        // in-degree the direction bytes hold (testing: forces the score-matrix retry earlier)
    int poa_member_lanes = 256, poa_cluster_min = 2048, poa_cluster_max = -1, poa_cluster_topk = -1, poa_wide_members = -1, poa_cluster_cols = -1;
    int poa_cols2_top = -1;        // the costliest shared edges of a call whose members take 2 columns per lane (twice the members, a shorter row): how many (-1: 4 in a few-edge call, else none)
    int poa_node_est_pct = 100, poa_far_rows = -1;
    int poa_far_shift = 3;         // rings of 4 kept rows (the many-edge regime): rows of H (rows read back from HBM) per edge = nodes >> this, + 256; an edge that needs more is redone with 4 x the room
    int poa_wave_max = 512, poa_cols = -1, poa_ring_kb = -1, poa_ring_zero = 0;
    int poa_balance = 1, poa_balance_pct = 125, poa_balance_lanes = 512;
    int poa_slots_pct = 100, poa_slots = 0, poa_batches = 0, poa_force_cm = 0, poa_streams = 8, poa_wide_delay_us = 60;
    int poa_prune = -1;            // exact score-bound pruning of the DP: -1 automatic (calls of thousands of edges), 0 never, else the threshold's percentage of the previous alignment's score per base
    int poa_pass_lanes = -1;       // column passes: unshared multi-wave edges run in workgroups of this many lanes, their DP columns in windows taken one after the other (-1 automatic: by
                                   // estimated chain length, where the rows are pruned; 0 never)
    int poa_own_bucket_first = 1;  // a persistent workgroup takes the edges of its OWN need bucket before those of the smaller buckets it can also serve (0: whichever next edge has the longest chain, as until round 6 - see k_poa)
    int poa_resident_first = 0;    // bit 0: the shared edges' launch of a many-edge call, bit 1: the wide persistent launches (512 lanes and more) - the next launch leaves when their workgroups have all begun (each adds itself to a word in host memory), not after a fixed delay. Measured at 140 Mb: the 37 workgroups of the 512-lane launch have all begun 40 us after it (the fixed delay is 60), and the one pass in five that took 550-620 ms was not about arrival at all (poa_own_bucket_first); 0 stays the default, the best pass is 0.459 against 0.480 s
    int poa_chain_pct = 70;        // the automatic chain cap: the smallest one that is at least this percentage of the call's estimated wave-slot time over the waves resident (size_edges; 60 until the persistent workgroups took their own bucket first)
    int poa_chain_ms = -1;         // ... the automatic choice: the narrowest workgroup whose estimated chain (size_edges: DP rows x what a row costs at that width and number of
                                   // windows) stays below this many milliseconds; -1: the cap that balances the longest chain against the call's wave-slot time
    int poa_prune_shared = 0;      // ... of the edges shared by several workgroups (round 6: their members take DP ATTEMPTS, not sequences, so a missed threshold is repeated by all of
                                   // them): 0 never (the default), else the percentage. Measured at 12 Mb / 4.6 Mb with 95: 65 % of the wave-rows skipped, same consensus - and the longest
                                   // chain 154 -> 207 ms / 106 -> 142 ms: in a pipeline of waves every row is live in SOME wave, which sets the pace of that row for all of them;
                                   // what a skipped wave-row frees is issue slots, and a lone chain is not short of those
    int poa_prune_lazy = 1;        // ... a wave that skipped a whole batch of rows polls for the next one rarely (0: like any wave)
    int poa_prune_lanes = 128;     // ... in launches of workgroups of at least this many lanes (a one-wave workgroup has no block to skip)
    int coords_lds_supp = -1;      // supports per edge the coordinate kernel sorts in LDS (testing: 0 sends every edge through the global scratch)
    int poa_general = 0;           // hx_poa_sequences_mode with HX_POA_NW runs the general path (kernels/poa_modes.hip) instead of the tuned one: the cross-check of what the modes share with kNW
    int poa_affine = 0;            // hx_poa_sequences_affine with gap_extend == gap_open runs the affine instances of the general path instead of the linear paths: the cross-check of the affine kernel against the linear ones
    int poa_weighted = 0;          // hx_poa_weighted without weights runs the weighted instances of the general path on weights of 1 instead of the MSA twins: the cross-check of the weighted graph update against the unit-weight one
    int poa_convex = 0;            // the convex entries with gap_extend2 <= gap_extend run the convex instances of the general path instead of the affine entries: the cross-check of the convex kernel against the affine one
    int poa_modes_slot_kb = 0;     // the general path's first round of slots holds at most this many KB (testing: forces the overflow and the rerun in a larger slot; 0 no cap)
    int poa_strand_one_h = 1;      // hx_poa_strand: one score matrix per slot, the winning reverse complement's DP runs once more (the only route built)
    int poa_graph_aln_cap = 0;     // hx_poa_graph: a set's first share of the alignment pool holds at most this many pairs (testing: forces the rerun with the exact room; 0 no cap)
};

// The shape of the last consensus call, as poa_consensus planned and launched it: what the report (hx_poa_report.h) prints beside the phase words
struct PoaCallShape {
    std::vector<uint32_t> lmax, nseq;   // per edge: longest sequence, sequences
    std::vector<uint8_t> cls;           // per edge: launch class (direction bytes 0-4, score matrix 5-9; 11 = not launched)
    std::vector<uint32_t> shape;        // per edge: lanes of its workgroup | column passes << 16 | members << 24
    uint32_t ring[11] = {};             // per launch class: kept rows of its LDS ring
    PoaReportView view(std::vector<unsigned long long>& words, int debug, int prof, FILE* out) const {
        return PoaReportView{words.data(), words.size() / hxk::POA_PHASE_WORDS, lmax.data(), nseq.data(), cls.data(), shape.data(), std::min(cls.size(), shape.size()), ring, debug, prof, out};
    }
};

}  // namespace hxi

struct hx_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    // resident inputs
    uint32_t n_contigs = 0, n_reads = 0;
    uint64_t n_hits = 0, n_ops = 0;
    hxi::DV<double> km;
    hxi::DV<uint32_t> clen;
    hxi::DV<uint8_t> cls;
    hxi::DV<uint32_t> rlen;
    hxi::DV<uint64_t> roff;
    hxi::DV<uint8_t> packed;
    hxi::HitCols hits;
    hxi::DV<uint64_t> rho;
    std::vector<uint32_t> h_rlen;
    std::vector<uint64_t> h_rho;
    uint32_t lr_begin = 0, lr_end = 0;
    bool prefiltered = false;   // the resident records are the filtered set of an index.longread
    hxi::DV<uint32_t> err;
    // chain results
    struct { hxi::ChainCols col; hxi::DV<uint32_t> cmp_aln; hxi::DV<uint64_t> aln_off, cmp_off; uint64_t n_aln = 0, n_cmp = 0; } chain;
    bool have_chain = false;
    // edge records
    hxi::RecBuf rec_un, rec;   // unsorted (emission order) and sorted
    uint64_t n_rec_un = 0, n_rec = 0, n_edge = 0;
    hxi::DV<uint64_t> edge_key, edge_off;
    std::vector<uint64_t> h_edge_key, h_edge_off;
    bool have_edges = false;
    // coords results
    hxi::CoordCols coords;
    bool have_coords = false;
    hxi::PoaCallShape poa_shape;
    bool poa_no_dir = false;   // diagnostics: force the score-matrix traceback
    int poa_block = 0;   // 0 = automatic (lanes per edge chosen from the gap length)
    hipStream_t poa_streams[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    uint32_t* poa_started = nullptr;    // 16 words of mapped host memory: workgroups that have begun, per launch of a batch (kernels/poa.hip k_poa)
    hipEvent_t poa_ev[9] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    hxi::Timer tm;
    // scratch of the chain / edge / coordinate operators lives as long as the context too (grows, never shrinks): no allocation, free or
    // synchronisation for temporaries in a call once the sizes have been seen
    hxk::Workspace ws;
    struct { hxi::ChainCols raw; hxi::DV<uint32_t> dp, cmp, naln, ncmp; hxi::DV<int32_t> from; } sc_chain;   // at raw-hit size; per read: naln, ncmp
    struct { hxi::DV<uint32_t> npairs, perm, perm_tmp, flag; hxi::DV<uint64_t> pair_off, key_tmp, fscan; } sc_edges;
    struct {   // per selected edge (ns; cap and out_off: + 1) and per record of the selected edges, doubled for hairpins (nc)
        hxi::DV<uint32_t> sel, nsupp, t_lr, t_sp, t_ep, best_list; hxi::DV<uint64_t> cap, out_off, b1, e1, b2, e2; hxi::DV<uint8_t> cur;
        hipError_t reserve(size_t ns, size_t nc) {
            hipError_t e;
            if ((e = sel.reserve(ns)) || (e = nsupp.reserve(ns)) || (e = cap.reserve(ns + 1)) || (e = out_off.reserve(ns + 1)) || (e = t_lr.reserve(nc)) || (e = t_sp.reserve(nc)) ||
                (e = t_ep.reserve(nc)) || (e = best_list.reserve(nc)) || (e = b1.reserve(nc)) || (e = e1.reserve(nc)) || (e = b2.reserve(nc)) || (e = e2.reserve(nc))) return e;
            return cur.reserve(nc);
        }
    } sc_coords;
    // POA workspace lives as long as the context: allocating tens of GB per call costs more than the kernel
    hxi::PoaPoolBufs poa_pools;
    hxi::PoaArena poa_arena;
    hxk::PoaModesWs poa_modes_ws;       // workspace of the general path (hx_poa_sequences_mode: kSW / kOV, and kNW under option poa_general; hx_poa_sequences_affine)
    std::mutex poa_arena_mu;            // hx_poa_reserve may run on a thread of its own beside the upload and the first stages
    double poa_host_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // host wall time of the last consensus call: plan, workspace, enqueue, device wait, collect, finish, (unused), total
    uint64_t poa_retry[6] = {0, 0, 0, 0, 0, 0};         // edges the last consensus call ran again, per reason: far rows, in-degree, graph overflow, wide rows, sinks, stalled
    uint64_t poa_budget = 0;
    hxi::DV<hxk::PoaEdge> poa_edges;
    hxi::DV<hxk::PoaSeq> poa_seqs;
    hxi::DV<uint32_t> poa_order, poa_len, poa_status, poa_counters, poa_btab;
    hxi::DV<hxk::PoaSlot> poa_slots;
    uint64_t poa_workspace_bytes = 0;   // largest POA workspace (pools) a call of this context has used
    uint64_t poa_last_workspace_bytes = 0, poa_free_at_first_call = 0;   // ... the last call's; free device memory when the budget was taken
    hxi::HxOptions opt;
    hxi::DV<uint32_t> poa_gather;            // collection: (source offset lo / hi, destination offset lo / hi, length) of every finished edge's consensus
    hxi::DV<char> poa_cns_dense;             // ... the strings side by side, as they are downloaded
    hxi::DV<unsigned long long> poa_phase_d, poa_cells_d;
    std::vector<unsigned long long> poa_phase;   // per edge POA_PHASE_WORDS diagnostic words of the last consensus call (kernels/poa_phase_words.h)

    DevHits hits_view() const { return hits.view(n_hits); }
    hxk::ChainFinal chain_view() const { hxk::ChainFinal v{}; chain.col.fill(v); v.cmp_aln = chain.cmp_aln.p; return v; }
    void tick() { (void)hipEventRecord(tm.a, stream); }
    void tock(int k) {
        (void)hipEventRecord(tm.b, stream);
        (void)hipEventSynchronize(tm.b);
        float ms = 0;
        (void)hipEventElapsedTime(&ms, tm.a, tm.b);
        tm.ms[k] += ms; tm.launches[k]++;
    }
};
