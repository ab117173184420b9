// hx_poa_plan.h - the planner of a POA consensus call: sub-sequences, per-edge capacities, launch classes, workspace slots and batches
// against the memory budget, and the layout of every batch (what its launch uploads and is given). Pure host heuristics: no HIP runtime call, no context - the context's two settings it reads come in as values.
#pragma once
#include "hx_internal.h"

namespace hxi {

struct PoaPlan {
    std::vector<hxk::PoaSeq> seqs;
    std::vector<hxk::PoaEdge> edges;
    std::vector<uint64_t> sumL;
    std::vector<uint32_t> nseq;
};

// what the POA stage reads: the supports of every edge (the cns_supp lists of Assemble.cpp:503-543) and the read set they point into
struct PoaInput {
    uint32_t n_edge;
    const uint64_t* supp_off;
    const uint32_t *supp_lr, *spos, *epos;
    const uint32_t* h_rlen;       // host copy of the read lengths
    const uint8_t* d_packed;      // device: 2-bit reads, their byte offsets and lengths
    const uint64_t* d_roff;
    const uint32_t* d_rlen;
};

struct Need { uint64_t nn = 0, ec = 0, hc = 0, dc = 0, wc = 0, lm = 0, st = 0, al = 0, mb = 0; };
inline void need_max(Need& a, const Need& b) {
    a.nn = std::max(a.nn, b.nn); a.ec = std::max(a.ec, b.ec); a.hc = std::max(a.hc, b.hc); a.dc = std::max(a.dc, b.dc); a.wc = std::max(a.wc, b.wc);
    a.lm = std::max(a.lm, b.lm); a.st = std::max(a.st, b.st); a.al = std::max(a.al, b.al); a.mb = std::max(a.mb, b.mb);
}
// bytes of a slot. The figures are the pool table's (hx_poa_pools.h), but for the node's: the slot counts under a binding budget depend on them,
// so 106 stays. (The slack: the per-node pools sum to 104 bytes - two bytes a node counted that no pool takes, an over-estimate.)
inline uint64_t need_bytes(const Need& n) { return n.nn * 106 + n.ec * 28 + n.hc * 4 + n.dc + n.wc + n.lm + n.st * 4 + n.al * 8 + n.mb * 8; }
static_assert(poa_pool_bytes_per(PoaPoolTotal::no) <= 106 && poa_pool_bytes_per(PoaPoolTotal::eo) == 28, "need_bytes: a node or a graph edge costs more than the pools' list says");
static_assert(poa_pool_bytes_per(PoaPoolTotal::ho) == 4 && poa_pool_bytes_per(PoaPoolTotal::dro) == 1 && poa_pool_bytes_per(PoaPoolTotal::wo) == 1 && poa_pool_bytes_per(PoaPoolTotal::so) == 1 &&
              poa_pool_bytes_per(PoaPoolTotal::sto) == 4 && poa_pool_bytes_per(PoaPoolTotal::ao) == 8 && poa_pool_bytes_per(PoaPoolTotal::clo) == 8 && poa_pool_bytes_per(PoaPoolTotal::co) == 1,
              "need_bytes: the other figures are the pools' list's");

// launch classes: (shared?, lanes per workgroup, columns per lane, traceback flavour) - one kernel instance each, so that every
// launch runs with the registers ITS row loop needs (kernels/poa.hip)
struct Cls {
    bool shared; uint32_t nt, cm; bool dir;
    uint32_t dpl = 0;   // lanes in the DP when the workgroups are wider (wide cluster members), else 0
    uint32_t pb = 0;    // unshared edges of a call with column passes: bucket of their workspace need (log2 of the megabytes) - one slot size per bucket, all buckets of a kernel instance in ONE launch
    bool pk = false;    // ... the pruned instance whatever the lanes (edges that take their columns in several passes are among the class's)
    std::vector<uint32_t> edges;
    size_t blocks = 0, order_at = 0, slot_at = 0, n_slots = 0;
    Need need{};
    bool persistent = false;
    double share = 0;   // of the batch's wave-slot time: DP rows x lanes reserved
};

constexpr int NCLS = 11;
constexpr uint64_t kPoaLdsMax = 140 * 1024;   // dynamic LDS of a POA workgroup at most (160 KB per CU less the 1024-lane kernel's static 16.5 KB: sink lists, wave mailboxes)
const int kClassNT[NCLS] = {0, 1024, 512, 256, 128, 64, 1024, 512, 256, 128, 64};
constexpr size_t kManyEdges = 3000;

// One launch of a batch as the layout leaves it: everything but the addresses. Persistent classes that differ only in their need bucket
// (build_classes) leave in ONE launch.
struct PoaLaunchRec {
    int stream = 0;                  // index of the stream / event of the launch (launches that share a stream run one after the other)
    uint32_t R = 0;                  // kept rows of the LDS ring
    uint64_t lds_bytes = 0;          // dynamic LDS of a workgroup
    int code = 0;                    // shape-class code of the launch's edges (PoaCallShape::cls, ::ring)
    size_t shapes_end = 0;           // one past the launch's last entry of BatchLayout::shapes (its first: where the launch before ends)
    hxk::PoaLaunch L{};              // every scalar field filled, every pointer null (launch_batch copies it whole and sets the pointers)
    bool persistent = false;         // (else: no counter, no btab, slots from 0)
    size_t order_at = 0, slot_at = 0, counter_at = 0, btab_at = 0;   // what the pointers order / slots / counter / btab get added
    int started_at = -1;             // index of the launch's `started` word, -1: none
    enum Wait { kNoWait, kWaitStarted, kWaitDelay } wait = kNoWait;   // the head start after it: until its workgroups have all begun (or 2 ms), or option poa_wide_delay_us
};

// Everything the launch of a batch computes before and between its HIP calls (PoaPlanner::layout_slots, ::layout_order, ::layout_launches). The edges' slot / cns_off / cl_off
// are written into PoaPlan::edges.
struct BatchLayout {
    std::vector<Cls> classes;                    // after build_classes and arrange, with slot_at / order_at / blocks
    std::vector<hxk::PoaSlot> h_slots;
    PoaPoolTotals tot;                           // of the pools
    uint64_t bytes = 0;                          // workspace of the batch as the budget counts it (total_bytes)
    PoaPoolOffsets off; size_t at = 0;           // the pools in the arena, its size
    std::vector<uint32_t> order_all;             // shared launches: one entry per workgroup (edge | member << 24, 0x00ffffff: a hole); persistent launches: the class's edges, costliest first
    std::vector<uint32_t> h_btab;                // per launch group of persistent classes: {buckets | own-bucket-first << 16, slot_end[], item_begin[], est[]} (kernels/kernels.h PoaLaunch)
    std::vector<std::array<size_t, 3>> groups;   // first class, one past the last, offset of the group's table in h_btab
    std::vector<PoaLaunchRec> launches;          // one per group, in launch order
    std::vector<std::array<uint32_t, 3>> shapes; // edge, class code, lanes | passes << 16 | members << 24 (PoaCallShape), in launch order
};

// The plan of one consensus call, and the per-edge retry state that the collection of every batch updates (hx_poa.hip: PoaCall).
struct PoaPlanner {
    const PoaInput& in;
    const hx_poa_params* pp;
    const HxOptions& o;
    const uint32_t ne;
    const int poa_block;       // the context's block size (hx_set_poa_block: 0 = automatic)
    const bool poa_no_dir;     // the context forces the score-matrix traceback (hx_set_poa_traceback)
    PoaPlan P;
    uint64_t seq_bases = 0, n_aligned = 0, budget = 0;
    std::vector<uint8_t> grow;         // times an edge's graph outgrew its workspace: the node estimate doubles each time
    std::vector<uint8_t> force_nodir;  // edges whose in-degrees outgrew the direction bytes
    std::vector<uint8_t> full_h;       // edges that run with the score-matrix traceback
    std::vector<uint8_t> wide_grow;    // times an edge had more rows with over 4 predecessors than its wide-row pool: the estimate quadruples each time
    std::vector<uint8_t> no_share;     // edges whose members did not get through together: one workgroup from now on
    std::vector<uint8_t> many_sinks;   // edges with more sink rows than the smaller kernels keep in LDS: one 1024-lane workgroup
    std::vector<uint8_t> far_full;     // times an edge's far rows outgrew the estimate: four times the room each time
    std::vector<uint8_t> ecols;        // shared edges: columns per lane their members aim at (cl_cols, or 2 for the costliest: option poa_cols2_top)
    std::vector<uint32_t> mlanes;      // shared edges: lanes per member (the option's, or 1024 where the gap needs them to fit at all)
    // knobs of this round (the option, or what the number of edges in the call asks for)
    bool many_edges = false, balanced = false;
    uint32_t cl_lanes = 256, cl_min = 2048, cl_max = 16, cl_pref = 16, cl_topk = 192, wide_k = 0, cl_cols = 4, cols_per_lane = 4, wave_max = 512, prune_pct = 0, prune_shared_pct = 0, pass_lanes = 0;
    bool pass_on = false;
    std::vector<uint16_t> plane;       // unshared edges with column passes: lanes of their workgroup
    std::vector<uint8_t> batch_by_work; // per batch of the current plan: the slot policy plan_batches settled on
    std::vector<float> chain_ms;       // estimated duration of the edge's chain (size_edges): the order of the launch lists
    uint64_t ring_kb_wave = 0;
    double balance_f = 1.25;
    uint32_t balance_nt = 512;
    mutable bool by_work = false;      // slots of the need buckets in proportion to their work (arrange): chosen per batch by plan_batches - where the memory budget binds
    uint64_t score_abs_max = 8;        // largest |match|, |mismatch|, |gap| of the call: |score| <= that x (nodes + columns) must fit the keys

    PoaPlanner(const PoaInput& in_, const hx_poa_params* pp_, const HxOptions& o_, int poa_block_, bool poa_no_dir_)
        : in(in_), pp(pp_), o(o_), ne(in_.n_edge), poa_block(poa_block_), poa_no_dir(poa_no_dir_) {}

    int plan_input(std::vector<uint32_t>& todo);
    int knobs(size_t n_todo);
    int class_of(uint32_t e) const;
    uint32_t lanes_of(uint32_t e) const { return P.edges[e].members > 1 ? mlanes[e] : (uint32_t)kClassNT[class_of(e)]; }   // lanes of the edge's workgroup(s)
    static uint32_t cm_round(uint32_t ncol, uint32_t lanes, uint32_t r = 4) { const uint32_t cm = (ncol + lanes - 1) / lanes; while (r < cm) r <<= 1; return r; }   // (r: the narrowest instance that exists for the launch)
    uint32_t ring_rows_of(uint32_t nt, uint32_t cm, uint64_t& row_bytes) const;
    // DP work of an edge ~ sum over its sequences of (nodes so far) x (length): with nodes growing linearly that is about half of
    // (final nodes) x (longest sequence) x (sequences). vcap < 2^21, lmax < 2^20, nseq < 2^24: no overflow
    uint64_t edge_cost(uint32_t e) const { return (uint64_t)P.edges[e].vcap * P.edges[e].lmax * std::max<uint32_t>(1, P.nseq[e]); }
    // DP rows of an edge's serial chain ~ the nodes of its graph before each sequence, summed (the model of the column passes: measured / model 1.10 .. 1.23). A call of
    // hundreds of edges ends when its last CHAIN ends, and a chain's duration goes with its rows, not with its cells: the order of the launch lists in such a call.
    double chain_rows(uint32_t e) const { const double S = std::max<uint32_t>(1, P.nseq[e]); return (double)P.edges[e].lmax * (S - 1.0) * (1.0 + 0.0275 * S) + (double)P.edges[e].lmax; }
    int size_edges(std::vector<uint32_t>& todo);
    Need need_of(uint32_t e) const;
    int build_classes(const std::vector<uint32_t>& batch, std::vector<Cls>& classes) const;
    size_t slots_wanted(const Cls& q, uint32_t shrink, size_t cu_reserved) const;
    void arrange(std::vector<Cls>& classes, uint32_t shrink) const;
    static bool same_instance(const Cls& a, const Cls& b) { return a.persistent && b.persistent && a.nt == b.nt && a.cm == b.cm && a.dir == b.dir && a.dpl == b.dpl && a.pk == b.pk; }
    Need slot_need(const Cls& q, size_t b) const { return q.persistent ? q.need : need_of(q.edges[b]); }   // per slot: the edge's own need, or (persistent) the largest of the class
    // what an edge takes beside its slot: the consensus output and, shared, the cluster mailboxes (words of 8 bytes)
    uint64_t cluster_words(uint32_t e) const { return (uint64_t)P.edges[e].members * ((uint64_t)P.edges[e].vcap + 1); }
    uint64_t edge_out_bytes(uint32_t e, bool shared) const { return P.edges[e].vcap + (shared ? cluster_words(e) * 8 : 0); }
    uint64_t total_bytes(std::vector<Cls>& classes, uint32_t shrink) const;
    // plan, part 5: the layout of a batch (no HIP call, no context, no clock), in the three steps its launch takes, in this order, each where that
    // arithmetic has always stood among the HIP calls
    int layout_slots(const std::vector<uint32_t>& batch, uint32_t shrink, BatchLayout& Y);   // classes, slots, pools
    void layout_order(BatchLayout& Y) const;                                                  // the order list (and the classes' blocks)
    void layout_launches(BatchLayout& Y) const;                                               // groups and tables, launches, shape entries
    int plan_batches(const std::vector<uint32_t>& todo, std::vector<std::vector<uint32_t>>& batches, std::vector<uint32_t>& batch_shrink);
    bool launch_pruned(const Cls& q) const;
};

}  // namespace hxi
