// poa_layout_text.h - what tests/poa_layout_driver.cpp and the harness that printed tests/golden/poa_layout/ share: the synthetic inputs of
// every case, and the text of a batch's layout. The text is printed from plain arrays - what a launch uploads and what a kernel is given -
// so that it can be printed from either side of the runtime ("The batch layout is a pure host step").
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <string>
#include <vector>
#include "hx_poa_plan.h"

namespace poa_layout {

// ---- inputs: every sequence is the head of a read of its own, forward
struct Input {
    std::vector<uint64_t> supp_off{0};
    std::vector<uint32_t> supp_lr, spos, epos, rlen;
    uint64_t rng;
    explicit Input(uint64_t seed) : rng(seed * 0x9e3779b97f4a7c15ull + 1) {}
    uint32_t rnd(uint32_t n) { rng = rng * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)((rng >> 33) % n); }
    void edge(uint32_t gap, uint32_t nseq) {   // the first sequence has `gap` bases, the others up to 3 % fewer
        for (uint32_t k = 0; k < nseq; k++) {
            const uint32_t len = k ? gap - rnd(gap / 32 + 1) : gap;
            supp_lr.push_back((uint32_t)rlen.size()); spos.push_back(0); epos.push_back(len - 1); rlen.push_back(len + rnd(50));
        }
        supp_off.push_back(supp_lr.size());
    }
    hxi::PoaInput view() const { return hxi::PoaInput{(uint32_t)supp_off.size() - 1, supp_off.data(), supp_lr.data(), spos.data(), epos.data(), rlen.data(), nullptr, nullptr, nullptr}; }
};

// an edge that the first round reports back with a status (case g): the second round plans it again
struct Mark { uint32_t edge; uint32_t status; };

struct Case {
    Input in{1};
    hxi::HxOptions opt;
    int poa_block = 0;
    bool poa_no_dir = false;
    std::vector<Mark> marks;
};

inline void few_edges(Input& in) {
    static const uint32_t gaps[13] = {40, 300, 511, 512, 700, 1500, 2047, 2048, 2100, 3000, 5000, 9000, 20000};
    for (uint32_t g : gaps) { in.edge(g, 3); in.edge(g, 6); }
}
inline void many_edges(Input& in, uint32_t n_small, uint32_t n_gaps, uint32_t gap_lo, uint32_t gap_hi, uint32_t gap_seqs) {
    for (uint32_t i = 0; i < n_small; i++) { const uint32_t len = 30 + in.rnd(201); in.edge(len, 3 + in.rnd(3)); }
    for (uint32_t i = 0; i < n_gaps; i++) { const uint32_t len = gap_lo + in.rnd(gap_hi - gap_lo + 1); in.edge(len, gap_seqs ? gap_seqs : 3 + in.rnd(6)); }
}

// the cases of tests/test_poa_layout.py; false: no such case
inline bool make_case(const std::string& name, Case& c) {
    if (name == "a" || name == "b" || name == "c_block" || name == "c_ring" || name == "g") {
        c.in = Input(7);
        few_edges(c.in);
        c.poa_no_dir = name == "b";
        if (name == "c_block") c.poa_block = 256;
        if (name == "c_ring") c.opt.poa_ring_zero = 1;
        // (edges 2 k and 2 k + 1: gap k of few_edges with 3 and 6 sequences) the graph of 5000 x 6 outgrew its workspace, 3000 x 6 an in-degree above the direction
        // bytes' limit, 9000 x 6 far rows, 2100 x 6 wide rows, 1500 x 6 sink rows, 20000 x 6 (shared) a member that gave up waiting
        if (name == "g") c.marks = {{21, HXE_POA_OVERFLOW}, {19, HXE_POA_NODIR}, {23, HXE_POA_FARROWS}, {17, HXE_POA_WIDEROWS}, {11, HXE_POA_SINKS}, {25, HXE_POA_STALLED}};
        return true;
    }
    if (name == "d" || name == "e") {
        c.in = Input(11);
        many_edges(c.in, 3300, 36, 600, 9000, 0);
        if (name == "e") c.opt.poa_workspace_gb = 0.4;
        return true;
    }
    if (name == "f") {
        c.in = Input(13);
        many_edges(c.in, 3300, 32 + 240, 5900, 6100, 3);   // beyond the 32 that stay shared: a 1024-lane class of more edges than its share of the chip holds (persistent) ...
        many_edges(c.in, 0, 20, 2900, 3100, 6);            // ... and a 512-lane class of fewer (one workgroup per edge: no head start)
        c.opt.poa_pass_lanes = 0; c.opt.poa_resident_first = 3;
        return true;
    }
    return false;
}
constexpr uint64_t kBudget = 64000000000ull;   // 64 GB: the budget of the cases that have no option poa_workspace_gb

// ---- text
struct Text {
    FILE* f;
    void batch(uint32_t shrink, bool by_work, uint64_t bytes, size_t at, uint64_t clo_memset, size_t n_counters) const {
        fprintf(f, "batch shrink %u by_work %d bytes %llu arena %zu mailbox_words %llu counters %zu\n", shrink, (int)by_work, (unsigned long long)bytes, at, (unsigned long long)clo_memset, n_counters);
    }
    void pool(const char* name, size_t off) const { fprintf(f, "pool %s %zu\n", name, off); }
    // the edges that `order` names, ascending: the PoaEdge table as uploaded, and the shape entries of the call's report
    void edges(const hxk::PoaEdge* E, const uint32_t* order, size_t n_order, const uint8_t* cls, const uint32_t* shape) const {
        std::vector<uint32_t> ids;
        for (size_t i = 0; i < n_order; i++) if (order[i] != 0x00ffffffu) ids.push_back(order[i] & 0x00ffffffu);
        std::sort(ids.begin(), ids.end());
        ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
        for (uint32_t e : ids)
            fprintf(f, "edge %u seq_begin %u seq_end %u vcap %u ecap %u lmax %u hrows %u cns_off %llu cl_off %llu members %u wrows %u slot %u passes %u cls %u shape 0x%08x\n", e, E[e].seq_begin, E[e].seq_end, E[e].vcap, E[e].ecap,
                    E[e].lmax, E[e].hrows, (unsigned long long)E[e].cns_off, (unsigned long long)E[e].cl_off, E[e].members, E[e].wrows, E[e].slot, E[e].passes, (unsigned)cls[e], shape[e]);
    }
    void slots(const hxk::PoaSlot* S, size_t n) const {
        for (size_t i = 0; i < n; i++)
            fprintf(f, "slot %zu node %llu edge %llu h %llu d %llu w %llu seq %llu stack %llu aln %llu mbox %llu\n", i, (unsigned long long)S[i].node_off, (unsigned long long)S[i].edge_off, (unsigned long long)S[i].h_off,
                    (unsigned long long)S[i].d_off, (unsigned long long)S[i].w_off, (unsigned long long)S[i].seq_off, (unsigned long long)S[i].stack_off, (unsigned long long)S[i].aln_off, (unsigned long long)S[i].mbox_off);
    }
    void order(const uint32_t* o, size_t n) const {
        for (size_t i = 0; i < n; i++) { if (o[i] == 0x00ffffffu) fprintf(f, "order %zu hole\n", i); else fprintf(f, "order %zu edge %u member %u\n", i, o[i] & 0x00ffffffu, o[i] >> 24); }
    }
    void btab(const uint32_t* b, size_t n) const { for (size_t i = 0; i < n; i++) fprintf(f, "btab %zu %u\n", i, b[i]); }
    // offsets: what was added to the buffers' base pointers, -1 where the pointer is null
    void launch(size_t gi, int stream, int code, uint32_t R, const hxk::PoaLaunch& L, long long order_at, long long slot_at, long long counter_at, long long btab_at, long long started_at, const char* wait) const {
        fprintf(f, "launch %zu stream %d code %d R %u n_items %u n_blocks %u match %d mismatch %d gap %d block_threads %d cm %d poll_limit %u ring_bytes %u use_dir %d max_indeg %u dp_lanes %u prune_pct 0x%x "
                   "order_at %lld slot_at %lld counter_at %lld btab_at %lld started_at %lld wait %s\n", gi, stream, code, R, L.n_items, L.n_blocks, L.match, L.mismatch, L.gap, L.block_threads, L.cm, L.poll_limit, L.ring_bytes,
                (int)L.use_dir, L.max_indeg, L.dp_lanes, L.prune_pct, order_at, slot_at, counter_at, btab_at, started_at, wait);
    }
};

}  // namespace poa_layout
