// hx_poa_plan.hip - the planner of a POA consensus call (hx_poa_plan.h): parts 1-5 of the plan and the launch-class decisions the
// launch reads back. Host code only.
#include "hx_poa_plan.h"

namespace hxi {

// ---- plan, part 1: the sub-sequence rule of Assemble.cpp:530-537 (u32 wrap + substr clamp; empty ones skipped)
int PoaPlanner::plan_input(std::vector<uint32_t>& todo) {
    P.edges.resize(ne); P.sumL.assign(ne, 0); P.nseq.assign(ne, 0);
    // (330 000 sequences of 13 000 edges at 140 Mb, a read-length lookup each: counted and filled by a few threads, each its range of the edges - 3.6 ms on one)
    const uint64_t n_supp = ne ? in.supp_off[ne] - in.supp_off[0] : 0;
    const uint32_t nt = n_supp > 50000 ? 8u : 1u;
    std::vector<uint64_t> t_seqs(nt + 1, 0), t_bases(nt, 0);
    std::atomic<int> bad{0};
    auto range = [&](uint32_t t, bool fill) {
        const uint32_t e0 = (uint32_t)((uint64_t)ne * t / nt), e1 = (uint32_t)((uint64_t)ne * (t + 1) / nt);
        uint64_t at = fill ? t_seqs[t] : 0, bases = 0;
        for (uint32_t e = e0; e < e1; e++) {
            hxk::PoaEdge& E = P.edges[e];
            if (fill) { memset(&E, 0, sizeof(E)); E.seq_begin = (uint32_t)at; }
            uint32_t cnt = 0, lmax = 0; uint64_t sum = 0;
            for (uint64_t k = in.supp_off[e]; k < in.supp_off[e + 1]; k++) {
                const uint32_t rid = in.supp_lr[k] & 0x7fffffffu, strand = in.supp_lr[k] >> 31;
                const uint32_t rl = in.h_rlen[rid], sp = in.spos[k], ep = in.epos[k];
                if (sp > rl) { bad = 1; return; }
                const uint32_t want = ep - sp + 1, n = std::min(want, rl - sp);
                if (n == 0) continue;
                if (fill) P.seqs[at] = hxk::PoaSeq{rid, strand, sp, n};
                at++; cnt++; sum += n; lmax = std::max(lmax, n);
            }
            if (fill) { E.seq_end = (uint32_t)at; E.lmax = lmax; P.sumL[e] = sum; P.nseq[e] = cnt; bases += sum; }
        }
        if (fill) t_bases[t] = bases; else t_seqs[t + 1] = at;   // (counting pass: `at` started at 0 - the range's own count)
    };
    auto all = [&](bool fill) {
        std::vector<std::thread> th;
        for (uint32_t t = 1; t < nt; t++) th.emplace_back(range, t, fill);
        range(0, fill);
        for (std::thread& x : th) x.join();
    };
    all(false);
    if (bad) return fail("hx_poa_batch: consensus support starts beyond its read (the reference would throw std::out_of_range, Assemble.cpp:530)");
    {   // the ranges' counts -> where each range's sequences begin
        uint64_t run = P.seqs.size();
        for (uint32_t t = 0; t < nt; t++) { const uint64_t n = t_seqs[t + 1]; t_seqs[t] = run; run += n; }
        t_seqs[nt] = run;
        P.seqs.resize(run);
    }
    all(true);
    for (uint32_t t = 0; t < nt; t++) seq_bases += t_bases[t];
    n_aligned += t_seqs[nt] - t_seqs[0];
    for (uint32_t e = 0; e < ne; e++) if (P.nseq[e]) todo.push_back(e);
    grow.assign(ne, 0); force_nodir.assign(ne, 0); full_h.assign(ne, 0); wide_grow.assign(ne, 0); no_share.assign(ne, 0); many_sinks.assign(ne, 0); far_full.assign(ne, 0);
    mlanes.assign(ne, 0); plane.assign(ne, 0); chain_ms.assign(ne, 0.f); ecols.assign(ne, 4);
    return 0;
}

// ---- plan, part 2: the knobs of a round. Sharing an edge buys latency for that edge and costs throughput. Hundreds of edges (the longest is the
// step): up to 16 members, the 192 costliest shared. Thousands (every CU busy anyway): 8 members (more only where a gap needs them to fit at
// all), the 32 costliest - measured on 13 262 edges: 2.10 s with 16 x 192, 1.98 s with 8 x 32, 2.29 s without sharing (the largest edges then
// run on after everything else has finished). (The two launch shapes cross between 2 200 and 3 300 edges: 292 against 313 ms at 2 214 edges,
// 390-400 against 374 ms at 3 294.)
int PoaPlanner::knobs(size_t n_todo) {
    const bool many_in = ne > kManyEdges;
    many_edges = n_todo > kManyEdges;
    cl_lanes = (uint32_t)o.poa_member_lanes; cl_min = (uint32_t)o.poa_cluster_min;
    cl_max = o.poa_cluster_max >= 0 ? (uint32_t)o.poa_cluster_max : 16;           // members per edge at most
    cl_pref = o.poa_cluster_max >= 0 ? cl_max : many_in ? 8 : 16;                 // ... unless the gap needs more to fit at all
    cl_topk = o.poa_cluster_topk >= 0 ? (uint32_t)o.poa_cluster_topk : many_in ? 32 : 192;   // shared edges per call at most (the costliest)
    wide_k = o.poa_wide_members >= 0 ? (uint32_t)o.poa_wide_members : 0;         // shared edges per call (the costliest) whose members are 1024-lane workgroups (default: size_edges)
    // columns per lane a member aims at: 4 while the longest edges set the duration; 8 in calls of thousands of edges - the 4-column instances take 145-158
    // registers, and ONE such wave on a SIMD leaves room for two waves of the 128-register instances instead of three: the 32 shared edges' 896 waves
    // held the whole chip at 3 200 resident waves of 4 096 while they ran (tools/dev_r05.sh edgedump: 3 870 with 8 columns, the call 705 -> 657 ms)
    cl_cols = o.poa_cluster_cols > 0 ? (uint32_t)o.poa_cluster_cols : many_in ? 8u : 4u;
    wave_max = (uint32_t)o.poa_wave_max;                                          // columns handled by ONE wavefront per edge
    // columns per lane of the multi-wave classes: 4 while edges are few (more lanes = a shorter row for the edges that set the step time),
    // 8 when thousands of edges keep every CU busy anyway (a row then costs fewer instructions in total: the per-row overhead is per wave).
    cols_per_lane = o.poa_cols > 0 ? (uint32_t)o.poa_cols : many_edges ? 8 : 4;
    // LDS of the kept-row ring. Few edges (their longest sets the duration): as many kept rows as fit, so that hardly any row is read back
    // from HBM. Thousands of edges (every CU busy): what counts is waves per SIMD - each wave spends most of its time waiting for its own
    // dependent instructions - so the ring is cut to `poa_ring_kb` per wave and several workgroups share a CU.
    ring_kb_wave = o.poa_ring_kb > 0 ? (uint64_t)o.poa_ring_kb : many_edges ? 11 : 0;   // 0 = no cut
    // Balanced launch for calls of thousands of edges: see build_classes / slots_wanted
    balanced = many_edges && o.poa_balance != 0;
    balance_f = std::max(10, o.poa_balance_pct) / 100.0;
    balance_nt = (uint32_t)o.poa_balance_lanes;                                   // classes of at least this many lanes per workgroup get a share
    // Exact score-bound pruning (kernels/poa.hip PRUNE) skips the (row, wave) blocks that cannot reach the alignment's score: work saved in the
    // multi-wave launches of a call whose CUs are all busy; a chain-bound call (hundreds of edges, the longest one is the step) gains nothing
    // from it - a row stays a row - so there the full-matrix instances run. poa_prune: -1 automatic, 0 never, else the percentage.
    // (round 6: automatic also in a few-edge call, for its unshared multi-wave classes and without the column passes - the step is the shared edges' and neither gains nor
    // loses, 164.98 against 165.54 ms at 12 Mb, but the dead wave-rows' nibble rows are not written)
    prune_pct = o.poa_prune < 0 ? 95u : (uint32_t)o.poa_prune;
    // The bound U = H + match x (columns left) and the lane test behind it are exact for scores of the usual signs only: gap <= 0, mismatch <= match,
    // gap <= match (hx_poa_sequences and spoa_hx.hpp take any int8 triple). Anything else runs the full-matrix instances.
    prune_shared_pct = (uint32_t)std::max(0, o.poa_prune_shared);
    if (!(pp->gap <= 0 && pp->mismatch <= pp->match && pp->gap <= pp->match && pp->match >= 0)) prune_pct = prune_shared_pct = 0;
    score_abs_max = std::max<uint64_t>({1, (uint64_t)std::abs((int)pp->match), (uint64_t)std::abs((int)pp->mismatch), (uint64_t)std::abs((int)pp->gap)});
    // Column passes (kernels/poa.hip): with the rows pruned, an edge's wave slots are mostly held by waves that skip - so the unshared multi-wave edges run
    // in workgroups of `pass_lanes` lanes and take their columns window by window. The call is bound by wave-slot time (thousands of edges, every slot
    // taken): an edge of 8 000 columns holds 4 waves instead of 16 for little more than the same time.
    pass_on = prune_pct != 0 && cols_per_lane <= 8 && o.poa_pass_lanes != 0 && (many_edges || o.poa_prune >= 0 || o.poa_pass_lanes > 0);   // (the automatic pruning of a few-edge call: without passes)
    pass_lanes = !pass_on || o.poa_pass_lanes < 0 ? 0u : (uint32_t)o.poa_pass_lanes;   // (0 with pass_on: by gap length, size_edges)
    if (pass_lanes != 0 && pass_lanes != 64 && pass_lanes != 128 && pass_lanes != 256 && pass_lanes != 512 && pass_lanes != 1024) return fail("option poa_pass_lanes must be 0, 64, 128, 256, 512 or 1024");
    if (cl_lanes != 64 && cl_lanes != 128 && cl_lanes != 256 && cl_lanes != 512 && cl_lanes != 1024) return fail("option poa_member_lanes must be 64, 128, 256, 512 or 1024");
    return 0;
}

// lanes per edge. Gaps up to 2047 bases: ONE wavefront per edge (row in registers, no barriers, many edges per CU).
// Longer gaps: a multi-wave workgroup with ~8 columns per lane (256..1024 lanes). One launch per class, classes run concurrently.
// Class 0 = edges shared by several workgroups (cluster members of cl_lanes lanes); classes 1..5 = one workgroup per edge.
// Classes 6..10 = classes 1..5 for the edges that need the score-matrix traceback (rare: an in-degree
// the direction bytes cannot hold, or the test switch), launched after their direction-byte twins on the same streams.
int PoaPlanner::class_of(uint32_t e) const {   // launch class of an edge that is not shared (members == 1), direction-byte flavour
    static const uint32_t kMaxCm[6] = {0, 8, 16, 32, 32, 32};   // columns per lane each kernel variant keeps in registers
    const uint32_t ncol = P.edges[e].lmax + 1;
    int k = 5;
    if (many_sinks[e]) return 1;   // (the 1024-lane kernel keeps the full sink list)
    if (poa_block) { for (k = 1; k < 5 && kClassNT[k] > poa_block; k++) {} }
    else if (ncol > wave_max) { k = 4; while (k > 1 && (uint64_t)kClassNT[k] * cols_per_lane < ncol) k--; }
    if (P.edges[e].passes > 1) { for (int q = 1; q <= 5; q++) if ((uint32_t)kClassNT[q] == plane[e]) return q; }   // (column passes: a narrow workgroup, whatever the gap length)
    while (k > 1 && (uint64_t)kClassNT[k] * kMaxCm[k] < ncol) k--;
    return k;
}

// kept rows the LDS ring holds; row_bytes returns the LDS bytes of the ring
uint32_t PoaPlanner::ring_rows_of(uint32_t nt, uint32_t cm, uint64_t& row_bytes) const {
    row_bytes = (uint64_t)cm * (nt / 64) * 65 * 4;   // planes of 65 words per wave
    uint64_t lds_budget = nt >= 1024 ? 128 * 1024 : nt == 64 ? 32 * 1024 : 64 * 1024 * (nt / 128 > 2 ? 2 : 1);
    if (ring_kb_wave) lds_budget = std::min<uint64_t>(lds_budget, std::max<uint64_t>(ring_kb_wave * 1024 * (nt / 64), 2 * row_bytes));
    if (2 * row_bytes > lds_budget) lds_budget = kPoaLdsMax;   // wide rows: whatever the CU has
    const uint64_t rows_fit = std::min<uint64_t>(lds_budget, kPoaLdsMax) / row_bytes;
    uint32_t R = rows_fit >= 8 ? 8 : rows_fit >= 4 ? 4 : rows_fit >= 2 ? 2 : 0;   // kept rows: a power of two (slot = kept-row counter & (R-1)); 0 = every kept row goes through HBM
    if (o.poa_ring_zero) R = 0;                                    // (testing: the ring-less mode that otherwise only gaps above 16 383 columns in ONE workgroup reach)
    row_bytes = row_bytes * std::max<uint32_t>(R, 1);              // -> LDS bytes (at least one row's worth: the kernel's other phases use the space too)
    return R;
}

// ---- plan, part 3: per-edge capacities, members, far / wide row estimates; orders `todo` costliest first
int PoaPlanner::size_edges(std::vector<uint32_t>& todo) {
    const uint64_t est_pct = (uint64_t)std::max(1, o.poa_node_est_pct);   // (testing: scales the node estimate)
    // ---- workspace sizes. Nodes of the finished graph: measured (nodes - L) / (L x sequences) on 13 %-error PacBio-like and 12 %-error
    // Nanopore-like reads is 0.05-0.06 (median), 0.07-0.08 (99th percentile, small edges). The estimate allows 0.09 plus a fifth of L
    // (a tighter one - 0.07 plus a twelfth - sent 7 of 13 230 edges of the 140 Mb data into a second attempt, which cost more than the memory was worth)
    // and doubles when a graph outgrows it, up to the proven bound (every base a node of its own).
    for (uint32_t e : todo) {
        hxk::PoaEdge& E = P.edges[e];
        if (E.lmax + 1 >= (1u << 20)) return fail("hx_poa_batch: a gap sub-sequence of " + std::to_string(E.lmax) + " bases is longer than the POA kernel's score keys hold (1 048 574)");
        const uint64_t est = std::max<uint64_t>(1, (((uint64_t)E.lmax * (120 + 9 * (uint64_t)P.nseq[e])) / 100 + 1024) * est_pct / 100) << std::min<uint32_t>(grow[e], 20);
        const uint64_t vc = std::max<uint64_t>(std::min<uint64_t>(P.sumL[e], est), E.lmax);   // (never below one sequence: per-base scratch shares the node pools)
        if (vc >= 0x7fffffffULL) return fail("hx_poa_batch: POA graph too large");
        // DP cells are keys = 64 x score + 6 tie-break bits in an int32: |score| <= 8 * (nodes + columns) must stay below 2^24
        if ((vc + E.lmax + 2) * score_abs_max >= (1ull << 24)) return fail("hx_poa_batch: POA graph of an edge exceeds 2^24 / " + std::to_string(score_abs_max) + " nodes + columns (score keys would overflow)");
        E.vcap = (uint32_t)vc; E.ecap = (uint32_t)(P.sumL[e] + P.nseq[e] + 1);
        // rows of H. The score-matrix traceback keeps every row; with direction bytes only rows that a successor reads after they left
        // the LDS ring go to HBM (about 1 row in 1000 on PacBio-like data): a sixteenth of the rows is the estimate, all of them the retry
        full_h[e] = poa_no_dir || force_nodir[e];   // (any number of sequences: the kernel reports an in-degree the direction bytes cannot hold, see max_indeg)
    }
    // (option poa_cols2_top, few-edge calls: the costliest edges that will be shared get members of 2 columns per lane - the kernel instances of the 256-lane
    // members and the 1024-lane wide members exist with 2 columns)
    for (uint32_t e : todo) ecols[e] = (uint8_t)cl_cols;
    // Measured (round 6, A/B in one GPU call): the longest 12 Mb edge's chain 159.6 -> 150 ms with 2 columns per lane (its row is ~28 instructions shorter, its
    // members twice as many); as the shape of ALL 192 shared edges the step got worse, 0.164 -> 0.195 s (twice the member waves crowd the chip: edges start
    // late); for the 4 costliest - the ones that get wide members - 0.164 -> 0.159 s (8: 0.161, 16: 0.164, 32: 0.175), 4.6 Mb 0.113 -> 0.110 s.
    const int cols2_top = o.poa_cols2_top >= 0 ? o.poa_cols2_top : (ne > kManyEdges ? 0 : 4);
    if (cols2_top > 0 && cl_lanes == 256) {
        std::vector<uint32_t> cand;
        for (uint32_t e : todo) if (P.edges[e].lmax + 1 > cl_min && !poa_block && !poa_no_dir && !force_nodir[e] && !many_sinks[e] && !no_share[e]) cand.push_back(e);
        std::sort(cand.begin(), cand.end(), [&](uint32_t a, uint32_t b) { const double ca = chain_rows(a), cb = chain_rows(b); return ca != cb ? ca > cb : a < b; });   // (the longest chains)
        for (size_t q = 0; q < cand.size() && q < (size_t)cols2_top; q++) ecols[cand[q]] = (uint8_t)(cl_cols >= 8 ? cl_cols / 2 : 2);   // (a many-edge call, whose members aim at 8 columns, when the option asks for it there: 4)
    }
    for (uint32_t e : todo) {
        hxk::PoaEdge& E = P.edges[e];
        // long gaps: the DP columns of the edge are shared by several workgroups (one CU each). Members of cl_lanes lanes x up to 32 columns per
        // lane x up to cl_max members hold 131 071 columns by default; a longer gap sub-sequence (the u32 wrap of Assemble.cpp:530 makes "the whole
        // tail of a read" a real case) gets 1024-lane members, 16 of which hold 524 287 columns.
        E.members = 1; mlanes[e] = cl_lanes;
        const uint32_t ncol = E.lmax + 1;
        const bool may_share = !poa_block && !poa_no_dir && !force_nodir[e] && !many_sinks[e] && !no_share[e];
        if (may_share && ncol > cl_min) {
            const uint64_t ecl = ecols[e], pref = ecl < cl_cols ? cl_max : cl_pref;   // (the longest chains, fewer columns per lane: as many members as that takes)
            auto members_for = [&](uint32_t lanes) -> uint64_t {
                return std::min<uint64_t>(cl_max, std::max<uint64_t>(std::min<uint64_t>(pref, (ncol + (uint64_t)lanes * ecl - 1) / ((uint64_t)lanes * ecl)), (ncol + (uint64_t)lanes * 32 - 1) / ((uint64_t)lanes * 32)));
            };
            uint64_t mb = members_for(cl_lanes);
            if (((uint64_t)ncol + mb * cl_lanes - 1) / (mb * cl_lanes) > 32 && cl_lanes < 1024) { mlanes[e] = 1024; mb = members_for(1024); }   // (the gap does not fit the configured members)
            E.members = (uint32_t)mb;
        }
        if (E.members < 2 || ((uint64_t)ncol + (uint64_t)E.members * mlanes[e] - 1) / ((uint64_t)E.members * mlanes[e]) > 32) E.members = 1;   // (members too small for this gap: one workgroup)
        E.passes = 1;
        if (E.members == 1 && ncol > 1024u * (uint32_t)hxk::poa_kernel_max_cm(1024))
            return fail("hx_poa_batch: a gap sub-sequence of " + std::to_string(ncol - 1) + " bases needs the shared (cluster) mode - direction-byte traceback, automatic block size - with " +
                        std::to_string((ncol + 1024 * 32 - 1) / (1024 * 32)) + " members of 1024 lanes (option poa_cluster_max: " + std::to_string(cl_max) + ")");
    }
    // Sharing an edge among several CUs buys latency for the edge and costs throughput (the other members idle while member 0 walks
    // back and updates the graph). It pays while large edges are few; with many of them only the costliest keep their members.
    {
        std::vector<uint32_t> sh;
        for (uint32_t e : todo) if (P.edges[e].members > 1) sh.push_back(e);
        if (sh.size() > cl_topk) {
            std::sort(sh.begin(), sh.end(), [&](uint32_t a, uint32_t b) { const uint64_t ca = edge_cost(a), cb = edge_cost(b); return ca != cb ? ca > cb : a < b; });
            for (size_t q = cl_topk; q < sh.size(); q++) if (P.edges[sh[q]].lmax + 1 <= 8192) P.edges[sh[q]].members = 1;   // (longer gaps than a 1024-lane workgroup holds with its ring stay shared)
        }
    }
    // Column passes for the multi-wave edges that run unshared (decided here, after the costliest have kept their members). With the rows pruned a call of
    // thousands of edges is bound by WAVE-SLOT TIME: a 256-lane workgroup holds four wave slots of which the live band of the matrix keeps one or two
    // busy, and all four sit through the serial phases (traceback, graph update, CSR rebuild). Measured per DP row of an edge, under the load of such a
    // call (tools/dev_r05.sh edgedump, profiles/r05_edge_model.txt): a workgroup of 64 / 128 / 256 lanes takes 1.5 / 1.4 / 1.1 us with one window, 2.6 /
    // 1.9 / 1.4 us with two, 3.3 / 2.5 / 1.9 us with four - the narrowest workgroup is always the cheapest in wave-slot time (1.6 against 2.7 against 4.5
    // slot-us per row) and always the longest chain. So every edge gets the NARROWEST workgroup whose estimated chain stays below a cap, and the cap
    // is the one that balances the longest chain against the call's wave-slot time over the chip's slots (list scheduling: costliest first).
    if (pass_on) {
        // cycles per DP row at 2.4 GHz: the DP with 1 .. 4 windows (then per further window), everything else of the chain
        static const uint32_t kLanes[5] = {64, 128, 256, 512, 1024};
        // (the first dump's figures, 3 200 waves resident: they rank the widths as the final build's do - whose own table, taken where the long chains had been
        // given the wide workgroups, puts 128 lanes above 64 and moved the choices to 256 lanes: 0.58-0.68 s against 0.55 s - and overestimate its chains by a third)
        static const double kDp[5][4] = {{1470, 2900, 3800, 4435}, {1862, 2685, 3273, 3797}, {1741, 2430, 2900, 3150}, {1900, 2000, 2300, 2600}, {1850, 2000, 2200, 2400}};
        static const double kDpMore[5] = {500, 450, 250, 250, 200}, kRest[5] = {3300, 1900, 1000, 930, 900};
        struct Opt { double ms[5]; uint32_t np[5]; int first, last; };
        std::vector<uint32_t> ord;
        std::vector<Opt> opts;
        double fixed_slot_ms = 0;   // wave-slot time of the edges that have no choice (shared edges, one-wave gaps, score-matrix retries)
        for (uint32_t e : todo) {
            const hxk::PoaEdge& E = P.edges[e];
            const uint32_t ncol = E.lmax + 1, S = std::max<uint32_t>(1, P.nseq[e]);
            const double rows = 1.18 * (double)E.lmax * (double)(S - 1) * (1.0 + 0.0275 * S);   // nodes of the graph before each sequence, summed (measured / model: 1.10 .. 1.23)
            if (E.members > 1) { chain_ms[e] = (float)(rows * (1000 + 1000) / 2.4e6); fixed_slot_ms += chain_ms[e] * E.members * (mlanes[e] / 64); continue; }
            if (ncol <= wave_max || poa_block || full_h[e] || many_sinks[e]) { chain_ms[e] = (float)(rows * (1470 + 2200) / 2.4e6); fixed_slot_ms += chain_ms[e]; continue; }
            Opt q{}; q.first = -1; q.last = -1;
            for (int k = 0; k < 5; k++) {
                const uint64_t win = (uint64_t)kLanes[k] * cols_per_lane;
                const uint32_t np = (uint32_t)((ncol + win - 1) / win);
                if (np > 64 || (pass_lanes && kLanes[k] != pass_lanes && np > 1)) continue;        // (option poa_pass_lanes: that width or the one that holds the gap)
                q.np[k] = np; q.ms[k] = rows * ((np <= 4 ? kDp[k][np - 1] : kDp[k][3] + kDpMore[k] * (np - 4)) + kRest[k]) / 2.4e6;
                if (q.first < 0) q.first = k;
                q.last = k;
                if (np == 1) break;                                                                // (wider than the gap: 4 columns per lane - not this model's)
            }
            if (q.first < 0) { chain_ms[e] = (float)(rows * 3000 / 2.4e6); continue; }
            ord.push_back(e); opts.push_back(q);
        }
        auto pick = [&](const Opt& q, double cap) { int k = q.first; while (k < q.last && (q.np[k] == 0 || q.ms[k] > cap)) k++; while (q.np[k] == 0) k--; return k; };
        double cap = o.poa_chain_ms > 0 ? (double)o.poa_chain_ms : 0;
        if (cap == 0) {
            // the smallest cap that is at least 0.65 of what the call then takes - its wave-slot time over the ~3 800 waves resident. (0.55 until the dead rows of
            // a window left in runs: the chains of the narrow workgroups - many windows, most of them dead - got shorter than this table says, and the sweep
            // moved: caps of 283 (= 0.55) / 310 / 330 / 360 / 400 / 450 ms -> 0.543-0.564 / 0.517-0.565 / 0.530-0.536 / 0.542-0.568 / 0.577 / 0.612 s. Before: measured on the 140 Mb
            // data, 13 197 edges: caps of 220 / 300 / 350 / 400 ms -> 0.78 / 0.74 / 0.71 / 0.80 s before the graph phases were rebuilt, 300 -> 0.55 s
            // after; below the balance the wide workgroups cost slots, above it the call waits for its last chains.)
            cap = 3200;
            for (double cq = 100; cq <= 3200; cq *= 1.0905) {   // (an eighth of an octave apart)
                double slot = fixed_slot_ms;
                for (const Opt& q : opts) { const int k = pick(q, cq); slot += q.ms[k] * (kLanes[k] / 64); }
                // (round 6, once the persistent workgroups took their own bucket first - the slow passes of the earlier sweeps were that, not the cap: 60 / 70 / 80 / 90 / 100 %
                // = caps of 308 / 366 / 399 / 435 / 475 ms at 140 Mb: 0.461 / 0.434 / 0.426 / 0.426 / 0.438 s, five passes each; at 400 Mb, 40 / 50 / 60 / 70 / 80 / 100 % =
                // 872 / 1037 / 1234 / 1467 / 1744 / 2074 ms: 1.84 / 1.81 / 1.77 / 1.76 / 1.89-2.26 / 2.10 s. 70: profiles/r06_chain_cap_sweep.txt)
                if (o.debug > 1) fprintf(stderr, "[hx] chain cap %.0f ms: wave-slot time over 3 800 waves %.0f ms\n", cq, slot / 3800.0);
                if (cq >= std::max(10, o.poa_chain_pct) / 100.0 * slot / 3800.0) { cap = cq; break; }   // (round 6, same data, caps of 260 / 290 / 315 / 336 = 0.65 / 340 / 370 ms: 0.597 / 0.480 / 0.476 / 0.496-0.509 / 0.493 / 0.508 s)
            }
        }
        size_t hist[5] = {};
        for (size_t i = 0; i < ord.size(); i++) {
            const int k = pick(opts[i], cap);
            hist[k]++;
            chain_ms[ord[i]] = (float)opts[i].ms[k];
            if (opts[i].np[k] > 1) { P.edges[ord[i]].passes = opts[i].np[k]; plane[ord[i]] = (uint16_t)kLanes[k]; }
        }
        if (o.debug) fprintf(stderr, "[hx] column passes: chain cap %.0f ms; %zu / %zu / %zu / %zu / %zu unshared multi-wave edges in workgroups of 64 / 128 / 256 / 512 / 1024 lanes\n", cap, hist[0], hist[1], hist[2], hist[3], hist[4]);
    }
    // Wide members (build_classes) pay when ONE edge's serial chain is what the call waits for, and cost when the chip is busy anyway (every wide
    // workgroup has a CU to itself): time of the longest chain ~ its DP rows (nodes x sequences) x ~1 750 cycles, time of everything ~ DP cells
    // / throughput. Measured (Nanopore-like 25x): 4.6 Mb / 12 Mb genomes (423 / 1 079 edges) 0.190 -> 0.177 s and 0.248 -> 0.230 s with them, but 20 Mb
    // (1 864 edges, a chain 1.75 x longer) 0.426 -> 0.454 s and 30 Mb (2 737 edges) 0.327 -> 0.351 s: from ~1 500 edges on the chip is busy whatever the
    // longest chain does, so the edge count decides and the chain / work ratio only keeps calls without a dominant edge out.
    if (o.poa_wide_members < 0) {
        uint64_t top_rows = 0, sum_cost = 0;
        for (uint32_t e : todo) { top_rows = std::max<uint64_t>(top_rows, (uint64_t)P.edges[e].vcap * std::max<uint32_t>(1, P.nseq[e])); sum_cost += edge_cost(e); }
        wide_k = ne <= 1500 && (double)top_rows * 5e5 > (double)sum_cost ? 4 : 0;
        if (o.debug) fprintf(stderr, "[hx] wide members: longest chain %.3g node-sequences, all edges %.3g cost units -> %u\n", (double)top_rows, (double)sum_cost, wide_k);
    }
    // rows of H (see full_h above): how many rows leave the LDS ring before their last reader depends on how many the ring holds
    for (uint32_t e : todo) {
        hxk::PoaEdge& E = P.edges[e];
        const uint32_t ncol = E.lmax + 1, nt = lanes_of(e);
        uint64_t rb;
        const uint32_t cmq = cm_round(ncol, E.members > 1 ? E.members * nt : nt * std::max<uint32_t>(1, E.passes), E.members > 1 && ecols[e] < 4 ? 2u : 4u);
        const uint32_t Rp = ring_rows_of(nt, cmq, rb);
        // measured on PacBio-like data, rows read back from HBM per DP row: 0.15-0.4 % with 8 ring rows, 3-5 % with 4, 16-25 % on average
        // with 2 (single edges: up to every kept row, ~60 % of the rows). Graphs fill ~70 % of the node estimate these are fractions of.
        uint32_t est = o.poa_far_rows >= 0 ? (uint32_t)o.poa_far_rows : Rp >= 8 ? E.vcap / 32 + 256 : Rp >= 4 ? (E.vcap >> std::min(8, std::max(0, o.poa_far_shift))) + 256 : Rp >= 2 ? E.vcap / 2 + 256 : E.vcap + 1;
        E.hrows = full_h[e] || far_full[e] >= 3 ? E.vcap + 1 : (uint32_t)std::min<uint64_t>((uint64_t)E.vcap + 1, far_full[e] ? (uint64_t)std::max<uint32_t>(est, 256) << (2 * far_full[e]) : est);   // (a fourth attempt gets a row per node)
        // rows with more than 4 predecessors (a move byte per cell instead of a nibble): 1-2 % of the rows the DPs of 25- to 45-fold edges run
        // over, up to ~10 % of a finished deep graph; a 16th of the node estimate (graphs fill about a third of it) is the room, four times
        // more after every overflow
        E.wrows = wide_grow[e] >= 3 ? E.vcap + 1 : (uint32_t)std::min<uint64_t>((uint64_t)E.vcap + 1, ((uint64_t)E.vcap / 16 + 64) << (2 * wide_grow[e]));
    }
    // largest first (block scheduling is in grid order): cost ~ rows x columns x sequences; with column passes: the longest estimated chain first
    if (pass_on) std::sort(todo.begin(), todo.end(), [&](uint32_t a, uint32_t b) { return chain_ms[a] != chain_ms[b] ? chain_ms[a] > chain_ms[b] : a < b; });
    // (round 6, few-edge calls: by the rows of the chain, not by the cells. Per-edge timeline of the 12 Mb call, HX_DEBUG=2: with the longest chain at 150 ms the call
    // ended at 156 ms - with an edge of 2 088 columns x 21 reads that BEGAN at 109 ms and one of 2 470 x 25, 71 ms of chain, that began at 66 ms: in cell order
    // they stood behind wide gaps aligned by a few reads, whose chains are short)
    else if (!many_edges) std::sort(todo.begin(), todo.end(), [&](uint32_t a, uint32_t b) { const double ca = chain_rows(a), cb = chain_rows(b); return ca != cb ? ca > cb : a < b; });
    else std::sort(todo.begin(), todo.end(), [&](uint32_t a, uint32_t b) { const uint64_t ca = edge_cost(a), cb = edge_cost(b); return ca != cb ? ca > cb : a < b; });
    return 0;
}

// ---- workspace. An edge that is shared by several workgroups owns a workspace slot for the call; every other launch class is PERSISTENT:
// a number of slots, each sized for the class's largest edge, each owned by one workgroup that pulls edges (costliest first) from the class's
// list (kernels/poa.hip). The workspace of a call is slots x largest edge, not the sum over its edges: 140 Mb on one GPU took 241 GB per
// edge, a 400 Mb genome three batches. When even that does not fit the budget the slot counts are halved (fewer workgroups in flight); when a
// class's slots alone do not fit, the edges are dealt to several batches in cost order as before.
Need PoaPlanner::need_of(uint32_t e) const {
    const hxk::PoaEdge& E = P.edges[e];
    const uint64_t rw = ((uint64_t)E.lmax + 1 + 31) & ~31ull;                 // rows padded to 32 columns (the widest lane chunk)
    const uint64_t waves = (uint64_t)E.members * std::max<uint32_t>(1, E.passes) * (lanes_of(e) / 64);
    const uint64_t rwh = rw + (waves > 1 ? (waves + 3) & ~3ull : 0);       // rows of H end with one word per wave of the edge's pipeline
    Need n;
    n.nn = (uint64_t)E.vcap + 1; n.ec = E.ecap; n.dc = full_h[e] ? 0 : n.nn * (rw / 2); n.hc = (uint64_t)E.hrows * rwh; n.wc = full_h[e] ? 0 : (uint64_t)E.wrows * rw;
    n.lm = E.lmax; n.st = 4 * n.nn + E.ecap; n.al = n.nn + E.lmax + 2 + 64;   // (+ 64: the traceback's guard against a walk that does not end looks once per tile)
    n.mb = E.passes > 1 ? (uint64_t)E.passes * n.nn : 0;   // the carries handed from one column pass to the next
    return n;
}

// Thousands of edges: every launch class is persistent and would, on its own, ask for the whole chip (4096 waves) - six classes oversubscribe it six
// times and the dispatcher deals the wave slots out as it pleases. A 1024-lane workgroup (16 waves: an EMPTY CU) can only be placed where nothing
// else sits, so the 1024-lane class ran on the CUs it had grabbed in the first microseconds until everything else had finished: measured at 140 Mb
// (profiles/r04_v1_fly_*), the classes ended at 920 / 1 130 / 1 440 / 1 730 / 1 900 ms - a tail of 0.8 s with the chip emptier and emptier.
// Balanced launch (option poa_balance=0 switches it off): the classes of 512- and 1024-lane workgroups get workgroups for THEIR SHARE of the call's
// wave-slot time (rows x lanes reserved: a workgroup holds its lanes whether or not a gap uses them all) x poa_balance_pct / 100, and a head start
// (poa_wide_delay_us) so that they are resident before the small workgroups fragment the CUs; the small classes keep asking for the whole
// chip and fill what is left - and what a large class that ends early leaves. Order: the 1024-lane class, then the shared edges (their waves are the
// OLDEST on their SIMDs and win the issue arbitration: launched behind the 512-lane class as well, their chain - the longest of the call - took
// 3.6 times as long), then the rest by size. (Measured on the way: 91 workgroups of 1024 lanes launched BEHIND the shared edges end at 2 230 ms,
// 87 launched first at 1 540 ms - residency is the whole point.)
int PoaPlanner::build_classes(const std::vector<uint32_t>& batch, std::vector<Cls>& classes) const {
    classes.clear();
    auto cls_of = [&](bool shared, uint32_t nt, uint32_t cm, bool dir, uint32_t dpl = 0, uint32_t pb = 0, bool pk = false) -> Cls& {
        for (Cls& q : classes) if (q.shared == shared && q.nt == nt && q.cm == cm && q.dir == dir && q.dpl == dpl && q.pb == pb && q.pk == pk) return q;
        classes.push_back(Cls{shared, nt, cm, dir, dpl, pb, pk, {}});
        return classes.back();
    };
    uint32_t n_wide = 0;
    for (uint32_t e : batch) {
        const uint32_t ncol = P.edges[e].lmax + 1;
        if (P.edges[e].members > 1) {
            const uint32_t ml = mlanes[e];
            uint32_t cmr = cm_round(ncol, P.edges[e].members * ml, ecols[e] < 4 ? 2u : 4u);
            if (cmr < 4 && hxk::poa_kernel_min_cm(n_wide < wide_k && ml < 1024 ? 1024 : (int)ml, true, true) > 2) cmr = 4;
            if (cmr > (uint32_t)hxk::poa_kernel_max_cm((int)ml)) return fail("hx_poa_batch: gap too long for the configured cluster size (raise option poa_cluster_max)");
            // the costliest shared edges run with WIDE members: workgroups of 1024 lanes of which the first cl_lanes take part in the DP (one
            // wave per SIMD, as before) and all sixteen waves in the graph phases of member 0 (graph update, CSR build, orders: latency-bound
            // loops over the nodes that want lanes). Such a workgroup has a CU to itself, so only a few edges get them.
            if (n_wide < wide_k && ml < 1024 && cmr <= 8) { n_wide++; cls_of(true, 1024, cmr, true, ml).edges.push_back(e); continue; }
            cls_of(true, ml, cmr, true).edges.push_back(e);   // batch is cost-sorted, so every class list is too
            continue;
        }
        const uint32_t nt = (uint32_t)kClassNT[class_of(e)];
        uint32_t cmq = cm_round(ncol, nt * std::max<uint32_t>(1, P.edges[e].passes));
        // (calls with column passes: the gaps of up to 255 bases run in the 8-column instance too - the 4-column instances take 143-158 registers, three waves
        // per SIMD, and one such wave on a SIMD leaves room for two of the 128-register ones instead of three: CUs sat at 12 waves of their 16)
        if (pass_on && !full_h[e] && cmq < 8) cmq = 8;
        if (o.poa_force_cm > 0) cmq = std::max<uint32_t>(cmq, std::min<uint32_t>((uint32_t)o.poa_force_cm, (uint32_t)hxk::poa_kernel_max_cm((int)nt)));   // (testing: a wider kernel instance than the gap needs)
        // (calls with column passes: a class per power of two of workspace need - a persistent workgroup's slot is sized for the largest edge of its
        // class, and a narrow workgroup may now hold a gap of any length; the classes of one kernel instance leave in one launch: launch_batch)
        uint32_t pb = 0;
        // (round 6: buckets HALF an octave apart where the memory budget binds - a slot holds the largest edge of its bucket, and with buckets an octave apart a
        // quarter of the slots' memory is slack on average. Where everything fits the octave stays: 140 Mb, alternating, five passes each: best 0.473 / 0.473 s in
        // 216 GB against 0.488 / 0.501 / 0.512 s in 183 GB)
        if (pass_on && !full_h[e]) {
            const uint64_t nb_ = need_bytes(need_of(e));
            if (by_work) { const double l = std::log2((double)(nb_ >> 10) + 1.0) - 10.0; pb = l <= 0 ? 0u : (uint32_t)std::ceil(l * 2.0); }
            else { const uint64_t mb = nb_ >> 20; while ((1ull << pb) <= mb) pb++; }
        }
        cls_of(false, nt, cmq, !full_h[e], 0, pb, pass_on && !full_h[e] && cmq > 4).edges.push_back(e);   // (pk: with column passes every 8-column launch is the pruned instance - one launch per width)
    }
    // order of the launches: shared edges first (they set the duration), then by lanes; score-matrix launches after their direction-byte twins
    const bool bal = balanced, bigf = !many_edges;
    std::stable_sort(classes.begin(), classes.end(), [bal, bigf](const Cls& a, const Cls& b) {
        if (a.dir != b.dir) return a.dir;
        // (few-edge calls: the 900 member workgroups of the shared edges used to go out first and fill every CU's LDS; the 512-lane workgroups of the unshared
        // edges - chains of up to 100 ms of a 163 ms call - then began when two members on some CU had ended, 65-85 ms into the call, and most passes
        // took 182 ms instead of 163: tools/dev_r05_ab.py, 12 Mb, five passes each way)
        if (bigf) {   // wide members, then the large unshared workgroups, then the 256-lane members, then the rest
            auto grp = [](const Cls& q) { return q.shared && q.nt >= 1024 ? 0 : !q.shared && q.nt >= 512 ? 1 : q.shared ? 2 : 3; };
            if (grp(a) != grp(b)) return grp(a) < grp(b);
        }
        // (balanced launch: the 1024-lane workgroups - a whole CU each - go out before anything else sits anywhere; they share no SIMD with
        // the shared edges' members, which stay the oldest waves wherever they land)
        if (bal && (a.nt >= 1024 && !a.shared) != (b.nt >= 1024 && !b.shared)) return a.nt >= 1024 && !a.shared;
        if (a.shared != b.shared) return a.shared;
        if (a.nt != b.nt) return a.nt > b.nt;
        if (a.cm != b.cm) return a.cm > b.cm;
        if (a.pk != b.pk) return a.pk;
        return a.pb > b.pb;
    });
    double total_cost = 0;
    for (Cls& q : classes) {
        q.need = Need{};
        for (uint32_t e : q.edges) {
            need_max(q.need, need_of(e));
            q.share += (double)P.edges[e].vcap * std::max<uint32_t>(1, P.nseq[e]) * (q.shared ? (double)P.edges[e].members * mlanes[e] : (double)q.nt);   // DP rows x lanes reserved
        }
        total_cost += q.share;
    }
    for (Cls& q : classes) q.share = total_cost > 0 ? q.share / total_cost : 0;
    // The need buckets of one kernel instance share a launch, and a workgroup serves its own bucket AND every smaller one out of the slot it owns: the slot
    // must hold the largest of every component - nodes, edges, H rows, wide rows ... - over all those buckets, not only over its own. A bucket is a power of two
    // of the TOTAL bytes, and the components usually grow together; an edge that is redone with sixteen times the H rows (far rows outgrew the estimate) or a
    // larger wide-row pool is small in all and large in one - and ran, in the slot of a larger bucket, over that slot's share of the pool (round 5's fuzz: a GPU
    // memory access fault in the retries after "rows read back from HBM outgrew H"; once a consensus that differed from the oracle's).
    if (pass_on)
        for (size_t k = classes.size(); k-- > 1;) {
            Cls& a = classes[k - 1];
            const Cls& b = classes[k];
            if (!a.shared && !b.shared && a.nt == b.nt && a.cm == b.cm && a.dir == b.dir && a.dpl == b.dpl && a.pk == b.pk) need_max(a.need, b.need);
        }
    return 0;
}

// Slots of a persistent class: as many workgroups as the chip holds of that size at 16 waves per CU (all classes share the CUs, but when the
// others have finished, what is left of this one still finds the whole chip: measured at 140 Mb, 1.95 s against 2.12 s with slots in
// proportion to the classes' shares), at most one per edge. `shrink` scales the number down (memory budget).
size_t PoaPlanner::slots_wanted(const Cls& q, uint32_t shrink, size_t cu_reserved) const {
    if (q.shared) return q.edges.size();
    size_t cap = std::max<size_t>(1, ((size_t)4096 / (q.nt / 64)) * (size_t)std::max(1, o.poa_slots_pct) / 100 * shrink / 1000);   // (`shrink`: per mille of the full count)
    if (balanced && q.dir && q.nt >= balance_nt) {
        cap = std::max<size_t>(1, std::min<size_t>(cap, (size_t)((double)cap * q.share * balance_f + 0.999)));   // the class's share of the chip
        // the members of shared edges must be resident TOGETHER (a member that waits for a CU stalls its edge: HXE_POA_STALLED and an unshared
        // redo): a wide class that holds most of the call's cost would otherwise take every CU before they are placed
        if (cu_reserved && q.nt >= 1024) cap = std::max<size_t>(1, std::min<size_t>(cap, 256 > cu_reserved ? 256 - cu_reserved : 1));
        cap = std::max<size_t>(cap, std::min<size_t>(4, q.edges.size()));   // (a floor: the share is a crude model and must not starve a class down to one workgroup)
    }
    if (o.poa_slots > 0) cap = (size_t)o.poa_slots;                        // (testing: workgroups per class, many edges each)
    return std::min(q.edges.size(), cap);
}

// A class runs persistent when it has more edges than slots: its list stays in DP-cost order (costliest first, taken by whoever is free) and
// every slot is sized for the class's largest edge. (Tried: the slots' first edges = the edges with the largest workspace need, slot b sized
// for its own first edge and the largest of the rest - 148 GB instead of 257 GB at 140 Mb, but 2.32-2.42 s against 2.03-2.09 s in the same
// call: need and cost do not agree well enough - a gap aligned by 60 reads costs 20 times one aligned by 3 at the same need - and the
// costliest edges then start late. Memory is saved by halving the slot counts instead: option poa_workspace_gb.)
void PoaPlanner::arrange(std::vector<Cls>& classes, uint32_t shrink) const {
    size_t cu_reserved = 0;   // CUs the shared edges' member workgroups need (a 256-lane member: a quarter of a CU's wave slots, a wide one: a CU)
    for (const Cls& q : classes) if (q.shared) for (uint32_t e : q.edges) cu_reserved += ((size_t)P.edges[e].members * q.nt + 1023) / 1024;
    cu_reserved = std::min<size_t>(cu_reserved, 192);
    for (Cls& q : classes) {
        q.n_slots = slots_wanted(q, shrink, cu_reserved);
        q.persistent = !q.shared && (q.n_slots < q.edges.size() || pass_on) && hxk::poa_persistent_ok(q.dir);   // (pass_on: the need buckets of an instance share a launch)
        if (!q.persistent) q.n_slots = q.edges.size();
    }
    // The need buckets of one kernel instance share a launch and the chip: workgroups for 5/4 of what the chip holds of that width in all (a workgroup serves its
    // bucket and every smaller one, not the other way round; a bucket keeps a few workgroups of its own). Round 6: dealt IN PROPORTION TO THE BUCKETS' WORK (the
    // estimated chain time of their edges), not from the largest need down. Dealt top-down, the buckets of large need took a slot per edge and the memory with
    // them: a 400 Mb genome (37 936 edges, HX_DEBUG=1) ran with 1 208 slots of 137 MB for one bucket's 1 771 edges, EIGHT slots each for the 33 000 edges of
    // 37 MB and less, and 1 558 one-wave workgroups resident in all where the chip holds 4 096 - 258 GB of workspace and a chip at 40 %. With every bucket
    // finishing at about the same time, the same memory buys several times the workgroups (the top-down deal where the budget binds was removed after this measurement).
    if (pass_on)
        for (size_t i = 0; i < classes.size();) {
            size_t j = i + 1;
            while (j < classes.size() && same_instance(classes[i], classes[j])) j++;
            if (classes[i].persistent && j - i > 1 && !o.poa_slots) {
                size_t left = std::max<size_t>(1, ((size_t)4096 / (classes[i].nt / 64)) * 5 / 4 * shrink / 1000);
                if (by_work) {
                    std::vector<double> w(j - i, 0.0);
                    double w_left = 0;
                    for (size_t k = i; k < j; k++) { for (uint32_t e : classes[k].edges) w[k - i] += std::max(1e-3, (double)chain_ms[e]); w_left += w[k - i]; }
                    for (size_t k = i; k < j; k++) {
                        Cls& q = classes[k];
                        const size_t floor_k = std::min<size_t>(q.edges.size(), 8);
                        const size_t share = w_left > 0 ? (size_t)((double)left * w[k - i] / w_left + 0.999) : 0;
                        q.n_slots = std::min(q.edges.size(), std::max(floor_k, std::min(share, left)));
                        left -= std::min(left, q.n_slots);
                        w_left -= w[k - i];
                    }
                } else
                    for (size_t k = i; k < j; k++) {
                        Cls& q = classes[k];
                        q.n_slots = std::min(q.n_slots, std::max<size_t>(left, std::min<size_t>(q.edges.size(), 8)));
                        left -= std::min(left, q.n_slots);
                    }
            }
            i = j;
        }
}

uint64_t PoaPlanner::total_bytes(std::vector<Cls>& classes, uint32_t shrink) const {
    uint64_t t = 0;
    arrange(classes, shrink);
    for (Cls& q : classes) {
        for (size_t b = 0; b < q.n_slots; b++) t += need_bytes(slot_need(q, b));
        for (uint32_t e : q.edges) t += edge_out_bytes(e, q.shared);
    }
    return t;
}

// ---- plan, part 5: the layout of one batch in three steps - layout_slots: classes, slots and pools; layout_order: the order list; layout_launches: the launch
// groups with their tables, and every launch but its addresses. (Three, because the launch of a batch takes each where that arithmetic has always stood among
// its HIP calls - the device works on what is queued meanwhile, and how the uploads and launches are spaced decides in which order workgroups reach the CUs.)
int PoaPlanner::layout_slots(const std::vector<uint32_t>& batch, uint32_t shrink, BatchLayout& Y) {
    Y = BatchLayout{};
    if (ne >= (1u << 24)) return fail("hx_poa_batch: more than 2^24 edges in one call");   // (an order entry is edge | member << 24)
    std::vector<Cls>& classes = Y.classes;
    if (build_classes(batch, classes)) return -1;
    arrange(classes, shrink);
    // ---- slots and their offsets into the pools. `bytes` is total_bytes' sum: a total is the sum of its slots' needs (clo: and the cluster words), need_bytes is linear
    PoaPoolTotals& T = Y.tot;
    T.ne = ne;
    auto add_slot = [&](const Need& n) {
        Y.h_slots.push_back(hxk::PoaSlot{T.no, T.eo, T.ho, T.dro, T.wo, T.so, T.sto, T.ao, T.clo});
        T.no += n.nn; T.eo += n.ec; T.ho += n.hc; T.dro += n.dc; T.wo += n.wc; T.so += n.lm; T.sto += n.st; T.ao += n.al; T.clo += n.mb;
        Y.bytes += need_bytes(n);
    };
    for (Cls& q : classes) {
        q.slot_at = Y.h_slots.size();
        for (size_t k = 0; k < q.n_slots; k++) {
            if (!q.persistent) P.edges[q.edges[k]].slot = (uint32_t)Y.h_slots.size();   // one workgroup (or cluster) per edge: the edge's own slot
            add_slot(slot_need(q, k));
        }
        for (uint32_t e : q.edges) {
            P.edges[e].cns_off = T.co; T.co += P.edges[e].vcap;
            if (q.shared) { P.edges[e].cl_off = T.clo; T.clo += cluster_words(e); }
            Y.bytes += edge_out_bytes(e, q.shared);
        }
    }
    Y.at = Y.off.place(T);   // the pools of the batch in the arena
    return 0;
}

static size_t edges_of(const std::vector<Cls>& classes) { size_t n = 0; for (const Cls& q : classes) n += q.edges.size(); return n; }

void PoaPlanner::layout_order(BatchLayout& Y) const {
    std::vector<Cls>& classes = Y.classes;
    Y.order_all.reserve(edges_of(classes));   // (what it holds at least)
    for (Cls& q : classes) {
        q.order_at = Y.order_all.size();
        if (q.shared) {
            // Workgroups are handed to the 8 XCDs round-robin by index: put the members of one edge 8 indices apart so that they share an
            // XCD (one L2 for the carries, the handshakes and the direction bytes member 0 walks back over). Holes are no-op workgroups.
            for (size_t g0 = 0; g0 < q.edges.size(); g0 += 8) {
                const size_t g1 = std::min(q.edges.size(), g0 + 8);
                uint32_t gmax = 0;
                for (size_t j = g0; j < g1; j++) gmax = std::max(gmax, P.edges[q.edges[j]].members);
                for (uint32_t m = 0; m < gmax; m++)
                    for (size_t j = g0; j < g0 + 8; j++)
                        Y.order_all.push_back(j < g1 && m < P.edges[q.edges[j]].members ? (q.edges[j] | (m << 24)) : 0x00ffffffu);
            }
        } else
            for (uint32_t e : q.edges) Y.order_all.push_back(e);
        q.blocks = q.shared ? Y.order_all.size() - q.order_at : q.n_slots;   // (not shared: one workgroup per slot - per edge unless persistent)
    }
}

void PoaPlanner::layout_launches(BatchLayout& Y) const {
    const std::vector<Cls>& classes = Y.classes;
    const size_t n_edges = edges_of(classes);
    Y.h_btab.reserve(n_edges + 4 * classes.size()); Y.shapes.reserve(n_edges);   // (what they hold at most / exactly)
    // ---- the launch groups. Persistent classes that differ only in their need bucket (build_classes) leave in ONE launch: their slots, lists and counters
    // lie side by side in class order (largest need first), `btab` tells a workgroup which bucket its slot belongs to (kernels/poa.hip k_poa).
    for (size_t i = 0; i < classes.size();) {
        size_t j = i + 1;
        const Cls& a = classes[i];
        while (j < classes.size() && same_instance(a, classes[j])) j++;
        Y.groups.push_back({i, j, Y.h_btab.size()});
        if (a.persistent) {
            Y.h_btab.push_back((uint32_t)(j - i) | (o.poa_own_bucket_first ? 1u << 16 : 0u));
            uint32_t se = 0, ib = 0;
            for (size_t k = i; k < j; k++) { se += (uint32_t)classes[k].blocks; Y.h_btab.push_back(se); }
            for (size_t k = i; k < j; k++) { Y.h_btab.push_back(ib); ib += (uint32_t)classes[k].edges.size(); }
            Y.h_btab.push_back(ib);
            for (size_t k = i; k < j; k++) for (uint32_t e : classes[k].edges) Y.h_btab.push_back((uint32_t)std::min(4.0e9, (double)chain_ms[e] * 1000.0));   // est[]: microseconds
        }
        i = j;
    }
    // ---- the launches
    const size_t n_streams = (size_t)std::min(8, std::max(1, o.poa_streams));   // (8: a stream per launch class of a 140 Mb call - with 6, the two one-wave classes waited 130 / 300 ms behind the shared edges)
    size_t wg_total = 0;
    for (const Cls& q : classes) wg_total += q.blocks;
    Y.launches.resize(Y.groups.size());
    for (size_t gi = 0; gi < Y.groups.size(); gi++) {
        const auto& grp = Y.groups[gi];
        const size_t ci = grp[0];
        const Cls& q = classes[ci];
        size_t g_blocks = 0, g_items = 0;
        for (size_t k = grp[0]; k < grp[1]; k++) { g_blocks += classes[k].blocks; g_items += classes[k].edges.size(); }
        PoaLaunchRec& rec = Y.launches[gi];
        rec.stream = (int)(gi % n_streams);
        // LDS of the launch: the ring its row width allows, a power of two of kept rows
        uint64_t ring_need = 0;
        const uint32_t dp_nt = q.dpl ? q.dpl : q.nt;   // lanes in the DP
        rec.R = ring_rows_of(dp_nt, q.cm, ring_need);
        // few edges: ask for enough LDS per workgroup that the dispatcher cannot stack them on a handful of CUs while others idle
        // (a lone wave runs at twice the speed of two waves sharing a SIMD); many edges: request only what the ring needs
        rec.lds_bytes = ring_need;
        {
            const uint64_t per_cu = (wg_total + 255) / 256;
            if (per_cu < 8) rec.lds_bytes = std::max<uint64_t>(rec.lds_bytes, std::min<uint64_t>(kPoaLdsMax, (158 * 1024) / per_cu - 18 * 1024));
            // hundreds of edges: the longest ones set the duration, and their waves run faster with two neighbours on a SIMD than with
            // three - 10 KB of LDS per wave keeps a CU at 12 waves (thousands of edges: 16, the ring alone is 8.3 KB per wave)
            if (!many_edges) rec.lds_bytes = std::max<uint64_t>(rec.lds_bytes, std::min<uint64_t>(kPoaLdsMax, 10 * 1024 * (uint64_t)(dp_nt / 64)));
            if (o.poa_ring_zero) rec.lds_bytes = ring_need;   // (one row's worth: the kernel then finds room for no kept row either)
        }
        const int dcls = q.shared ? 0 : q.nt >= 1024 ? 1 : q.nt >= 512 ? 2 : q.nt >= 256 ? 3 : q.nt >= 128 ? 4 : 5;
        rec.code = dcls + (q.dir ? 0 : 5);
        for (size_t k = grp[0]; k < grp[1]; k++)
            for (uint32_t e : classes[k].edges) Y.shapes.push_back({e, (uint32_t)rec.code, q.nt | std::min<uint32_t>(255, P.edges[e].passes) << 16 | std::min<uint32_t>(255, P.edges[e].members) << 24});
        rec.shapes_end = Y.shapes.size();
        rec.persistent = q.persistent;
        rec.order_at = q.order_at; rec.slot_at = q.persistent ? q.slot_at : 0; rec.counter_at = ci; rec.btab_at = grp[2];
        hxk::PoaLaunch& L = rec.L;
        L.n_items = q.persistent ? (uint32_t)g_items : (uint32_t)q.blocks; L.n_blocks = (uint32_t)g_blocks;
        L.match = pp->match; L.mismatch = pp->mismatch; L.gap = pp->gap;
        L.block_threads = (int)q.nt; L.cm = (int)q.cm; L.poll_limit = (uint32_t)o.poa_poll_limit; L.ring_bytes = (uint32_t)rec.lds_bytes;
        L.use_dir = q.dir; L.max_indeg = (uint32_t)std::min(16, std::max(1, o.poa_max_indeg)); L.dp_lanes = q.dpl;
        // a 1024-lane workgroup needs an EMPTY CU: give the dispatcher a head start before the other launches fill the chip with small
        // workgroups (once they have, a CU only empties when its longest resident workgroup ends)
        const bool wide_q = q.dpl || (balanced && q.nt >= balance_nt && q.nt >= 512 && q.persistent), shared_first = many_edges && q.shared && (o.poa_resident_first & 1);
        if (((wide_q && (o.poa_resident_first & 2)) || shared_first) && gi < 16) rec.started_at = (int)gi;
        rec.wait = !(wide_q || shared_first) ? PoaLaunchRec::kNoWait : rec.started_at >= 0 ? PoaLaunchRec::kWaitStarted : PoaLaunchRec::kWaitDelay;
        L.prune_pct = launch_pruned(q) ? (std::min<uint32_t>(q.shared ? prune_shared_pct : prune_pct, 1000u) | (o.poa_prune_lazy ? 1u << 16 : 0u)) : 0u;
    }
}

// ---- plan, part 4: batches and slot counts against the budget
int PoaPlanner::plan_batches(const std::vector<uint32_t>& todo, std::vector<std::vector<uint32_t>>& batches, std::vector<uint32_t>& batch_shrink) {
    const size_t forced = o.poa_batches > 0 ? (size_t)o.poa_batches : 0;   // (testing)
    for (size_t nb = std::max<size_t>(1, forced);; nb++) {
        nb = std::min(nb, std::max<size_t>(1, todo.size()));
        batches.assign(nb, {}); batch_shrink.assign(nb, 1000); batch_by_work.assign(nb, 0);
        for (size_t i = 0; i < todo.size(); i++) batches[i % nb].push_back(todo[i]);   // dealt in cost order: every batch has its share of the large edges
        bool fits = true;
        for (size_t bi = 0; bi < nb && fits; bi++) {
            std::vector<Cls> cl;
            by_work = false;
            if (build_classes(batches[bi], cl)) return -1;
            uint32_t sh = 1000;   // per mille of the full slot counts: the largest that fits (down to 1 %: below that, more batches)
            // (the slots of the need buckets: from the largest need down while everything fits - at 140 Mb, 215 GB of a 257 GB budget, that is 3 % faster: the
            // long chains of the large buckets all start at once, 0.499 against 0.515 s - and in proportion to the buckets' work as soon as the budget binds:
            // 0.595 against 0.731 s under 140 GB, and one rank's 400 Mb share of configs[4] 2.00 against 2.95 s in its 260 GB)
            if (total_bytes(cl, sh) > budget) { by_work = true; if (build_classes(batches[bi], cl)) return -1; }   // (... and the buckets half an octave apart)
            batch_by_work[bi] = by_work;
            if (total_bytes(cl, sh) > budget) {
                uint32_t lo = 10, hi = 1000;
                while (hi - lo > 10) { const uint32_t mid = (lo + hi) / 2; if (total_bytes(cl, mid) <= budget) lo = mid; else hi = mid; }
                sh = lo;
            }
            batch_shrink[bi] = sh;
            fits = total_bytes(cl, sh) <= budget;
        }
        if (fits) break;
        if (nb >= todo.size()) return fail("hx_poa_batch: a single edge needs more POA workspace than the device has free");
    }
    return 0;
}

// the pruned instance: unshared edges, direction bytes, 4 or 8 columns per lane, a workgroup of several waves - or of any width when its edges take their
// columns in passes (a one-wave workgroup that holds its gap has nothing to skip: its rows are whole rows)
bool PoaPlanner::launch_pruned(const Cls& q) const {
    if (q.shared) return hxk::poa_prune_ok(q.dir, (int)q.cm) && prune_shared_pct != 0;
    return hxk::poa_prune_ok(q.dir, (int)q.cm) && (q.nt >= (uint32_t)o.poa_prune_lanes || q.pk) && prune_pct != 0;
}

}  // namespace hxi
