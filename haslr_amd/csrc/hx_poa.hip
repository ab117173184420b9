// hx_poa.hip - the POA consensus call of the C-ABI: launch and collection of the batches the planner (hx_poa_plan.hip) lays out, the
// hx_poa_* entry points, the workspace reservation and the statistics of the last call.
#include "hx_poa_plan.h"

using namespace hxi;

// Every k_poa instance uses private memory (288 to 928 bytes per lane: spills, a by-value argument), and a hardware queue grows its scratch when a
// dispatch asks for more per wave than the queue has had - a trip through the runtime (an allocation of device memory: slow while the driver is still
// wiping what another process freed) that holds THAT launch back. In a process that has run the few-edge instances, the first many-edge call then had
// some of its launches held and others not, they reached the CUs in another order, and the call took 600-640 ms instead of 415-440 (tools/dev_cold.py:
// a 12 Mb context, then the 140 Mb one; bench.py's configs[3] leg: five runs of five). Once per process and device, every stream of the pool runs one
// wave that asks for the most: from hx_poa_reserve (beside the parse) or, without a reservation, before the first launches.
static int scratch_warm_once(hx_ctx* c) {
    static std::mutex warm_mu;
    static std::vector<char> warmed;
    std::lock_guard<std::mutex> lk(warm_mu);
    if ((int)warmed.size() <= c->device) warmed.resize((size_t)c->device + 1, 0);
    if (warmed[(size_t)c->device]) return 0;
    for (int i = 0; i < 8; i++) hxk::scratch_warm(c->poa_streams[i]);
    for (int i = 0; i < 8; i++) HIPCHK(hipStreamSynchronize(c->poa_streams[i]));
    warmed[(size_t)c->device] = 1;
    return 0;
}

static double since(std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count(); }   // milliseconds

namespace {
// One consensus call: the PLAN (PoaPlanner, hx_poa_plan.hip: sub-sequences, per-edge capacities, launch classes, workspace slots and batches against the
// memory budget), the LAUNCH of a batch, and the COLLECTION of its results with the verdict on every edge (done / again with more room / again another way).
struct PoaCall : PoaPlanner {
    hx_ctx* c;
    const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    struct CnsView { const char* p = nullptr; size_t n = 0; const char* data() const { return p; } size_t size() const { return n; } };
    std::vector<CnsView> cns;                            // per edge: where its finished consensus lies in ...
    std::vector<std::unique_ptr<char[]>> cns_blocks;     // ... the download of its batch (kept to the end of the call: no copy per edge, no zero fill)

    PoaCall(hx_ctx* c_, const PoaInput& in_, const hx_poa_params* pp_) : PoaPlanner(in_, pp_, c_->opt, c_->poa_block, c_->poa_no_dir), c(c_), cns(in_.n_edge) {}
    double ms_since_start() const { return since(t0); }
    // ---- launch of one batch: what needs the device. The arithmetic is the layout's three steps (PoaPlanner::layout_slots, ::layout_order, ::layout_launches), each
    // taken where it has always stood among the HIP calls: the device works on what is queued meanwhile, and the launches leave when their inputs are on the way
    struct Launched { std::vector<uint32_t> edges; uint64_t bytes = 0; };   // what the collection needs afterwards
    int launch_batch(const std::vector<uint32_t>& batch, uint32_t shrink, Launched& lb) {
        hipStream_t s = c->stream;
        PoaPoolBufs& B = c->poa_pools;
        BatchLayout Y;
        if (layout_slots(batch, shrink, Y)) return -1;
        lb.edges = batch; lb.bytes = Y.bytes;
        // ---- the arena. It grows when a batch needs more than it holds - by an eighth more than asked, so that the retries of a call (a few edges with more
        // room) do not each allocate again - and never shrinks.
        {
            const auto tw0 = std::chrono::steady_clock::now();
            const size_t at = Y.at;
            std::lock_guard<std::mutex> lk(c->poa_arena_mu);
            if (at > c->poa_arena.cap) {
                HIPCHK(hipStreamSynchronize(s));   // (nothing of an earlier batch is in flight: collect_batch has read its results)
                hipError_t e = c->poa_arena.ensure(std::min<size_t>(at + at / 8, std::max<size_t>(at, (size_t)budget + (size_t)ne * 8400)));
                if (e != hipSuccess) { (void)hipGetLastError(); e = c->poa_arena.ensure(at); }
                if (e != hipSuccess) {
                    // the budget was taken from what hipMemGetInfo called free - which somebody else (another context on this device: ranks that share a GPU, another
                    // process) has taken since. The caller looks again and plans anew with what is there now.
                    (void)hipGetLastError();
                    g_err = "hx_poa_batch: cannot allocate " + std::to_string(at >> 20) + " MB of POA workspace: " + hipGetErrorString(e);
                    return 1;
                }
            }
            B.bind(c->poa_arena.p, Y.off);
            c->poa_host_ms[1] += since(tw0);
        }
        c->poa_workspace_bytes = std::max<uint64_t>(c->poa_workspace_bytes, Y.bytes);
        c->poa_last_workspace_bytes = std::max<uint64_t>(c->poa_last_workspace_bytes, Y.bytes);
        // ---- memsets and uploads: the edges, the order list, the slots, the counters, the groups' tables
        const auto te0 = std::chrono::steady_clock::now();
        HIPCHK(hipMemsetAsync(B.csync, 0, (size_t)ne * 8 * 4, s));
        if (Y.tot.clo) HIPCHK(hipMemsetAsync(B.mbox, 0, Y.tot.clo * 8, s));   // tag 0 = nothing published
        HIPCHK(c->poa_edges.reserve(ne)); HIPCHK(c->poa_len.reserve(ne)); HIPCHK(c->poa_status.reserve(ne));
        layout_order(Y);   // (beside the memsets)
        HIPCHK(hipMemcpyAsync(c->poa_edges.p, P.edges.data(), (size_t)ne * sizeof(hxk::PoaEdge), hipMemcpyHostToDevice, s));
        HIPCHK(c->poa_order.reserve(Y.order_all.size()));
        HIPCHK(hipMemcpyAsync(c->poa_order.p, Y.order_all.data(), Y.order_all.size() * 4, hipMemcpyHostToDevice, s));
        HIPCHK(c->poa_slots.reserve(Y.h_slots.size()));
        HIPCHK(hipMemcpyAsync(c->poa_slots.p, Y.h_slots.data(), Y.h_slots.size() * sizeof(hxk::PoaSlot), hipMemcpyHostToDevice, s));
        HIPCHK(c->poa_counters.reserve(Y.classes.size()));
        HIPCHK(hipMemsetAsync(c->poa_counters.p, 0, Y.classes.size() * 4, s));
        c->tick();
        layout_launches(Y);   // (beside the uploads)
        HIPCHK(c->poa_btab.reserve(std::max<size_t>(1, Y.h_btab.size())));
        if (!Y.h_btab.empty()) HIPCHK(hipMemcpyAsync(c->poa_btab.p, Y.h_btab.data(), Y.h_btab.size() * 4, hipMemcpyHostToDevice, s));
        if (scratch_warm_once(c)) return -1;
        HIPCHK(hipEventRecord(c->poa_ev[8], s));
        // ---- the launches: a record of the layout + the addresses
        const hxk::PoaPools pools = B.view();
        for (size_t gi = 0, si = 0; gi < Y.launches.size(); gi++) {
            const PoaLaunchRec& rec = Y.launches[gi];
            const int sk = rec.stream;
            for (; si < rec.shapes_end; si++) { const auto& es = Y.shapes[si]; c->poa_shape.cls[es[0]] = (uint8_t)es[1]; c->poa_shape.shape[es[0]] = es[2]; }   // (the launch's own, as ever between two launches)
            c->poa_shape.ring[rec.code] = rec.R;
            HIPCHK(hipStreamWaitEvent(c->poa_streams[sk], c->poa_ev[8], 0));
            hxk::PoaLaunch L = rec.L;   // every scalar; now every pointer
            L.edges = c->poa_edges.p; L.seqs = c->poa_seqs.p; L.packed = in.d_packed; L.read_off = in.d_roff; L.read_len = in.d_rlen; L.pools = pools;
            L.cns = B.cns; L.cns_len = c->poa_len.p; L.status = c->poa_status.p; L.cells = c->poa_cells_d.p; L.phase = c->poa_phase_d.p;
            L.order = c->poa_order.p + rec.order_at; L.slots = c->poa_slots.p + rec.slot_at;
            L.counter = rec.persistent ? c->poa_counters.p + rec.counter_at : nullptr; L.btab = rec.persistent ? c->poa_btab.p + rec.btab_at : nullptr;
            L.started = rec.started_at >= 0 ? c->poa_started + rec.started_at : nullptr;
            if (L.started) *(volatile uint32_t*)L.started = 0u;
            if (o.debug) { int occ = 0; L.occupancy = &occ; hxk::poa_run(L, c->poa_streams[sk]); L.occupancy = nullptr; fprintf(stderr, "[hx] launch %zu: %zu workgroups of %u lanes, %.1f KB of ring: %d workgroups per CU\n", gi, (size_t)L.n_blocks, (unsigned)L.block_threads, rec.lds_bytes / 1024.0, occ); }
            hxk::poa_run(L, c->poa_streams[sk]);
            HIPCHK(hipEventRecord(c->poa_ev[sk], c->poa_streams[sk]));
            HIPCHK(hipStreamWaitEvent(s, c->poa_ev[sk], 0));
            if (rec.wait != PoaLaunchRec::kNoWait) {   // the head start of a wide or a shared launch (layout_launches)
                HIPCHK(hipEventSynchronize(c->poa_ev[8]));   // (what precedes the launches on `s` is done: the wide launch is starting)
                const auto tw = std::chrono::steady_clock::now();
                if (rec.wait == PoaLaunchRec::kWaitStarted) {
                    // (round 6: not a fixed delay but the launch's own word - every workgroup adds itself when it begins. One pass in five of the 140 Mb call took 610-650 ms
                    // instead of 440-470: no edge redone, the same launches - in another order of arrival on the CUs. The shared edges' members and the wide classes
                    // must be the oldest waves where they sit; the next launch leaves when they have all begun, or after 2 ms)
                    volatile uint32_t* w = L.started;
                    while (*w < L.n_blocks && since(tw) < 2.0) { }
                    if (o.debug) fprintf(stderr, "[hx] launch %zu: %u of %u workgroups had begun %.0f us after the launch\n", gi, (unsigned)*w, L.n_blocks, since(tw) * 1000.0);
                } else
                    while (since(tw) * 1000.0 < o.poa_wide_delay_us) { }
            }
        }
        // ---- the laps
        const double enqueue_ms = since(te0);
        const auto te1 = std::chrono::steady_clock::now();
        c->tock(3);
        c->poa_host_ms[2] += enqueue_ms;
        c->poa_host_ms[3] += since(te1);
        HIPCHK(hipGetLastError());
        if (o.debug) {
            HIPCHK(hipStreamSynchronize(s));
            fprintf(stderr, "[hx] POA batch: %zu edges, %.2f GB workspace, workgroups", batch.size(), Y.bytes / 1e9);
            for (const Cls& q : Y.classes) fprintf(stderr, " %s%s%s%s%ux%u:%zu(%zu edges, largest %.1f MB)", q.shared ? "shared/" : "", q.persistent ? "persistent/" : "", q.dir ? "" : "matrix/",
                                                   launch_pruned(q) ? (q.pk ? "pruned/passes/" : "pruned/") : "", q.nt, q.cm, q.blocks, q.edges.size(), need_bytes(q.need) / 1e6);
            fprintf(stderr, ", %.1f ms since the call began\n", ms_since_start());
        }
        return 0;
    }

    // ---- collection: consensus strings of the edges that are done; the others go to `retry` (worst-case workspace next) / `retry_same` (another way)
    int collect_batch(const Launched& lb, std::vector<uint32_t>& retry, std::vector<uint32_t>& retry_same) {
        hipStream_t s = c->stream;
        std::vector<uint32_t> h_len(ne), h_status(ne);
        HIPCHK(hipMemcpy(h_len.data(), c->poa_len.p, (size_t)ne * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(h_status.data(), c->poa_status.p, (size_t)ne * 4, hipMemcpyDeviceToHost));
        // the finished strings, moved side by side on the device before the download: the buffer the kernels write into is sized by the node estimates
        // (100 MB for the 13 000 edges of a 140 Mb genome, of which 30 MB are consensus)
        std::vector<uint32_t> desc;
        std::vector<uint64_t> dense_off(lb.edges.size() + 1, 0);
        desc.reserve(lb.edges.size() * 5);
        for (size_t i = 0; i < lb.edges.size(); i++) {
            const uint32_t e = lb.edges[i];
            const uint32_t n = h_status[e] ? 0u : std::min<uint32_t>(h_len[e], P.edges[e].vcap);
            dense_off[i + 1] = dense_off[i] + n;
            if (!n) continue;
            const uint64_t so = P.edges[e].cns_off, to = dense_off[i];
            desc.insert(desc.end(), {(uint32_t)so, (uint32_t)(so >> 32), (uint32_t)to, (uint32_t)(to >> 32), n});
        }
        cns_blocks.emplace_back(new char[std::max<uint64_t>(1, dense_off.back())]);
        const char* h_cns = cns_blocks.back().get();
        if (!desc.empty()) {
            HIPCHK(c->poa_gather.reserve(desc.size())); HIPCHK(c->poa_cns_dense.reserve(dense_off.back()));
            HIPCHK(hipMemcpyAsync(c->poa_gather.p, desc.data(), desc.size() * 4, hipMemcpyHostToDevice, s));
            hxk::gather_bytes(c->poa_pools.cns, c->poa_gather.p, (uint32_t)(desc.size() / 5), c->poa_cns_dense.p, s);
            HIPCHK(hipMemcpyAsync(cns_blocks.back().get(), c->poa_cns_dense.p, dense_off.back(), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
        }
        {
            size_t n_far = 0, n_nodir = 0, n_over = 0, n_wide = 0, n_sinks = 0, n_stall = 0;
            for (uint32_t e : lb.edges) { n_far += !!(h_status[e] & HXE_POA_FARROWS); n_nodir += !!(h_status[e] & HXE_POA_NODIR); n_over += !!(h_status[e] & HXE_POA_OVERFLOW); n_wide += !!(h_status[e] & HXE_POA_WIDEROWS); n_sinks += !!(h_status[e] & HXE_POA_SINKS); n_stall += !!(h_status[e] & HXE_POA_STALLED); }
            const size_t n6[6] = {n_far, n_nodir, n_over, n_wide, n_sinks, n_stall};
            for (int k = 0; k < 6; k++) c->poa_retry[k] += n6[k];   // (hx_poa_retry_stats)
            if (o.debug && n_far + n_nodir + n_over + n_wide + n_sinks + n_stall) fprintf(stderr, "[hx] POA batch: to be redone: %zu (rows read back from HBM outgrew H), %zu (in-degree above the direction bytes' limit), %zu (graph outgrew its workspace), %zu (rows with more than 4 predecessors outgrew the wide-row pool), %zu (more sink rows than the launch keeps), %zu (members of a shared edge not resident together%s: unshared next)\n",
                                                                       n_far, n_nodir, n_over, n_wide, n_sinks, n_stall, balanced ? ", in a balanced launch" : "");
        }
        for (size_t i = 0; i < lb.edges.size(); i++) {
            const uint32_t e = lb.edges[i];
            if (h_status[e] & HXE_POA_FARROWS) { if (P.edges[e].hrows >= P.edges[e].vcap + 1) return fail("hx_poa_batch: internal error (far-row retry)"); far_full[e]++; retry_same.push_back(e); continue; }
            if (h_status[e] & HXE_POA_STALLED) {
                if (P.edges[e].members < 2) return fail("hx_poa_batch: internal error (a wave of an unshared edge gave up waiting)");
                no_share[e] = 1; retry_same.push_back(e); continue;
            }
            if (h_status[e] & HXE_POA_WIDEROWS) { if (P.edges[e].wrows >= P.edges[e].vcap + 1) return fail("hx_poa_batch: internal error (wide-row retry)"); wide_grow[e]++; retry_same.push_back(e); continue; }
            if (h_status[e] & HXE_POA_SINKS) { if (many_sinks[e]) return fail("hx_poa_batch: internal error (sink-list retry)"); many_sinks[e] = 1; retry_same.push_back(e); continue; }
            if (h_status[e] & HXE_POA_NODIR) { if (force_nodir[e]) return fail("hx_poa_batch: internal error (direction-byte retry)"); force_nodir[e] = 1; retry_same.push_back(e); continue; }
            if (h_status[e] & ~(uint32_t)HXE_POA_OVERFLOW) return fail("hx_poa_batch: internal error (kernel variant / column count mismatch)");
            if (h_status[e] & HXE_POA_OVERFLOW) {
                if (P.edges[e].vcap >= P.sumL[e]) return fail("hx_poa_batch: POA workspace overflow at worst-case size (internal error)");
                grow[e]++;
                retry.push_back(e);
            } else cns[e] = CnsView{h_cns + dense_off[i], (size_t)(dense_off[i + 1] - dense_off[i])};
        }
        return 0;
    }
};
}  // namespace

static int poa_consensus(hx_ctx* c, const PoaInput& in, const hx_poa_params* pp, hx_cns_out* out) {
    memset(out, 0, sizeof(*out));
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    PoaCall K(c, in, pp);
    const uint32_t ne = K.ne;
    std::vector<uint32_t> todo;
    for (double& v : c->poa_host_ms) v = 0;
    for (uint64_t& v : c->poa_retry) v = 0;
    if (K.plan_input(todo)) return -1;
    c->poa_host_ms[0] += K.ms_since_start();
    if (c->opt.debug) fprintf(stderr, "[hx] POA call: %u edges prepared in %.1f ms\n", (unsigned)ne, K.ms_since_start());
    PoaCallShape& sh = c->poa_shape;
    sh.cls.assign(ne, POA_NO_CLASS); for (int k = 0; k < 11; k++) sh.ring[k] = 0;
    sh.shape.assign(ne, 0);
    sh.nseq = K.P.nseq; sh.lmax.resize(ne); for (uint32_t e = 0; e < ne; e++) sh.lmax[e] = K.P.edges[e].lmax;
    HIPCHK(c->poa_seqs.reserve(K.P.seqs.size()));
    if (!K.P.seqs.empty()) HIPCHK(hipMemcpyAsync(c->poa_seqs.p, K.P.seqs.data(), K.P.seqs.size() * sizeof(hxk::PoaSeq), hipMemcpyHostToDevice, s));
    HIPCHK(c->poa_cells_d.reserve(1));
    HIPCHK(hipMemsetAsync(c->poa_cells_d.p, 0, 8, s));
    if (!c->poa_budget) {   // measured once: later calls would count the context's own (persistent) workspace as used
        size_t free_b = 0, total_b = 0;
        HIPCHK(hipMemGetInfo(&free_b, &total_b));
        { std::lock_guard<std::mutex> lk(c->poa_arena_mu); free_b += c->poa_arena.cap; }   // (an arena reserved ahead - hx_poa_reserve - is the workspace's own)
        c->poa_budget = (uint64_t)(free_b * 0.9);
        c->poa_free_at_first_call = free_b;
    }
    // option poa_workspace_gb: cap of the POA workspace (default: 90 % of what was free when the context first ran a consensus). The workgroups in
    // flight per launch class are scaled down until the slots fit. Measured at 140 Mb (13 230 edges): 257 GB 2.0-2.1 s, 138 GB 2.10-2.13 s (and
    // the first call, which allocates the pools, 4.1 instead of 5-7.6 s), 39 GB 4.6 s, 22 GB 8.5 s; a 400 Mb genome (37 608 edges): 148 GB 6.7 s.
    // (Round 6, measured on the 140 Mb data set, 13 197 edges: 0.50 s with the 215 GB the plan takes of a 257 GB budget, 0.75-0.90 s under a cap of 140 GB, 1.04 s
    // under 100 GB - the slot counts of the one-wave classes are what shrinks. No cap of its own, then: 90 % of what is free.)
    K.budget = c->opt.poa_workspace_gb > 0 ? (uint64_t)(c->opt.poa_workspace_gb * 1e9) : c->poa_budget;
    c->poa_last_workspace_bytes = 0;
    HIPCHK(c->poa_phase_d.reserve((size_t)ne * hxk::POA_PHASE_WORDS));
    HIPCHK(hipMemsetAsync(c->poa_phase_d.p, 0, std::max<size_t>(1, (size_t)ne * hxk::POA_PHASE_WORDS) * 8, s));
    while (!todo.empty()) {
        const auto tp0 = std::chrono::steady_clock::now();
        if (K.knobs(todo.size()) || K.size_edges(todo)) return -1;
        const double t_size = since(tp0);
        std::vector<std::vector<uint32_t>> batches;
        std::vector<uint32_t> batch_shrink;
        if (K.plan_batches(todo, batches, batch_shrink)) return -1;
        c->poa_host_ms[0] += since(tp0);
        if (c->opt.debug) fprintf(stderr, "[hx] POA plan: widths and rooms of %zu edges %.2f ms, batches and slots %.2f ms\n", todo.size(), t_size, since(tp0) - t_size);
        std::vector<uint32_t> retry, retry_same;   // retry with the worst-case workspace / with the score-matrix traceback
        for (size_t bi = 0; bi < batches.size(); bi++) {
            if (batches[bi].empty()) continue;
            PoaCall::Launched lb;
            K.by_work = bi < K.batch_by_work.size() && K.batch_by_work[bi] != 0;
            const int rc = K.launch_batch(batches[bi], batch_shrink[bi], lb);
            if (rc == 1) {   // the arena could not be had at the planned size: the budget again from what is free NOW, the rest of the round planned anew
                size_t free_b = 0, total_b = 0;
                HIPCHK(hipMemGetInfo(&free_b, &total_b));
                uint64_t now_b;
                { std::lock_guard<std::mutex> lk(c->poa_arena_mu); now_b = (uint64_t)((double)(free_b + c->poa_arena.cap) * 0.9); }
                if (now_b + (now_b >> 6) >= K.budget) return -1;   // (nothing changed: the error stands)
                if (c->opt.debug) fprintf(stderr, "[hx] POA workspace: %.1f GB could not be allocated; %.1f GB are free now, budget %.1f -> %.1f GB\n", lb.bytes / 1e9, free_b / 1e9, K.budget / 1e9, now_b / 1e9);
                K.budget = now_b;
                if (c->opt.poa_workspace_gb <= 0) c->poa_budget = now_b;
                for (size_t bj = bi; bj < batches.size(); bj++) retry_same.insert(retry_same.end(), batches[bj].begin(), batches[bj].end());
                break;
            }
            if (rc) return -1;
            const auto tc0 = std::chrono::steady_clock::now();
            const int rc_collect = K.collect_batch(lb, retry, retry_same);
            c->poa_host_ms[4] += since(tc0);
            if (rc_collect) return -1;
        }
        todo.swap(retry);
        todo.insert(todo.end(), retry_same.begin(), retry_same.end());
    }
    const auto tf0 = std::chrono::steady_clock::now();
    unsigned long long cells = 0;
    HIPCHK(hipMemcpy(&cells, c->poa_cells_d.p, 8, hipMemcpyDeviceToHost));
    c->poa_phase.resize((size_t)ne * hxk::POA_PHASE_WORDS);
    if (ne) HIPCHK(hipMemcpy(c->poa_phase.data(), c->poa_phase_d.p, (size_t)ne * hxk::POA_PHASE_WORDS * 8, hipMemcpyDeviceToHost));
    std::vector<uint64_t> off((size_t)ne + 1, 0);
    for (uint32_t e = 0; e < ne; e++) off[e + 1] = off[e] + K.cns[e].size();
    out->n_edge = ne;
    out->cns_off = (uint64_t*)malloc(((size_t)ne + 1) * 8); memcpy(out->cns_off, off.data(), ((size_t)ne + 1) * 8);
    out->cns = (char*)malloc(std::max<uint64_t>(1, off[ne]));
    {   // (30 MB of strings at 140 Mb: a few threads, each its range of the edges)
        const uint32_t nt = off[ne] > (4u << 20) ? 4u : 1u;
        auto part = [&](uint32_t t) { for (uint32_t e = (uint32_t)((uint64_t)ne * t / nt); e < (uint32_t)((uint64_t)ne * (t + 1) / nt); e++) if (K.cns[e].size()) memcpy(out->cns + off[e], K.cns[e].data(), K.cns[e].size()); };
        std::vector<std::thread> th;
        for (uint32_t t = 1; t < nt; t++) th.emplace_back(part, t);
        part(0);
        for (std::thread& x : th) x.join();
    }
    out->dp_cells = cells; out->seq_bases = K.seq_bases; out->n_aligned = K.n_aligned;
    c->poa_host_ms[5] = since(tf0); c->poa_host_ms[7] = K.ms_since_start();
    if (c->opt.debug) fprintf(stderr, "[hx] POA call, host wall time: plan %.1f ms, workspace %.1f ms (%llu device allocations so far, %.0f ms), enqueue %.1f ms, device %.1f ms, collect %.1f ms, finish %.1f ms, total %.1f ms\n",
                              c->poa_host_ms[0], c->poa_host_ms[1], (unsigned long long)c->poa_arena.n_alloc, c->poa_arena.alloc_ms, c->poa_host_ms[2], c->poa_host_ms[3], c->poa_host_ms[4], c->poa_host_ms[5], c->poa_host_ms[7]);
    return 0;
}

extern "C" int hx_poa_batch(hx_ctx* c, const hx_poa_params* pp, hx_cns_out* out) {
    memset(out, 0, sizeof(*out));
    if (!c->have_coords) return fail("hx_poa_batch: hx_edge_coords has not run");
    const PoaInput in{c->coords.n_sel, c->coords.h_supp_off.data(), c->coords.h_supp_lr.data(), c->coords.h_spos.data(), c->coords.h_epos.data(), c->h_rlen.data(), c->packed.p, c->roff.p, c->rlen.p};
    return poa_consensus(c, in, pp, out);
}

extern "C" int hx_poa_supports(hx_ctx* c, const hx_coords_out* sup, const hx_poa_params* pp, hx_cns_out* out) {
    memset(out, 0, sizeof(*out));
    if (!c->n_reads) return fail("hx_poa_supports: no reads are resident (hx_upload)");
    for (uint64_t k = 0; k < sup->supp_off[sup->n_edge]; k++)
        if ((sup->supp_lr[k] & 0x7fffffffu) >= c->n_reads) return fail("hx_poa_supports: long-read id out of range");
    const PoaInput in{sup->n_edge, sup->supp_off, sup->supp_lr, sup->spos, sup->epos, c->h_rlen.data(), c->packed.p, c->roff.p, c->rlen.p};
    return poa_consensus(c, in, pp, out);
}

extern "C" int hx_poa_sequences(hx_ctx* c, uint32_t n_sets, const uint64_t* set_off, const uint64_t* seq_off, const char* bases, const hx_poa_params* pp, hx_cns_out* out) {
    memset(out, 0, sizeof(*out));
    HIPCHK(hipSetDevice(c->device));
    const uint64_t nseq = set_off[n_sets];
    if (nseq >= 0x7fffffffULL) return fail("hx_poa_sequences: too many sequences");
    // pack like the long reads (2 bits, A0 C1 G2 T3, anything else A; every sequence on a 4-byte boundary) and align them whole, forward
    std::vector<uint32_t> len(nseq), lr(nseq), sp(nseq, 0), ep(nseq);
    std::vector<uint64_t> off(nseq + 1, 0);
    for (uint64_t i = 0; i < nseq; i++) {
        const uint64_t L = seq_off[i + 1] - seq_off[i];
        if (L >= 0xffffffffULL) return fail("hx_poa_sequences: sequence too long");
        len[i] = (uint32_t)L; lr[i] = (uint32_t)i; ep[i] = (uint32_t)L - 1;   // an empty sequence gives epos = spos - 1: skipped, as in the reference (Assemble.cpp:537)
        off[i + 1] = off[i] + ((L + 15) / 16) * 4;
    }
    std::vector<uint8_t> packed(std::max<uint64_t>(4, off[nseq]), 0);
    for (uint64_t i = 0; i < nseq; i++)
        for (uint32_t j = 0; j < len[i]; j++) {
            packed[off[i] + (j >> 2)] |= (uint8_t)(hxk::base_code(bases[seq_off[i] + j]) << ((j & 3) * 2));
        }
    DV<uint8_t> d_packed; DV<uint64_t> d_off; DV<uint32_t> d_len;
    if (up(d_packed, packed.data(), packed.size()) || up(d_off, off.data(), off.size()) || up(d_len, len.data(), std::max<size_t>(1, len.size()))) return -1;
    const PoaInput in{n_sets, set_off, lr.data(), sp.data(), ep.data(), len.data(), d_packed.p, d_off.p, d_len.p};
    const int rc = poa_consensus(c, in, pp, out);
    HIPCHK(hipStreamSynchronize(c->stream));
    return rc;
}

// ---- the general path (kernels/poa_modes.hip). Its entry points differ in what they validate and in the outputs they hand over; the call itself is one.
// The scores of a call of the general path and its gap model (kernels/poa_modes.h: 0 linear, 1 affine, 2 convex); open2 / extend2 count under the convex model only
struct GapScores { int32_t match, mismatch, open, extend, open2, extend2, type; int model; };

// The request of an entry point `who` (the name its errors carry), as far as every entry has it; the entry adds its own flags.
static hxk::PoaModesArgs general_args(const char* who, uint32_t n_sets, const uint64_t* set_off, const uint64_t* seq_off, const char* bases, const GapScores& sc) {
    hxk::PoaModesArgs a;
    a.who = who; a.n_sets = n_sets; a.set_off = set_off; a.seq_off = seq_off; a.bases = bases;
    a.match = sc.match; a.mismatch = sc.mismatch; a.gap = sc.open; a.gap_extend = sc.extend; a.gap_open2 = sc.open2; a.gap_extend2 = sc.extend2; a.type = sc.type; a.gap_model = sc.model;
    return a;
}

// runs a validated request with the context's options, books its time and prints the debug line (tag: what that line calls the entry)
static int poa_general_run(hx_ctx* c, const char* tag, hxk::PoaModesArgs& a, hxk::PoaModesOut& o) {
    HIPCHK(hipSetDevice(c->device));
    a.slot_kb_cap = (uint32_t)std::max(0, c->opt.poa_modes_slot_kb); a.aln_cap = (uint32_t)std::max(0, c->opt.poa_graph_aln_cap); a.workspace_gb = c->opt.poa_workspace_gb; a.debug = c->opt.debug;
    std::string err;
    if (hxk::poa_modes_run(c->stream, c->poa_modes_ws, a, o, err)) return fail(err);
    c->tm.ms[3] += o.kernel_ms; c->tm.launches[3] += o.launches;
    if (c->opt.debug) {
        char rows[96] = "", part[96] = "";   // what an MSA or a weighted call adds to the line
        if (a.msa) { snprintf(rows, sizeof rows, "%zu bytes of rows, ", o.msa.size()); snprintf(part, sizeof part, " (rows %.3f ms)", o.msa_rows_ms); }
        if (a.weighted) snprintf(part, sizeof part, " (coverage %.3f ms)", o.cov_ms);
        if (a.strand) snprintf(part, sizeof part, " (%llu of %llu sequences reversed)", (unsigned long long)o.third_passes, (unsigned long long)o.n_aligned);
        if (a.band) snprintf(part, sizeof part, " (band %u, %u reruns after a band miss)", a.band, o.band_reruns);
        if (a.graph) { snprintf(rows, sizeof rows, "%zu nodes, %zu edges, %zu pairs, ", o.node_base.size(), o.edge_w.size(), o.aln_pos.size()); snprintf(part, sizeof part, " (gather %.3f ms, %u sets rerun for their alignments)", o.gather_ms, o.aln_retried); }
        fprintf(stderr, "[hx] POA %s call%s: %u sets, %.3g cells, %skernels %.2f ms%s, %u sets rerun in a larger slot\n", tag, hxk::gap_model_label(a.gap_model), a.n_sets, (double)o.cells, rows, o.kernel_ms, part, o.retried);
    }
    return 0;
}

// a malloc'ed copy for an output struct (freed by hx_free_*)
template <class T> static T* dup(const T* p, size_t n) { void* q = malloc(std::max<size_t>(1, n * sizeof(T))); memcpy(q, p, n * sizeof(T)); return (T*)q; }

static int poa_general_call(hx_ctx* c, hxk::PoaModesArgs a, hx_cns_out* out) {
    hxk::PoaModesOut o;
    if (poa_general_run(c, "modes", a, o)) return -1;
    out->n_edge = a.n_sets;
    out->cns_off = dup(o.cns_off.data(), (size_t)a.n_sets + 1);
    out->cns = dup(o.cns.data(), o.cns.size());
    out->dp_cells = o.cells; out->seq_bases = o.seq_bases; out->n_aligned = o.n_aligned;
    return 0;
}

extern "C" int hx_poa_sequences_mode(hx_ctx* c, uint32_t n_sets, const uint64_t* set_off, const uint64_t* seq_off, const char* bases, const hx_poa_mode_params* mp, hx_cns_out* out) {
    memset(out, 0, sizeof(*out));
    if (!mp) return fail("hx_poa_sequences_mode: no parameters");
    if (mp->gap >= 0) return fail("hx_poa_sequences_mode: the gap score must be negative (linear gap penalty), not " + std::to_string(mp->gap));
    if (mp->type != HX_POA_SW && mp->type != HX_POA_NW && mp->type != HX_POA_OV) return fail("hx_poa_sequences_mode: unknown alignment type " + std::to_string(mp->type) + " (HX_POA_SW 0, HX_POA_NW 1, HX_POA_OV 2)");
    if (set_off[n_sets] >= 0x7fffffffULL) return fail("hx_poa_sequences_mode: too many sequences");
    const hx_poa_params pp{mp->match, mp->mismatch, mp->gap};
    if (mp->type == HX_POA_NW && !c->opt.poa_general) return hx_poa_sequences(c, n_sets, set_off, seq_off, bases, &pp, out);   // the tuned global path
    return poa_general_call(c, general_args("hx_poa_sequences_mode", n_sets, set_off, seq_off, bases, GapScores{mp->match, mp->mismatch, mp->gap, mp->gap, 0, 0, mp->type, 0}), out);
}

// what hx_poa_sequences_affine, hx_poa_msa and hx_poa_weighted ask of their scores, type and sequence count (0 = fine)
static int check_affine_call(const std::string& who, int32_t gap_open, int32_t gap_extend, int32_t type, uint64_t n_seq) {
    if (gap_open >= 0) return fail(who + ": the gap open score must be negative, not " + std::to_string(gap_open));
    if (gap_extend > 0) return fail(who + ": the gap extend score must not be positive, not " + std::to_string(gap_extend));
    // (spoa is said to fall back to its linear engine here, silently; that cannot be checked without the library, so the call is refused)
    if (gap_extend < gap_open) return fail(who + ": the gap extend score " + std::to_string(gap_extend) + " is below the gap open score " + std::to_string(gap_open) + " (extending a gap must not cost more than opening one)");
    if (type != HX_POA_SW && type != HX_POA_NW && type != HX_POA_OV) return fail(who + ": unknown alignment type " + std::to_string(type) + " (HX_POA_SW 0, HX_POA_NW 1, HX_POA_OV 2)");
    if (n_seq >= 0x7fffffffULL) return fail(who + ": too many sequences");
    return 0;
}

// what the three convex entries ask on top of that: the second piece is a valid piece of its own and opens no cheaper than the first
static int check_convex_call(const std::string& who, const hx_poa_convex_params& p, uint64_t n_seq) {
    if (check_affine_call(who, p.gap_open, p.gap_extend, p.type, n_seq)) return -1;
    if (p.gap_open2 >= 0) return fail(who + ": the second gap open score must be negative, not " + std::to_string(p.gap_open2));
    if (p.gap_extend2 > 0) return fail(who + ": the second gap extend score must not be positive, not " + std::to_string(p.gap_extend2));
    if (p.gap_extend2 < p.gap_open2) return fail(who + ": the second gap extend score " + std::to_string(p.gap_extend2) + " is below the second gap open score " + std::to_string(p.gap_open2) + " (extending a gap must not cost more than opening one)");
    if (p.gap_open2 > p.gap_open) return fail(who + ": the second gap open score " + std::to_string(p.gap_open2) + " is above the first gap open score " + std::to_string(p.gap_open) + " (the first piece is the one that opens no dearer)");
    return 0;
}
// a second piece that extends no cheaper than the first never wins (it opens no cheaper either): the call is the affine one with the first piece,
// unless option poa_convex keeps it on the convex kernel (the cross-check of that kernel against the affine one)
static bool convex_is_affine(const hx_ctx* c, const hx_poa_convex_params& p) { return p.gap_extend2 <= p.gap_extend && !c->opt.poa_convex; }
static GapScores convex_scores(const hx_poa_convex_params& p) { return GapScores{p.match, p.mismatch, p.gap_open, p.gap_extend, p.gap_open2, p.gap_extend2, p.type, 2}; }
// the scores of hx_poa_graph and hx_poa_strand, which have the convex entries' parameters only: when the second piece never wins, the call takes the affine route
static GapScores convex_or_affine_scores(const hx_ctx* c, const hx_poa_convex_params& p) {
    GapScores sc = convex_scores(p);
    if (convex_is_affine(c, p)) { sc.open2 = sc.extend2 = 0; sc.model = p.gap_extend != p.gap_open || c->opt.poa_affine; }
    return sc;
}

extern "C" int hx_poa_sequences_affine(hx_ctx* c, uint32_t n_sets, const uint64_t* set_off, const uint64_t* seq_off, const char* bases, const hx_poa_affine_params* ap, hx_cns_out* out) {
    memset(out, 0, sizeof(*out));
    if (!ap) return fail("hx_poa_sequences_affine: no parameters");
    if (check_affine_call("hx_poa_sequences_affine", ap->gap_open, ap->gap_extend, ap->type, set_off[n_sets])) return -1;
    if (ap->gap_extend == ap->gap_open && !c->opt.poa_affine) {   // the linear model: the linear paths (kNW keeps the tuned one)
        const hx_poa_mode_params mp{ap->match, ap->mismatch, ap->gap_open, ap->type};
        return hx_poa_sequences_mode(c, n_sets, set_off, seq_off, bases, &mp, out);
    }
    return poa_general_call(c, general_args("hx_poa_sequences_affine", n_sets, set_off, seq_off, bases, GapScores{ap->match, ap->mismatch, ap->gap_open, ap->gap_extend, 0, 0, ap->type, 1}), out);
}

extern "C" int hx_poa_sequences_convex(hx_ctx* c, uint32_t n_sets, const uint64_t* set_off, const uint64_t* seq_off, const char* bases, const hx_poa_convex_params* cp, hx_cns_out* out) {
    memset(out, 0, sizeof(*out));
    if (!cp) return fail("hx_poa_sequences_convex: no parameters");
    if (check_convex_call("hx_poa_sequences_convex", *cp, set_off[n_sets])) return -1;
    if (convex_is_affine(c, *cp)) {
        const hx_poa_affine_params ap{cp->match, cp->mismatch, cp->gap_open, cp->gap_extend, cp->type};
        return hx_poa_sequences_affine(c, n_sets, set_off, seq_off, bases, &ap, out);
    }
    return poa_general_call(c, general_args("hx_poa_sequences_convex", n_sets, set_off, seq_off, bases, convex_scores(*cp)), out);
}

// the multiple sequence alignment of every set: the general path's MSA instances (all three types: the tuned kNW path keeps no node per
// base) of the gap model the scores name
static int poa_msa_call(hx_ctx* c, const char* who, uint32_t n_sets, const uint64_t* set_off, const uint64_t* seq_off, const char* bases, const GapScores& sc, int include_consensus, hx_msa_out* out) {
    hxk::PoaModesArgs a = general_args(who, n_sets, set_off, seq_off, bases, sc);
    a.msa = 1; a.include_consensus = include_consensus != 0;
    hxk::PoaModesOut o;
    if (poa_general_run(c, "MSA", a, o)) return -1;
    out->n_set = n_sets;
    out->n_rows = dup(o.msa_rows.data(), n_sets);
    out->n_cols = dup(o.msa_cols.data(), n_sets);
    out->msa_off = dup(o.msa_off.data(), (size_t)n_sets + 1);
    out->msa = dup(o.msa.data(), o.msa.size());
    out->cns_off = dup(o.cns_off.data(), (size_t)n_sets + 1);
    out->cns = dup(o.cns.data(), o.cns.size());
    out->dp_cells = o.cells; out->seq_bases = o.seq_bases; out->n_aligned = o.n_aligned;
    out->rows_kernel_ms = o.msa_rows_ms; out->rows_kernel_bytes = o.msa_moved_bytes;
    return 0;
}

// linear instances when the two gap scores are equal
extern "C" int hx_poa_msa(hx_ctx* c, uint32_t n_sets, const uint64_t* set_off, const uint64_t* seq_off, const char* bases, const hx_poa_msa_params* mp, hx_msa_out* out) {
    memset(out, 0, sizeof(*out));
    if (!mp) return fail("hx_poa_msa: no parameters");
    if (check_affine_call("hx_poa_msa", mp->gap_open, mp->gap_extend, mp->type, set_off[n_sets])) return -1;
    return poa_msa_call(c, "hx_poa_msa", n_sets, set_off, seq_off, bases, GapScores{mp->match, mp->mismatch, mp->gap_open, mp->gap_extend, 0, 0, mp->type, mp->gap_extend != mp->gap_open || c->opt.poa_affine}, mp->include_consensus, out);
}

extern "C" int hx_poa_msa_convex(hx_ctx* c, uint32_t n_sets, const uint64_t* set_off, const uint64_t* seq_off, const char* bases, const hx_poa_convex_params* cp, int include_consensus, hx_msa_out* out) {
    memset(out, 0, sizeof(*out));
    if (!cp) return fail("hx_poa_msa_convex: no parameters");
    if (check_convex_call("hx_poa_msa_convex", *cp, set_off[n_sets])) return -1;
    if (convex_is_affine(c, *cp)) {
        const hx_poa_msa_params mp{cp->match, cp->mismatch, cp->gap_open, cp->gap_extend, cp->type, include_consensus != 0};
        return hx_poa_msa(c, n_sets, set_off, seq_off, bases, &mp, out);
    }
    return poa_msa_call(c, "hx_poa_msa_convex", n_sets, set_off, seq_off, bases, convex_scores(*cp), include_consensus, out);
}

// the consensus under per-base weights with coverage and profile: the general path's instances that keep the node of every base (all
// three types), the weighted ones when weights are given
// 0, or the error that names the first weight of 0
static int check_weights(const std::string& who, uint32_t n_sets, const uint64_t* set_off, const uint64_t* seq_off, const uint8_t* weights) {
    if (weights)
        for (uint32_t i = 0; i < n_sets; i++)
            for (uint64_t k = set_off[i]; k < set_off[i + 1]; k++)
                for (uint64_t p = seq_off[k]; p < seq_off[k + 1]; p++)
                    if (weights[p] == 0)
                        return fail(who + ": set " + std::to_string(i) + ", sequence " + std::to_string(k - set_off[i]) + ", position " + std::to_string(p - seq_off[k]) + ": a weight of 0 is not accepted (weights are 1..255)");
    return 0;
}

static int poa_weighted_call(hx_ctx* c, const std::string& who, uint32_t n_sets, const uint64_t* set_off, const uint64_t* seq_off, const char* bases, const uint8_t* weights, const GapScores& sc,
                             int want_coverage, int want_profile, hx_wcns_out* out) {
    if (check_weights(who, n_sets, set_off, seq_off, weights)) return -1;
    hxk::PoaModesArgs a = general_args(who.c_str(), n_sets, set_off, seq_off, bases, sc);
    a.weighted = 1; a.weights = weights; a.want_coverage = want_coverage != 0; a.want_profile = want_profile != 0;
    std::vector<uint8_t> ones;
    if (!weights && c->opt.poa_weighted) { ones.assign(std::max<uint64_t>(1, seq_off[set_off[n_sets]]), 1); a.weights = ones.data(); }
    hxk::PoaModesOut o;
    if (poa_general_run(c, "weighted", a, o)) return -1;
    out->n_set = n_sets;
    out->cns_off = dup(o.cns_off.data(), (size_t)n_sets + 1);
    out->cns = dup(o.cns.data(), o.cns.size());
    if (a.want_coverage || a.want_profile) out->coverage = dup(o.cov.data(), o.cov.size());
    if (a.want_profile) out->profile = dup(o.prof.data(), o.prof.size());
    out->dp_cells = o.cells; out->seq_bases = o.seq_bases; out->n_aligned = o.n_aligned;
    out->cov_kernel_ms = o.cov_ms; out->cov_kernel_bytes = o.cov_moved_bytes;
    return 0;
}

extern "C" int hx_poa_weighted(hx_ctx* c, uint32_t n_sets, const uint64_t* set_off, const uint64_t* seq_off, const char* bases, const uint8_t* weights, const hx_poa_weighted_params* wp, hx_wcns_out* out) {
    memset(out, 0, sizeof(*out));
    if (!wp) return fail("hx_poa_weighted: no parameters");
    if (check_affine_call("hx_poa_weighted", wp->gap_open, wp->gap_extend, wp->type, set_off[n_sets])) return -1;
    return poa_weighted_call(c, "hx_poa_weighted", n_sets, set_off, seq_off, bases, weights, GapScores{wp->match, wp->mismatch, wp->gap_open, wp->gap_extend, 0, 0, wp->type, wp->gap_extend != wp->gap_open || c->opt.poa_affine},
                             wp->want_coverage, wp->want_profile, out);
}

extern "C" int hx_poa_weighted_convex(hx_ctx* c, uint32_t n_sets, const uint64_t* set_off, const uint64_t* seq_off, const char* bases, const uint8_t* weights, const hx_poa_convex_params* cp, int want_coverage,
                                      int want_profile, hx_wcns_out* out) {
    memset(out, 0, sizeof(*out));
    if (!cp) return fail("hx_poa_weighted_convex: no parameters");
    if (check_convex_call("hx_poa_weighted_convex", *cp, set_off[n_sets])) return -1;
    if (convex_is_affine(c, *cp)) {
        const hx_poa_weighted_params wp{cp->match, cp->mismatch, cp->gap_open, cp->gap_extend, cp->type, want_coverage != 0, want_profile != 0};
        return hx_poa_weighted(c, n_sets, set_off, seq_off, bases, weights, &wp, out);
    }
    return poa_weighted_call(c, "hx_poa_weighted_convex", n_sets, set_off, seq_off, bases, weights, convex_scores(*cp), want_coverage, want_profile, out);
}

// the graph, the paths and the alignments of every set: the general path's graph instances (all three types) of the gap model the scores
// name, chosen by the rules of the convex entries
extern "C" int hx_poa_graph(hx_ctx* c, uint32_t n_sets, const uint64_t* set_off, const uint64_t* seq_off, const char* bases, const uint8_t* weights, const hx_poa_convex_params* cp, hx_graph_out* out) {
    memset(out, 0, sizeof(*out));
    if (!cp) return fail("hx_poa_graph: no parameters");
    if (check_convex_call("hx_poa_graph", *cp, set_off[n_sets])) return -1;
    if (check_weights("hx_poa_graph", n_sets, set_off, seq_off, weights)) return -1;
    hxk::PoaModesArgs a = general_args("hx_poa_graph", n_sets, set_off, seq_off, bases, convex_or_affine_scores(c, *cp));
    a.graph = 1; a.weights = weights;
    hxk::PoaModesOut o;
    if (poa_general_run(c, "graph", a, o)) return -1;
    const uint64_t n_seq = set_off[n_sets];
    out->n_set = n_sets; out->n_seq = n_seq;
    out->node_off = dup(o.node_off.data(), (size_t)n_sets + 1);
    out->node_base = dup(o.node_base.data(), o.node_base.size()); out->node_rank = dup(o.node_rank.data(), o.node_rank.size()); out->node_col = dup(o.node_col.data(), o.node_col.size());
    out->edge_off = dup(o.edge_off.data(), (size_t)n_sets + 1);
    out->edge_from = dup(o.edge_from.data(), o.edge_from.size()); out->edge_to = dup(o.edge_to.data(), o.edge_to.size()); out->edge_w = dup(o.edge_w.data(), o.edge_w.size());
    out->base_node = dup(o.base_node.data(), o.base_node.size());
    out->cns_off = dup(o.cns_off.data(), (size_t)n_sets + 1);
    out->cns = dup(o.cns.data(), o.cns.size()); out->cns_node = dup(o.cns_node.data(), o.cns_node.size());
    out->aln_off = dup(o.aln_off.data(), (size_t)n_seq + 1);
    out->aln_node = dup(o.aln_node.data(), o.aln_node.size()); out->aln_pos = dup(o.aln_pos.data(), o.aln_pos.size()); out->aln_score = dup(o.aln_score.data(), o.aln_score.size());
    out->dp_cells = o.cells; out->seq_bases = o.seq_bases; out->n_aligned = o.n_aligned;
    out->gather_kernel_ms = o.gather_ms; out->gather_kernel_bytes = o.gather_moved_bytes;
    out->slot_reruns = o.retried; out->aln_reruns = o.aln_retried;
    return 0;
}

// the consensus of sets whose sequences may lie on either strand: the general path's strand instances (all three types) of the gap model
// the scores name, chosen by hx_poa_graph's rules
extern "C" int hx_poa_strand(hx_ctx* c, uint32_t n_sets, const uint64_t* set_off, const uint64_t* seq_off, const char* bases, const uint8_t* weights, const hx_poa_convex_params* cp,
                             const hx_poa_strand_want* want, hx_strand_out* out) {
    memset(out, 0, sizeof(*out));
    if (!cp || !want) return fail("hx_poa_strand: no parameters");
    if (check_convex_call("hx_poa_strand", *cp, set_off[n_sets])) return -1;
    if (check_weights("hx_poa_strand", n_sets, set_off, seq_off, weights)) return -1;
    hxk::PoaModesArgs a = general_args("hx_poa_strand", n_sets, set_off, seq_off, bases, convex_or_affine_scores(c, *cp));
    a.strand = 1; a.weights = weights;
    a.msa = want->want_msa != 0; a.include_consensus = a.msa && want->include_consensus != 0;
    a.want_coverage = want->want_coverage != 0; a.want_profile = want->want_profile != 0;
    hxk::PoaModesOut o;
    if (poa_general_run(c, "strand", a, o)) return -1;
    const uint64_t n_seq = set_off[n_sets];
    out->n_set = n_sets; out->n_seq = n_seq;
    out->cns_off = dup(o.cns_off.data(), (size_t)n_sets + 1);
    out->cns = dup(o.cns.data(), o.cns.size());
    out->reversed = dup(o.reversed.data(), o.reversed.size()); out->score_fwd = dup(o.score_fwd.data(), o.score_fwd.size()); out->score_rev = dup(o.score_rev.data(), o.score_rev.size());
    if (a.msa) {
        out->n_rows = dup(o.msa_rows.data(), n_sets); out->n_cols = dup(o.msa_cols.data(), n_sets);
        out->msa_off = dup(o.msa_off.data(), (size_t)n_sets + 1); out->msa = dup(o.msa.data(), o.msa.size());
    }
    if (a.want_coverage || a.want_profile) out->coverage = dup(o.cov.data(), o.cov.size());
    if (a.want_profile) out->profile = dup(o.prof.data(), o.prof.size());
    out->dp_cells = o.cells; out->seq_bases = o.seq_bases; out->n_aligned = o.n_aligned; out->third_passes = o.third_passes;
    out->slot_reruns = o.retried;
    return 0;
}

// the consensus of sets aligned inside an adaptive band: the general path's band instances (all three types) of the gap model the scores
// name, chosen by hx_poa_graph's rules; sets that miss their band climb to twice the band and at last to the full-matrix instances
extern "C" int hx_poa_banded(hx_ctx* c, uint32_t n_sets, const uint64_t* set_off, const uint64_t* seq_off, const char* bases, const uint8_t* weights, const hx_poa_convex_params* cp,
                             const hx_poa_band_params* bp, hx_band_out* out) {
    memset(out, 0, sizeof(*out));
    if (!cp || !bp) return fail("hx_poa_banded: no parameters");
    if (check_convex_call("hx_poa_banded", *cp, set_off[n_sets])) return -1;
    if (bp->band < 1 || bp->band > hxk::MAX_BAND) return fail("hx_poa_banded: the band half-width must be 1.." + std::to_string(hxk::MAX_BAND) + ", not " + std::to_string(bp->band));
    if (check_weights("hx_poa_banded", n_sets, set_off, seq_off, weights)) return -1;
    hxk::PoaModesArgs a = general_args("hx_poa_banded", n_sets, set_off, seq_off, bases, convex_or_affine_scores(c, *cp));
    a.band = bp->band; a.weights = weights;
    a.msa = bp->want_msa != 0; a.include_consensus = a.msa && bp->include_consensus != 0;
    a.want_coverage = bp->want_coverage != 0; a.want_profile = bp->want_profile != 0;
    a.weighted = weights || a.msa || a.want_coverage || a.want_profile;   // (the consensus alone keeps no node per base)
    hxk::PoaModesOut o;
    if (poa_general_run(c, "banded", a, o)) return -1;
    out->n_set = n_sets;
    out->cns_off = dup(o.cns_off.data(), (size_t)n_sets + 1);
    out->cns = dup(o.cns.data(), o.cns.size());
    out->band_used = dup(o.band_used.data(), n_sets);
    if (a.msa) {
        out->n_rows = dup(o.msa_rows.data(), n_sets); out->n_cols = dup(o.msa_cols.data(), n_sets);
        out->msa_off = dup(o.msa_off.data(), (size_t)n_sets + 1); out->msa = dup(o.msa.data(), o.msa.size());
    }
    if (a.want_coverage || a.want_profile) out->coverage = dup(o.cov.data(), o.cov.size());
    if (a.want_profile) out->profile = dup(o.prof.data(), o.prof.size());
    out->dp_cells = o.cells; out->seq_bases = o.seq_bases; out->n_aligned = o.n_aligned; out->workspace_bytes = o.workspace_bytes;
    out->slot_reruns = o.retried; out->band_reruns = o.band_reruns;
    return 0;
}

// one consensus per caller-given label over the one graph of every set: the general path's label instances (all three types) of the gap
// model the scores name, chosen by hx_poa_graph's rules
extern "C" int hx_poa_labelled(hx_ctx* c, uint32_t n_sets, const uint64_t* set_off, const uint64_t* seq_off, const char* bases, const uint8_t* weights, const uint8_t* labels,
                               const hx_poa_convex_params* cp, const hx_poa_label_params* lp, hx_label_out* out) {
    memset(out, 0, sizeof(*out));
    if (!cp || !lp) return fail("hx_poa_labelled: no parameters");
    if (check_convex_call("hx_poa_labelled", *cp, set_off[n_sets])) return -1;
    if (lp->n_labels < 1 || lp->n_labels > 16) return fail("hx_poa_labelled: n_labels must be 1..16, not " + std::to_string(lp->n_labels));
    if (!labels) return fail("hx_poa_labelled: no labels");
    for (uint32_t i = 0; i < n_sets; i++)
        for (uint64_t k = set_off[i]; k < set_off[i + 1]; k++)
            if (labels[k] >= lp->n_labels && labels[k] != 255)
                return fail("hx_poa_labelled: set " + std::to_string(i) + ", sequence " + std::to_string(k - set_off[i]) + ": label " + std::to_string(labels[k]) + " is not below n_labels = " + std::to_string(lp->n_labels) + " and not 255 (no label)");
    if (check_weights("hx_poa_labelled", n_sets, set_off, seq_off, weights)) return -1;
    hxk::PoaModesArgs a = general_args("hx_poa_labelled", n_sets, set_off, seq_off, bases, convex_or_affine_scores(c, *cp));
    a.labels = labels; a.n_labels = lp->n_labels; a.weights = weights;
    a.msa = lp->want_msa != 0; a.include_consensus = a.msa && lp->include_consensus != 0;
    a.want_coverage = lp->want_coverage != 0; a.want_profile = lp->want_profile != 0;
    hxk::PoaModesOut o;
    if (poa_general_run(c, "labelled", a, o)) return -1;
    out->n_set = n_sets; out->n_labels = lp->n_labels;
    out->cns_off = dup(o.cns_off.data(), o.cns_off.size());
    out->cns = dup(o.cns.data(), o.cns.size());
    out->cns_col = dup(o.cns_col.data(), o.cns_col.size());
    if (a.msa) {
        out->n_rows = dup(o.msa_rows.data(), n_sets); out->n_cols = dup(o.msa_cols.data(), n_sets);
        out->msa_off = dup(o.msa_off.data(), (size_t)n_sets + 1); out->msa = dup(o.msa.data(), o.msa.size());
    }
    if (a.want_coverage || a.want_profile) out->coverage = dup(o.cov.data(), o.cov.size());
    if (a.want_profile) out->profile = dup(o.prof.data(), o.prof.size());
    out->dp_cells = o.cells; out->seq_bases = o.seq_bases; out->n_aligned = o.n_aligned;
    out->slot_reruns = o.retried;
    return 0;
}

extern "C" void hx_free_label(hx_ctx*, hx_label_out* o) {
    free(o->cns_off); free(o->cns); free(o->cns_col); free(o->coverage); free(o->profile); free(o->n_rows); free(o->n_cols); free(o->msa_off); free(o->msa);
    memset(o, 0, sizeof(*o));
}

// two consensus strings per set from reads the call phases itself: the general path's phase instances (the label instances with the phasing
// of the set's reads in front of the per-label views), chosen by hx_poa_graph's rules
extern "C" int hx_poa_phased(hx_ctx* c, uint32_t n_sets, const uint64_t* set_off, const uint64_t* seq_off, const char* bases, const uint8_t* weights,
                             const hx_poa_convex_params* cp, const hx_poa_phase_params* pp, hx_phase_out* out) {
    memset(out, 0, sizeof(*out));
    if (!cp || !pp) return fail("hx_poa_phased: no parameters");
    if (check_convex_call("hx_poa_phased", *cp, set_off[n_sets])) return -1;
    if (pp->min_count < 1 || pp->min_count > 255) return fail("hx_poa_phased: min_count must be 1..255, not " + std::to_string(pp->min_count));
    if (pp->min_pct < 1 || pp->min_pct > 50) return fail("hx_poa_phased: min_pct must be 1..50, not " + std::to_string(pp->min_pct));
    if (check_weights("hx_poa_phased", n_sets, set_off, seq_off, weights)) return -1;
    hxk::PoaModesArgs a = general_args("hx_poa_phased", n_sets, set_off, seq_off, bases, convex_or_affine_scores(c, *cp));
    a.phase = 1; a.phase_min_count = pp->min_count; a.phase_min_pct = pp->min_pct; a.weights = weights;
    a.msa = pp->want_msa != 0; a.include_consensus = a.msa && pp->include_consensus != 0;
    a.want_coverage = pp->want_coverage != 0; a.want_profile = pp->want_profile != 0;
    hxk::PoaModesOut o;
    if (poa_general_run(c, "phased", a, o)) return -1;
    out->n_set = n_sets; out->n_labels = 2;
    out->cns_off = dup(o.cns_off.data(), o.cns_off.size());
    out->cns = dup(o.cns.data(), o.cns.size());
    out->cns_col = dup(o.cns_col.data(), o.cns_col.size());
    if (a.msa) {
        out->n_rows = dup(o.msa_rows.data(), n_sets); out->n_cols = dup(o.msa_cols.data(), n_sets);
        out->msa_off = dup(o.msa_off.data(), (size_t)n_sets + 1); out->msa = dup(o.msa.data(), o.msa.size());
    }
    if (a.want_coverage || a.want_profile) out->coverage = dup(o.cov.data(), o.cov.size());
    if (a.want_profile) out->profile = dup(o.prof.data(), o.prof.size());
    out->dp_cells = o.cells; out->seq_bases = o.seq_bases; out->n_aligned = o.n_aligned;
    out->slot_reruns = o.retried;
    out->hap = dup(o.hap.data(), o.hap.size());
    out->n_haps = dup(o.n_haps.data(), n_sets); out->rounds = dup(o.phase_rounds.data(), n_sets); out->site_off = dup(o.site_off.data(), (size_t)n_sets + 1);
    out->site_col = dup(o.site_col.data(), o.site_col.size()); out->site_a1 = dup(o.site_a1.data(), o.site_a1.size());
    out->site_a2 = dup(o.site_a2.data(), o.site_a2.size()); out->site_phase = dup(o.site_phase.data(), o.site_phase.size());
    return 0;
}

extern "C" void hx_free_phase(hx_ctx*, hx_phase_out* o) {
    free(o->cns_off); free(o->cns); free(o->cns_col); free(o->coverage); free(o->profile); free(o->n_rows); free(o->n_cols); free(o->msa_off); free(o->msa);
    free(o->hap); free(o->n_haps); free(o->rounds); free(o->site_off); free(o->site_col); free(o->site_a1); free(o->site_a2); free(o->site_phase);
    memset(o, 0, sizeof(*o));
}
extern "C" void hx_free_band(hx_ctx*, hx_band_out* o) {
    free(o->cns_off); free(o->cns); free(o->band_used); free(o->n_rows); free(o->n_cols); free(o->msa_off); free(o->msa); free(o->coverage); free(o->profile);
    memset(o, 0, sizeof(*o));
}
extern "C" void hx_free_strand(hx_ctx*, hx_strand_out* o) {
    free(o->cns_off); free(o->cns); free(o->reversed); free(o->score_fwd); free(o->score_rev); free(o->n_rows); free(o->n_cols); free(o->msa_off); free(o->msa);
    free(o->coverage); free(o->profile);
    memset(o, 0, sizeof(*o));
}
extern "C" void hx_free_graph(hx_ctx*, hx_graph_out* o) {
    free(o->node_off); free(o->node_base); free(o->node_rank); free(o->node_col); free(o->edge_off); free(o->edge_from); free(o->edge_to); free(o->edge_w); free(o->base_node);
    free(o->cns_off); free(o->cns); free(o->cns_node); free(o->aln_off); free(o->aln_node); free(o->aln_pos); free(o->aln_score);
    memset(o, 0, sizeof(*o));
}
extern "C" void hx_free_wcns(hx_ctx*, hx_wcns_out* o) { free(o->cns_off); free(o->cns); free(o->coverage); free(o->profile); memset(o, 0, sizeof(*o)); }
extern "C" void hx_free_cns(hx_ctx*, hx_cns_out* o) { free(o->cns_off); free(o->cns); memset(o, 0, sizeof(*o)); }
extern "C" void hx_free_msa(hx_ctx*, hx_msa_out* o) { free(o->n_rows); free(o->n_cols); free(o->msa_off); free(o->msa); free(o->cns_off); free(o->cns); memset(o, 0, sizeof(*o)); }

extern "C" uint32_t hx_poa_phase_cycles(hx_ctx* c, uint64_t* sum6, uint64_t* max6) { return poa_phase_report(c->poa_shape.view(c->poa_phase, c->opt.debug, c->opt.prof, stderr), sum6, max6).edges; }
extern "C" uint64_t hx_poa_workspace_bytes(const hx_ctx* c) { return c->poa_workspace_bytes; }
extern "C" int hx_poa_release_workspace(hx_ctx* c) {
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    { std::lock_guard<std::mutex> lk(c->poa_arena_mu); c->poa_arena.release(); }
    c->poa_modes_ws.release();
    c->poa_budget = 0;   // taken again, from what is free then, by the next consensus call
    return 0;
}
extern "C" int hx_poa_reserve(hx_ctx* c, uint64_t bytes) {
    // the arena of the consensus workspace, ahead of the first call (the CLI: on a thread of its own, beside the parse of the text inputs): at most 80 % of
    // what is free now (counting what the arena already holds), whatever the caller guessed; a later call that needs more allocates again
    HIPCHK(hipSetDevice(c->device));
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    std::lock_guard<std::mutex> lk(c->poa_arena_mu);
    uint64_t cap_b = (uint64_t)((double)(free_b + c->poa_arena.cap) * 0.8);                             // (the inputs go beside it: hx_upload gives the arena back if they do not fit)
    if (c->opt.poa_workspace_gb > 0) cap_b = std::min<uint64_t>(cap_b, (uint64_t)(c->opt.poa_workspace_gb * 1.02e9) + (64ull << 20));   // (option poa_workspace_gb: no call will take more)
    const size_t want = (size_t)std::min<uint64_t>(bytes, cap_b);
    if (want <= c->poa_arena.cap) return 0;
    const hipError_t e = c->poa_arena.ensure(want);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(std::string("hx_poa_reserve: ") + hipGetErrorString(e)); }
    if (scratch_warm_once(c)) return -1;
    return 0;
}
extern "C" void hx_poa_host_times(const hx_ctx* c, double* ms8) { for (int k = 0; k < 8; k++) ms8[k] = c->poa_host_ms[k]; }
extern "C" void hx_poa_arena_stats(const hx_ctx* c, uint64_t* capacity, uint64_t* allocations, double* alloc_ms) { *capacity = c->poa_arena.cap; *allocations = c->poa_arena.n_alloc; *alloc_ms = c->poa_arena.alloc_ms; }
extern "C" void hx_poa_memory_stats(const hx_ctx* c, uint64_t* free_at_first_call, uint64_t* budget, uint64_t* last_call_workspace) {
    *free_at_first_call = c->poa_free_at_first_call; *budget = c->poa_budget; *last_call_workspace = c->poa_last_workspace_bytes;
}
extern "C" void hx_poa_prune_stats(const hx_ctx* c, uint64_t* out4) { poa_prune_sums(c->poa_phase.data(), c->poa_phase.size() / hxk::POA_PHASE_WORDS, out4); }
extern "C" void hx_poa_retry_stats(const hx_ctx* c, uint64_t* out6) { for (int k = 0; k < 6; k++) out6[k] = c->poa_retry[k]; }
extern "C" void hx_set_poa_traceback(hx_ctx* c, int use_direction_bytes) { c->poa_no_dir = !use_direction_bytes; }
extern "C" void hx_set_poa_block(hx_ctx* c, int t) { c->poa_block = t <= 0 ? 0 : t >= 1024 ? 1024 : t >= 512 ? 512 : t >= 256 ? 256 : t >= 128 ? 128 : 64; }
