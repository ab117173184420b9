// hx_api.hip — implementation of the C-ABI in include/haslr_hip.h: device context, resident inputs, options,
// the chain, edge and coordinate operators (kernel orchestration + result download), timing. The POA consensus is in hx_poa.hip (its
// planner in hx_poa_plan.hip), the multi-GPU group in hx_group.hip.
// There is no CPU fallback here: without a usable HIP device every entry point fails with an error.
#include "hx_internal.h"

using namespace hxi;

namespace hxi {
thread_local std::string g_err;
int fail(const std::string& m) { g_err = m; return -1; }
}  // namespace hxi

namespace {
struct OptDesc { const char* name; int HxOptions::*ip; double HxOptions::*dp; };
const OptDesc kOptions[] = {
    {"debug", &HxOptions::debug, nullptr}, {"prof", &HxOptions::prof, nullptr}, {"poa_workspace_gb", nullptr, &HxOptions::poa_workspace_gb},
    {"poa_poll_limit", &HxOptions::poa_poll_limit, nullptr}, {"poa_max_indeg", &HxOptions::poa_max_indeg, nullptr}, {"poa_member_lanes", &HxOptions::poa_member_lanes, nullptr},
    {"poa_cluster_min", &HxOptions::poa_cluster_min, nullptr}, {"poa_cluster_max", &HxOptions::poa_cluster_max, nullptr}, {"poa_cluster_topk", &HxOptions::poa_cluster_topk, nullptr},
    {"poa_wide_members", &HxOptions::poa_wide_members, nullptr}, {"poa_cluster_cols", &HxOptions::poa_cluster_cols, nullptr}, {"poa_cols2_top", &HxOptions::poa_cols2_top, nullptr}, {"poa_node_est_pct", &HxOptions::poa_node_est_pct, nullptr},
    {"poa_far_rows", &HxOptions::poa_far_rows, nullptr}, {"poa_far_shift", &HxOptions::poa_far_shift, nullptr}, {"poa_wave_max", &HxOptions::poa_wave_max, nullptr}, {"poa_cols", &HxOptions::poa_cols, nullptr},
    {"poa_ring_kb", &HxOptions::poa_ring_kb, nullptr}, {"poa_ring_zero", &HxOptions::poa_ring_zero, nullptr}, {"poa_balance", &HxOptions::poa_balance, nullptr},
    {"poa_balance_pct", &HxOptions::poa_balance_pct, nullptr}, {"poa_balance_lanes", &HxOptions::poa_balance_lanes, nullptr}, {"poa_slots_pct", &HxOptions::poa_slots_pct, nullptr},
    {"poa_slots", &HxOptions::poa_slots, nullptr}, {"poa_batches", &HxOptions::poa_batches, nullptr}, {"poa_force_cm", &HxOptions::poa_force_cm, nullptr},
    {"poa_streams", &HxOptions::poa_streams, nullptr}, {"poa_wide_delay_us", &HxOptions::poa_wide_delay_us, nullptr},
    {"poa_prune", &HxOptions::poa_prune, nullptr}, {"poa_prune_lanes", &HxOptions::poa_prune_lanes, nullptr}, {"poa_prune_lazy", &HxOptions::poa_prune_lazy, nullptr}, {"poa_prune_shared", &HxOptions::poa_prune_shared, nullptr}, {"poa_pass_lanes", &HxOptions::poa_pass_lanes, nullptr}, {"poa_chain_ms", &HxOptions::poa_chain_ms, nullptr}, {"poa_chain_pct", &HxOptions::poa_chain_pct, nullptr}, {"poa_resident_first", &HxOptions::poa_resident_first, nullptr}, {"poa_own_bucket_first", &HxOptions::poa_own_bucket_first, nullptr}, {"coords_lds_supp", &HxOptions::coords_lds_supp, nullptr},
    {"poa_general", &HxOptions::poa_general, nullptr}, {"poa_modes_slot_kb", &HxOptions::poa_modes_slot_kb, nullptr},
    {"poa_affine", &HxOptions::poa_affine, nullptr}, {"poa_weighted", &HxOptions::poa_weighted, nullptr}, {"poa_convex", &HxOptions::poa_convex, nullptr},
    {"poa_graph_aln_cap", &HxOptions::poa_graph_aln_cap, nullptr}, {"poa_strand_one_h", &HxOptions::poa_strand_one_h, nullptr},
};
}  // namespace

extern "C" const char* hx_last_error(void) { return g_err.c_str(); }

extern "C" int hx_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return fail("hipGetDeviceCount failed: no usable HIP device (the HIP path has no CPU fallback)");
    return n;
}

// the streams, events and buffers of a new context; on failure the caller hands `c` to hx_ctx_destroy
static int ctx_init(hx_ctx* c, void* stream) {
    const int device = c->device;
    if (stream) c->stream = (hipStream_t)stream;
    else { HIPCHK(hipStreamCreate(&c->stream)); c->own_stream = true; }
    HIPCHK(hipEventCreate(&c->tm.a));
    HIPCHK(hipEventCreate(&c->tm.b));
    {   // distinct priorities map to distinct hardware queues, so the lane-count classes really run side by side.
        // Round 6: the eight streams of the launch classes are the PROCESS's, one set per device, created by the first context on it and handed to every later
        // one (never destroyed). A second context of a process used to run the 12 Mb step 13 % slower, whichever path it was - streams created when
        // the first context's had already taken the hardware queues do not get queues of their own, and destroying the first context did not give them back.
        static std::mutex pool_mu;
        static std::vector<std::array<hipStream_t, 8>> pool;   // by device
        std::lock_guard<std::mutex> lk(pool_mu);
        if ((int)pool.size() <= device) pool.resize((size_t)device + 1, std::array<hipStream_t, 8>{});
        if (!pool[(size_t)device][0]) {
            int lo = 0, hi = 0;
            HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));   // lo = least priority (largest number), hi = greatest
            std::array<hipStream_t, 8> made{};   // (published only once all eight exist: a later context must not find null streams)
            for (int i = 0; i < 8; i++) {
                int pr = hi + i; if (pr > lo) pr = lo;
                const hipError_t e = hipStreamCreateWithPriority(&made[(size_t)i], hipStreamNonBlocking, pr);
                if (e != hipSuccess) {
                    for (hipStream_t x : made) if (x) (void)hipStreamDestroy(x);
                    return fail(std::string("hipStreamCreateWithPriority: ") + hipGetErrorString(e));
                }
            }
            pool[(size_t)device] = made;
        }
        for (int i = 0; i < 8; i++) c->poa_streams[i] = pool[(size_t)device][(size_t)i];
    }
    for (int i = 0; i < 9; i++) HIPCHK(hipEventCreateWithFlags(&c->poa_ev[i], hipEventDisableTiming));
    HIPCHK(hipHostMalloc((void**)&c->poa_started, 16 * sizeof(uint32_t), hipHostMallocMapped));
    HIPCHK(c->err.reserve(1));
    return 0;
}

extern "C" int hx_ctx_create(int device, void* stream, hx_ctx** out) {
    *out = nullptr;
    // (the POA launch classes go to separate streams and overlap only with enough hardware queues: the APPLICATION sets GPU_MAX_HW_QUEUES >= 8
    //  before HIP initialises - haslr_assemble, haslr_amd/hip.py and bench.py do; the library does not touch the process environment)
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail("hx_ctx_create: no HIP device available (libhaslr_hip.so has no CPU fallback)");
    if (device < 0 || device >= n) return fail("hx_ctx_create: device index out of range");
    HIPCHK(hipSetDevice(device));
    hx_ctx* c = new hx_ctx;
    c->device = device;
    if (ctx_init(c, stream)) { hx_ctx_destroy(c); return -1; }   // (the shared pool streams are not the context's: hx_ctx_destroy leaves them)
    *out = c;
    return 0;
}

extern "C" void hx_ctx_destroy(hx_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->tm.a) (void)hipEventDestroy(c->tm.a);
    if (c->tm.b) (void)hipEventDestroy(c->tm.b);
    for (int i = 0; i < 9; i++) if (c->poa_ev[i]) (void)hipEventDestroy(c->poa_ev[i]);
    if (c->own_stream) (void)hipStreamDestroy(c->stream);
    if (c->poa_started) (void)hipHostFree(c->poa_started);
    delete c;
}

static int upload_inputs(hx_ctx* c, const hx_contigs* ctg, const hx_reads* rd, const hx_hits* h, const uint64_t* rho) {
    HIPCHK(hipSetDevice(c->device));
    c->n_contigs = ctg->n; c->n_reads = rd->n; c->n_hits = h->n; c->n_ops = h->cg_off[h->n];
    if (up(c->km, ctg->mean_kmer, ctg->n) || up(c->clen, ctg->len, ctg->n)) return -1;
    HIPCHK(c->cls.reserve(ctg->n));
    if (up(c->rlen, rd->len, rd->n) || up(c->roff, rd->off, (size_t)rd->n + 1) || up(c->packed, rd->packed, (size_t)rd->off[rd->n])) return -1;
    if (c->hits.upload(h, c->n_ops) || up(c->rho, rho, (size_t)rd->n + 1)) return -1;
    c->h_rlen.assign(rd->len, rd->len + rd->n);
    c->h_rho.assign(rho, rho + rd->n + 1);
    c->lr_begin = 0; c->lr_end = rd->n;
    c->prefiltered = false;
    c->have_chain = c->have_edges = c->have_coords = false;
    return 0;
}
extern "C" int hx_upload(hx_ctx* c, const hx_contigs* ctg, const hx_reads* rd, const hx_hits* h, const uint64_t* rho) {
    if (upload_inputs(c, ctg, rd, h, rho) == 0) return 0;
    // a consensus arena reserved ahead of the inputs (hx_poa_reserve) must never be what keeps them out: give it back and try once more
    {
        std::lock_guard<std::mutex> lk(c->poa_arena_mu);
        if (!c->poa_arena.cap) return -1;
        (void)hipGetLastError();
        c->poa_arena.release();
    }
    return upload_inputs(c, ctg, rd, h, rho);
}

extern "C" void hx_set_prefiltered(hx_ctx* c, int on) { c->prefiltered = on != 0; }

// option names: lower case, as in kOptions; the old environment variable spellings (HX_POA_SLOTS, HX_DEBUG ...) are accepted too
static std::string opt_key(const char* name) {
    std::string k(name ? name : "");
    for (char& ch : k) ch = (char)tolower((unsigned char)ch);
    if (k.rfind("hx_", 0) == 0) k = k.substr(3);
    return k;
}
extern "C" int hx_set_option(hx_ctx* c, const char* name, const char* value) {
    const std::string k = opt_key(name);
    const HxOptions dflt;
    const bool reset = !value || !*value;
    if (k == "prof1" || k == "prof2" || k == "prof3" || k == "prof4") { c->opt.prof = reset ? 0 : k[4] - '0'; return 0; }   // (HX_PROF1 / 2 / 3 / 4 of the development builds)
    for (const OptDesc& d : kOptions)
        if (k == d.name) {
            char* end = nullptr;
            if (d.ip) { const long v = reset ? dflt.*(d.ip) : strtol(value, &end, 10); if (!reset && (end == value || *end)) return fail(std::string("hx_set_option: ") + d.name + " takes an integer, not '" + value + "'"); c->opt.*(d.ip) = (int)v; }
            else { const double v = reset ? dflt.*(d.dp) : strtod(value, &end); if (!reset && (end == value || *end)) return fail(std::string("hx_set_option: ") + d.name + " takes a number, not '" + value + "'"); c->opt.*(d.dp) = v; }
            return 0;
        }
    return fail("hx_set_option: unknown option '" + std::string(name ? name : "") + "' (hx_option_names lists them)");
}
extern "C" const char* hx_option_names(void) {
    static const std::string names = [] { std::string n; for (const OptDesc& d : kOptions) { if (!n.empty()) n += ","; n += d.name; } return n; }();
    return names.c_str();
}
extern "C" int hx_get_option(const hx_ctx* c, const char* name, double* value) {
    const std::string k = opt_key(name);
    for (const OptDesc& d : kOptions) if (k == d.name) { *value = d.ip ? (double)(c->opt.*(d.ip)) : c->opt.*(d.dp); return 0; }
    return fail("hx_get_option: unknown option '" + std::string(name ? name : "") + "'");
}

extern "C" int hx_set_read_shard(hx_ctx* c, uint32_t b, uint32_t e) {
    if (b > e || e > c->n_reads) return fail("hx_set_read_shard: bad range");
    c->lr_begin = b; c->lr_end = e;
    return 0;
}

// the scan / sort launchers skip their work when their scratch cannot be allocated (Workspace::oom): nothing they were to write may be read
static int ws_ok(hx_ctx* c, const char* who) {
    if (!c->ws.oom) return 0;
    c->ws.oom = false;
    return fail(std::string(who) + ": out of device memory for scan / sort scratch");
}

static int check_err(hx_ctx* c, const char* who) {
    if (ws_ok(c, who)) return -1;
    uint32_t e = 0;
    HIPCHK(hipMemcpy(&e, c->err.p, 4, hipMemcpyDeviceToHost));
    if (!e) return 0;
    std::string m = std::string(who) + ":";
    if (e & HXE_TRIM_NO_M) m += " overlap trim ran off an alignment without M;";
    if (e & HXE_CHAIN_TOO_MANY) m += " more than 10000 chainable hits on one read (reference limit, Longread.cpp:529);";
    if (e & HXE_SPOS_RANGE) m += " consensus support starts beyond its read;";
    if (e & HXE_BAD_TID) m += " contig id out of range;";
    return fail(m);
}

// the end of an operator's download. A result array that could not be allocated or downloaded: the out-struct comes back freed and zeroed, the device side stays as it is
template <class O> static int downloaded(bool ok, hx_ctx* c, O* out, void (*release)(hx_ctx*, O*), const char* who) {
    return ok ? 0 : (release(c, out), fail(std::string(who) + ": a result array could not be allocated or downloaded"));
}

// ================================================================================================ K1-K3
extern "C" int hx_chain_reads(hx_ctx* c, const hx_params* prm, hx_chain_out* out) {
    memset(out, 0, sizeof(*out));
    HIPCHK(hipSetDevice(c->device));
    const uint32_t nr = c->lr_end - c->lr_begin;
    const uint64_t nraw = c->h_rho[c->lr_end] - c->h_rho[c->lr_begin];
    hipStream_t s = c->stream;
    HIPCHK(hipMemsetAsync(c->err.p, 0, 4, s));
    const double thr_load = prm->uniq_freq * (3 + prm->max_uniq_dev), thr_uniq = prm->uniq_freq * (1 + prm->max_uniq_dev);
    auto& S = c->sc_chain; auto& C = c->chain;   // the scratch at raw-hit granularity, the result
    c->ws.reset(s);
    HIPCHK(S.raw.reserve(nraw)); HIPCHK(S.dp.reserve(nraw)); HIPCHK(S.cmp.reserve(nraw)); HIPCHK(S.from.reserve(nraw));
    HIPCHK(S.naln.reserve(nr)); HIPCHK(S.ncmp.reserve(nr)); HIPCHK(C.aln_off.reserve((size_t)nr + 1)); HIPCHK(C.cmp_off.reserve((size_t)nr + 1));
    hxk::ChainScratch sc{}; S.raw.fill(sc); sc.dp = S.dp.p; sc.from = S.from.p; sc.cmp = S.cmp.p; sc.n_aln = S.naln.p; sc.n_cmp = S.ncmp.p;
    c->tick();
    hxk::contig_class(c->km.p, c->n_contigs, thr_load, thr_uniq, c->cls.p, s);
    hxk::chain_reads(c->hits_view(), c->rho.p, c->cls.p, c->n_contigs, c->lr_begin, c->lr_end, prm->min_aln_block, prm->min_aln_sim, prm->min_aln_mapq, sc, c->err.p, c->prefiltered, s);
    hxk::exclusive_scan_u32(S.naln.p, C.aln_off.p, nr, s, c->ws);
    hxk::exclusive_scan_u32(S.ncmp.p, C.cmp_off.p, nr, s, c->ws);
    if (ws_ok(c, "hx_chain_reads")) return -1;
    uint64_t tot[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(&tot[0], C.aln_off.p + nr, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&tot[1], C.cmp_off.p + nr, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const uint64_t n_aln = C.n_aln = tot[0], n_cmp = C.n_cmp = tot[1];
    if (n_aln >= 0xffffffffULL) return fail("hx_chain_reads: more than 2^32-1 alignments in one shard");
    HIPCHK(C.col.reserve(n_aln)); HIPCHK(C.cmp_aln.reserve(n_cmp));
    hxk::chain_compact(sc, c->rho.p, c->lr_begin, c->lr_end, C.aln_off.p, C.cmp_off.p, c->chain_view(), s);
    c->tock(0);
    HIPCHK(hipGetLastError());
    if (check_err(c, "hx_chain_reads")) return -1;
    c->have_chain = true; c->have_edges = c->have_coords = false;
    out->n_aln = n_aln; out->n_reads = nr; out->n_cmp = n_cmp;
    const bool ok = C.col.download(out, n_aln) && fetch(out->read_off, C.aln_off.p, (size_t)nr + 1) && fetch(out->cmp_off, C.cmp_off.p, (size_t)nr + 1) && fetch(out->cmp_aln, C.cmp_aln.p, n_cmp);
    return downloaded(ok, c, out, hx_free_chain, "hx_chain_reads");
}

extern "C" void hx_free_chain(hx_ctx*, hx_chain_out* o) { ChainCols::free_host(o); free(o->read_off); free(o->cmp_off); free(o->cmp_aln); memset(o, 0, sizeof(*o)); }

// ================================================================================================ K4
extern "C" int hx_edge_emit(hx_ctx* c, const hx_params*, uint64_t* n_records) {
    if (!c->have_chain) return fail("hx_edge_emit: hx_chain_reads has not run");
    HIPCHK(hipSetDevice(c->device));
    const uint32_t nr = c->lr_end - c->lr_begin;
    hipStream_t s = c->stream;
    auto& E = c->sc_edges;
    c->ws.reset(s);
    HIPCHK(E.npairs.reserve(nr)); HIPCHK(E.pair_off.reserve((size_t)nr + 1));
    c->tick();
    hxk::edge_count(c->hits_view(), c->cls.p, c->chain_view(), c->chain.cmp_off.p, c->lr_begin, c->lr_end, E.npairs.p, s);
    hxk::exclusive_scan_u32(E.npairs.p, E.pair_off.p, nr, s, c->ws);
    if (ws_ok(c, "hx_edge_emit")) return -1;
    uint64_t tot = 0;
    HIPCHK(hipMemcpyAsync(&tot, E.pair_off.p + nr, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    c->n_rec_un = 2 * tot;
    HIPCHK(c->rec_un.reserve(c->n_rec_un));
    hxk::edge_emit(c->hits_view(), c->cls.p, c->chain_view(), c->chain.cmp_off.p, c->lr_begin, c->lr_end, E.pair_off.p, c->rec_un.view(), s);
    c->tock(1);
    HIPCHK(hipGetLastError());
    if (n_records) *n_records = c->n_rec_un;
    return 0;
}

// sort the n records sitting in rec_un by key (stable), segment into edges, download
static int finish_edges(hx_ctx* c, uint64_t n, hx_edges_out* out) {
    hipStream_t s = c->stream;
    if (n >= 0xffffffffULL) return fail("hx_edge_support: more than 2^32-1 edge-support records");
    int bits = 1;
    while (bits < 32 && (1ull << bits) < 2ull * std::max<uint32_t>(1, c->n_contigs)) bits++;
    auto& E = c->sc_edges;
    c->ws.reset(s);
    HIPCHK(E.perm.reserve(n)); HIPCHK(E.perm_tmp.reserve(n)); HIPCHK(E.flag.reserve(n)); HIPCHK(E.key_tmp.reserve(n)); HIPCHK(E.fscan.reserve(n + 1));
    HIPCHK(c->rec.reserve(n));
    c->tick();
    hxk::iota_u32(E.perm.p, n, s);
    // the keys are sorted in the copy: rec_un stays the record set as it was emitted or imported, for a later hx_edge_records_export
    if (n) HIPCHK(hipMemcpyAsync(c->rec.key.p, c->rec_un.key.p, n * 8, hipMemcpyDeviceToDevice, s));
    hxk::radix_sort_pairs(c->rec.key.p, E.perm.p, E.key_tmp.p, E.perm_tmp.p, n, bits, bits, s, c->ws);
    hxk::edge_gather(c->rec_un.view(), E.perm.p, n, c->rec.view(), s);
    hxk::segment_flags(c->rec.key.p, n, E.flag.p, s);
    hxk::exclusive_scan_u32(E.flag.p, E.fscan.p, n, s, c->ws);
    if (ws_ok(c, "hx_edge_support")) return -1;
    uint64_t ne = 0;
    HIPCHK(hipMemcpyAsync(&ne, E.fscan.p + n, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(c->edge_key.reserve(ne)); HIPCHK(c->edge_off.reserve(ne + 1));
    if (n == 0) HIPCHK(hipMemsetAsync(c->edge_off.p, 0, 8, s));
    hxk::segment_scatter(c->rec.key.p, E.fscan.p, n, c->edge_key.p, c->edge_off.p, s);
    c->tock(1);
    HIPCHK(hipGetLastError());
    memset(out, 0, sizeof(*out));
    c->n_rec = out->n_rec = n; c->n_edge = out->n_edge = ne;
    bool ok = fetch(out->edge_key, c->edge_key.p, ne) && fetch(out->edge_off, c->edge_off.p, ne + 1);
    if (ok) {   // the host keeps the edges too, for hx_edge_coords
        c->h_edge_key.assign(out->edge_key, out->edge_key + ne); c->h_edge_off.assign(out->edge_off, out->edge_off + ne + 1); c->have_edges = true; c->have_coords = false;
        ok = c->rec.download(out, n) && c->rec.head.download(&out->head, n) && c->rec.tail.download(&out->tail, n);
    }
    return downloaded(ok, c, out, hx_free_edges, "hx_edge_support");
}

extern "C" int hx_edge_support(hx_ctx* c, const hx_params* prm, hx_edges_out* out) {
    memset(out, 0, sizeof(*out));
    uint64_t n = 0;
    return hx_edge_emit(c, prm, &n) ? -1 : finish_edges(c, n, out);
}

extern "C" uint32_t hx_edge_records_bytes(void) { return hxk::EDGE_REC_WORDS * 4; }

extern "C" int hx_edge_records_export(hx_ctx* c, void* dst, uint64_t cap) {
    if (cap < c->n_rec_un) return fail("hx_edge_records_export: destination too small");
    HIPCHK(hipSetDevice(c->device));
    hxk::edge_pack(c->rec_un.view(), c->n_rec_un, (uint32_t*)dst, c->stream);
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int hx_edge_records_import(hx_ctx* c, const void* src, uint64_t n, hx_edges_out* out) {
    memset(out, 0, sizeof(*out));
    if (n & 1) return fail("hx_edge_records_import: records come in (forward, twin) pairs, the count must be even");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(c->rec_un.reserve(n));
    hxk::edge_unpack((const uint32_t*)src, n, c->rec_un.view(), c->stream);
    c->n_rec_un = n;
    return finish_edges(c, n, out);
}

extern "C" void hx_free_edges(hx_ctx*, hx_edges_out* o) {
    RecCols::free_host(o); DevSideBuf::free_host(&o->head); DevSideBuf::free_host(&o->tail); free(o->edge_key); free(o->edge_off); memset(o, 0, sizeof(*o));
}

// ================================================================================================ K5
extern "C" int hx_edge_coords(hx_ctx* c, uint32_t n_sel, const uint32_t* sel, hx_coords_out* out) {
    memset(out, 0, sizeof(*out));
    if (!c->have_edges) return fail("hx_edge_coords: hx_edge_support has not run");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    std::vector<uint64_t> cap_off((size_t)n_sel + 1, 0);
    for (uint32_t i = 0; i < n_sel; i++) {
        if (sel[i] >= c->n_edge) return fail("hx_edge_coords: edge index out of range");
        uint64_t key = c->h_edge_key[sel[i]], n = c->h_edge_off[sel[i] + 1] - c->h_edge_off[sel[i]];
        bool hairpin = (((uint32_t)key) ^ 1u) == (uint32_t)(key >> 32);
        cap_off[i + 1] = cap_off[i] + (hairpin ? 2 * n : n);
    }
    const uint64_t cap = cap_off[n_sel];
    auto& K = c->sc_coords; auto& R = c->coords;   // the scratch, the results
    c->ws.reset(s);
    HIPCHK(K.reserve(n_sel, cap));
    HIPCHK(R.edge.reserve(n_sel));
    if (n_sel) HIPCHK(hipMemcpyAsync(K.sel.p, sel, (size_t)n_sel * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(K.cap.p, cap_off.data(), ((size_t)n_sel + 1) * 8, hipMemcpyHostToDevice, s));
    hxk::CoordsScratch sc{}; sc.beg1 = K.b1.p; sc.end1 = K.e1.p; sc.beg2 = K.b2.p; sc.end2 = K.e2.p; sc.cur = K.cur.p; sc.best_list = K.best_list.p;
    c->tick();
    hxk::edge_coords(c->rec.view(), c->edge_key.p, c->edge_off.p, c->hits.cg_ops.p, c->clen.p, c->rlen.p, n_sel, K.sel.p, K.cap.p, sc,
                     R.edge.head_end.p, R.edge.tail_beg.p, K.nsupp.p, K.t_lr.p, K.t_sp.p, K.t_ep.p, c->opt.coords_lds_supp, s);
    hxk::exclusive_scan_u32(K.nsupp.p, K.out_off.p, n_sel, s, c->ws);
    if (ws_ok(c, "hx_edge_coords")) return -1;
    uint64_t tot = 0;
    HIPCHK(hipMemcpyAsync(&tot, K.out_off.p + n_sel, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(R.supp.reserve(tot));
    hxk::coords_compact(K.cap.p, K.out_off.p, n_sel, K.t_lr.p, K.t_sp.p, K.t_ep.p, R.supp.supp_lr.p, R.supp.spos.p, R.supp.epos.p, s);
    c->tock(2);
    HIPCHK(hipGetLastError());
    R.n_sel = out->n_edge = n_sel;
    bool ok = fetch(out->supp_off, K.out_off.p, (size_t)n_sel + 1) && R.supp.download(out, tot);
    if (ok) { R.keep(out, tot); c->have_coords = true; ok = R.edge.download(out, n_sel); }   // (the host keeps the supports too, for hx_poa_batch)
    return downloaded(ok, c, out, hx_free_coords, "hx_edge_coords");
}

extern "C" void hx_free_coords(hx_ctx*, hx_coords_out* o) { CoordEdgeCols::free_host(o); CoordSuppCols::free_host(o); free(o->supp_off); memset(o, 0, sizeof(*o)); }

// ================================================================================================ misc
extern "C" void hx_timing_reset(hx_ctx* c) { for (int i = 0; i < 4; i++) { c->tm.ms[i] = 0; c->tm.launches[i] = 0; } }
extern "C" void hx_timing_get(hx_ctx* c, double* ms, uint64_t* launches) { for (int i = 0; i < 4; i++) { ms[i] = c->tm.ms[i]; launches[i] = c->tm.launches[i]; } }

static int be_chain(void* p, const hx_params* a, hx_chain_out* o) { return hx_chain_reads((hx_ctx*)p, a, o); }
static int be_edges(void* p, const hx_params* a, hx_edges_out* o) { return hx_edge_support((hx_ctx*)p, a, o); }
static int be_coords(void* p, uint32_t n, const uint32_t* s, hx_coords_out* o) { return hx_edge_coords((hx_ctx*)p, n, s, o); }
static int be_poa(void* p, const hx_poa_params* a, hx_cns_out* o) { return hx_poa_batch((hx_ctx*)p, a, o); }
static void be_fc(void* p, hx_chain_out* o) { hx_free_chain((hx_ctx*)p, o); }
static void be_fe(void* p, hx_edges_out* o) { hx_free_edges((hx_ctx*)p, o); }
static void be_fk(void* p, hx_coords_out* o) { hx_free_coords((hx_ctx*)p, o); }
static void be_fn(void* p, hx_cns_out* o) { hx_free_cns((hx_ctx*)p, o); }

extern "C" void hx_backend_fill(hx_ctx* c, void* table) {
    hx_backend* b = (hx_backend*)table;
    b->ctx = c; b->chain_reads = be_chain; b->edge_support = be_edges; b->edge_coords = be_coords; b->poa_batch = be_poa;
    b->free_chain = be_fc; b->free_edges = be_fe; b->free_coords = be_fk; b->free_cns = be_fn; b->last_error = hx_last_error;
}
