// hx_group.hip - the in-process multi-GPU group of the C-ABI: one context per rank, the exchange of the edge-support records.
// What asm_calc_edge_coordinates_MT / asm_cal_cns_seq_MT (Assemble.cpp:453-477, :580-605; called from main.cpp:203-208) are to the reference -
// a fan-out of the per-read / per-edge work over the threads of ONE process - this is to the GPUs of one node: a group of contexts (one per
// device, one host thread each) with one RCCL communicator each (ncclCommInitAll), and ONE collective on the data path: the all-gather of
// the packed edge-support records between the chain stage and the key sort (hx_edge_merge). librccl is looked up at run time (it is half a
// gigabyte: a single-GPU run never maps it). HASLR_GROUP_TRANSPORT=host stages the exchange through host memory instead, which also allows
// several ranks on one device (rehearsal of the multi-GPU logic on a one-GPU box).
#include "hx_internal.h"

#include <dlfcn.h>
#include <rccl/rccl.h>

#include <atomic>
#include <condition_variable>
#include <thread>
#include <memory>
#include <mutex>

using namespace hxi;

namespace {
struct GroupRank { hx_group* g; int rank; };
}
struct hx_group {
    int n = 0;
    std::vector<hx_ctx*> ctx;
    std::vector<int> dev;
    std::vector<GroupRank> self;             // opaque `ctx` of the ranks' backend tables
    bool rccl = false;
    void* lib = nullptr;
    std::vector<ncclComm_t> comm;
    ncclResult_t (*p_init_all)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*p_all_gather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*p_destroy)(ncclComm_t) = nullptr;
    ncclResult_t (*p_abort)(ncclComm_t) = nullptr;
    ncclResult_t (*p_count)(const ncclComm_t, int*) = nullptr;
    const char* (*p_errstr)(ncclResult_t) = nullptr;
    std::atomic<int> abort_flag{0};               // a rank failed inside the collective: the ranks still waiting on their streams abort their communicators
    std::atomic<bool> broken{false};              // ... after which the group refuses further exchanges (written and read by the rank threads)
    double timeout_s = 300;                       // bound of the wait for the collective (hx_group_set_timeout)
    std::atomic<int> fault_rank{-1};              // (testing, hx_group_inject_fault: this rank's all-gather "returns an error")
    // rendezvous of the rank threads: everybody arrives with a status, everybody leaves with the worst one (so that no rank enters a
    // collective the others will never join)
    std::mutex mu;
    std::condition_variable cv;
    int arrived = 0, worst = 0, agreed = 0;
    uint64_t generation = 0;
    std::vector<uint64_t> counts;
    std::vector<std::unique_ptr<DV<uint8_t>>> sendb, recvb, merged;
    std::vector<std::vector<uint8_t>> stage;      // host transport
    uint64_t last_bytes = 0;
    double last_ms = 0;

    int rendezvous(int status) {
        std::unique_lock<std::mutex> lk(mu);
        const uint64_t gen = generation;
        worst = std::max(worst, status);
        if (++arrived == n) { agreed = worst; worst = 0; arrived = 0; generation++; cv.notify_all(); return agreed; }
        cv.wait(lk, [&] { return generation != gen; });
        return agreed;
    }
};

extern "C" int hx_group_create(int n, const int* devices, const char* transport, hx_group** out) {
    *out = nullptr;
    int ndev = 0;
    if (n < 1) return fail("hx_group_create: at least one rank");
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail("hx_group_create: no HIP device available (no CPU fallback)");
    std::unique_ptr<hx_group> g(new hx_group);
    g->n = n;
    const char* tr = transport && *transport ? transport : nullptr;   // (the applications pass what their HASLR_GROUP_TRANSPORT says: the library reads no environment)
    bool distinct = true;
    for (int r = 0; r < n; r++) {
        const int d = devices ? devices[r] : (tr && !strcmp(tr, "host") ? r % ndev : r);
        if (d < 0 || d >= ndev) return fail("hx_group_create: rank " + std::to_string(r) + " asks for device " + std::to_string(d) + " of " + std::to_string(ndev) +
                                            " (one device per rank over RCCL; transport \"host\" lets ranks share devices)");
        for (int q : g->dev) distinct = distinct && q != d;
        g->dev.push_back(d);
    }
    if (tr && strcmp(tr, "host") && strcmp(tr, "rccl")) return fail("hx_group_create: transport must be \"rccl\" or \"host\" (or NULL: automatic)");
    g->rccl = tr ? !strcmp(tr, "rccl") : distinct;
    if (g->rccl && !distinct) return fail("hx_group_create: RCCL needs one device per rank");
    g->ctx.assign(n, nullptr);
    for (int r = 0; r < n; r++)
        if (hx_ctx_create(g->dev[r], nullptr, &g->ctx[r]) != 0) { for (hx_ctx* c : g->ctx) hx_ctx_destroy(c); return -1; }
    g->self.resize(n);
    for (int r = 0; r < n; r++) g->self[r] = GroupRank{g.get(), r};
    g->counts.assign(n, 0); g->stage.resize(n);
    for (int r = 0; r < n; r++) { g->sendb.emplace_back(new DV<uint8_t>); g->recvb.emplace_back(new DV<uint8_t>); g->merged.emplace_back(new DV<uint8_t>); }
    if (g->rccl) {
        g->lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!g->lib) g->lib = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
        if (!g->lib) g->lib = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!g->lib) { const std::string m = std::string("hx_group_create: cannot load librccl: ") + dlerror(); for (hx_ctx* c : g->ctx) hx_ctx_destroy(c); return fail(m); }
        g->p_init_all = (decltype(g->p_init_all))dlsym(g->lib, "ncclCommInitAll");
        g->p_all_gather = (decltype(g->p_all_gather))dlsym(g->lib, "ncclAllGather");
        g->p_destroy = (decltype(g->p_destroy))dlsym(g->lib, "ncclCommDestroy");
        g->p_errstr = (decltype(g->p_errstr))dlsym(g->lib, "ncclGetErrorString");
        g->p_abort = (decltype(g->p_abort))dlsym(g->lib, "ncclCommAbort");
        g->p_count = (decltype(g->p_count))dlsym(g->lib, "ncclCommCount");
        if (!g->p_init_all || !g->p_all_gather || !g->p_destroy || !g->p_errstr) { for (hx_ctx* c : g->ctx) hx_ctx_destroy(c); return fail("hx_group_create: librccl lacks ncclCommInitAll / ncclAllGather"); }
        g->comm.assign(n, nullptr);
        const ncclResult_t rc = g->p_init_all(g->comm.data(), n, g->dev.data());
        if (rc != ncclSuccess) { const std::string m = std::string("ncclCommInitAll: ") + g->p_errstr(rc); for (hx_ctx* c : g->ctx) hx_ctx_destroy(c); return fail(m); }
    }
    *out = g.release();
    return 0;
}

extern "C" void hx_group_destroy(hx_group* g) {
    if (!g) return;
    // (a group whose collective failed has had its communicators aborted by their own ranks - hx_edge_merge - and whatever is left of it is aborted too:
    // ncclCommDestroy on a communicator whose peers are gone may wait for them)
    if (g->rccl) for (int r = 0; r < g->n; r++) if (g->comm[r]) { (void)hipSetDevice(g->dev[r]); if (g->broken.load() && g->p_abort) (void)g->p_abort(g->comm[r]); else (void)g->p_destroy(g->comm[r]); g->comm[r] = nullptr; }
    for (int r = 0; r < g->n; r++) { (void)hipSetDevice(g->dev[r]); g->sendb[r]->release(); g->recvb[r]->release(); g->merged[r]->release(); }
    for (hx_ctx* c : g->ctx) hx_ctx_destroy(c);
    // (librccl stays mapped: unloading it while the HIP runtime is alive buys nothing)
    delete g;
}
extern "C" int hx_group_size(const hx_group* g) { return g->n; }
extern "C" void hx_group_inject_fault(hx_group* g, int rank) { g->fault_rank.store(rank); }
extern "C" void hx_group_set_timeout(hx_group* g, double seconds) { g->timeout_s = seconds > 0 ? seconds : 300; }
extern "C" hx_ctx* hx_group_ctx(hx_group* g, int rank) { return rank >= 0 && rank < g->n ? g->ctx[rank] : nullptr; }
extern "C" const char* hx_group_transport(const hx_group* g) { return g->rccl ? "rccl" : "host"; }
extern "C" int hx_group_rccl_ranks(const hx_group* g, int* out) {   // what ncclCommCount says on every rank's communicator (0 for every rank: host transport)
    for (int r = 0; r < g->n; r++) {
        out[r] = 0;
        if (g->rccl && g->p_count && g->comm[r] && g->p_count(g->comm[r], &out[r]) != ncclSuccess) out[r] = -1;
    }
    return g->rccl ? 1 : 0;
}
extern "C" void hx_group_exchange_stats(const hx_group* g, uint64_t* bytes, double* ms) { *bytes = g->last_bytes; *ms = g->last_ms; }

extern "C" int hx_edge_merge(hx_group* g, int rank, const hx_params* prm, hx_edges_out* out) {
    memset(out, 0, sizeof(*out));
    if (rank < 0 || rank >= g->n) return fail("hx_edge_merge: rank out of range");
    if (g->broken.load()) return fail("hx_edge_merge: the group's collective failed earlier (communicators aborted): create a new group");
    hx_ctx* c = g->ctx[rank];
    const uint32_t rb = hx_edge_records_bytes();
    uint64_t n = 0;
    int rc = hx_edge_emit(c, prm, &n);
    g->counts[rank] = rc == 0 ? n : 0;
    std::string own_err = rc ? g_err : std::string();
    if (g->rendezvous(rc != 0)) return fail(rc ? own_err : "hx_edge_merge: another rank failed to emit its edge records");
    uint64_t cap_rec = 1, total = 0;
    bool equal = true;
    for (int r = 0; r < g->n; r++) { cap_rec = std::max(cap_rec, g->counts[r]); total += g->counts[r]; equal = equal && g->counts[r] == g->counts[0]; }
    const uint64_t cap = cap_rec * rb;
    DV<uint8_t>&sb = *g->sendb[rank], &rv = *g->recvb[rank];
    rc = 0;
    if (hipSetDevice(c->device) != hipSuccess || sb.reserve(cap) != hipSuccess || rv.reserve(cap * g->n) != hipSuccess) { rc = -1; own_err = "hx_edge_merge: out of device memory for the exchange buffers"; }
    if (!rc && hx_edge_records_export(c, sb.p, cap_rec) != 0) { rc = -1; own_err = g_err; }
    if (g->rendezvous(rc != 0)) return fail(rc ? own_err : "hx_edge_merge: another rank failed before the exchange");
    const auto t0 = std::chrono::steady_clock::now();
    if (g->rccl) {
        // THE collective of the path: every rank contributes its packed records padded to the largest shard (counts travelled through the
        // process's memory above: the ranks are threads of one process)
        // A failure INSIDE the collective must not leave the other ranks parked on their streams: the wait is a bounded poll of the stream; a rank
        // whose ncclAllGather returns an error (or whose stream faults, or whose wait runs out) raises the group's abort flag, every rank that sees it
        // aborts its communicator (ncclCommAbort ends the kernels of the collective on its device) and all of them meet at the rendezvous below with
        // the failure. The group is unusable afterwards (hx_edge_merge refuses).
        int want = rank;
        const bool injected = g->fault_rank.compare_exchange_strong(want, -1);   // (one shot, taken by the rank it names)
        const ncclResult_t nr = injected ? ncclInternalError : g->p_all_gather(sb.p, rv.p, cap, ncclUint8, g->comm[rank], c->stream);
        if (nr != ncclSuccess) { rc = -1; own_err = std::string("ncclAllGather: ") + g->p_errstr(nr); g->abort_flag.store(1); }
        else {
            const auto deadline = std::chrono::steady_clock::now() + std::chrono::duration<double>(g->timeout_s);
            for (;;) {
                const hipError_t q = hipStreamQuery(c->stream);
                if (q == hipSuccess) break;
                if (q != hipErrorNotReady) { rc = -1; own_err = std::string("hx_edge_merge: all-gather failed on the stream: ") + hipGetErrorString(q); g->abort_flag.store(1); break; }
                const bool late = std::chrono::steady_clock::now() > deadline;
                if (g->abort_flag.load() || late) {
                    rc = -1; own_err = late ? "hx_edge_merge: the all-gather did not finish within " + std::to_string((int)g->timeout_s) + " s (hx_group_set_timeout)" : "hx_edge_merge: another rank failed inside the all-gather";
                    g->abort_flag.store(1);
                    if (g->p_abort && g->comm[rank]) { (void)g->p_abort(g->comm[rank]); g->comm[rank] = nullptr; }
                    (void)hipStreamSynchronize(c->stream);
                    break;
                }
                std::this_thread::sleep_for(std::chrono::microseconds(50));
            }
        }
        } else {
        g->stage[rank].resize(cap);
        if (hipMemcpy(g->stage[rank].data(), sb.p, cap, hipMemcpyDeviceToHost) != hipSuccess) { rc = -1; own_err = "hx_edge_merge: copy to the host staging buffer failed"; }
        if (g->rendezvous(rc != 0)) return fail(rc ? own_err : "hx_edge_merge: another rank failed in the exchange");
        for (int r = 0; r < g->n && !rc; r++)
            if (hipMemcpy(rv.p + (uint64_t)r * cap, g->stage[r].data(), cap, hipMemcpyHostToDevice) != hipSuccess) { rc = -1; own_err = "hx_edge_merge: copy from the host staging buffer failed"; }
    }
    if (g->rendezvous(rc != 0)) {
        if (g->rccl) {
            // EVERY rank leaves a failed collective with its own communicator aborted - the rank whose call returned the error and the ranks whose part
            // had already completed included (their peers are gone: ncclCommDestroy on such a communicator may wait for them) - and the group refuses
            // further exchanges
            g->broken.store(true);
            if (g->p_abort && g->comm[rank]) { (void)g->p_abort(g->comm[rank]); g->comm[rank] = nullptr; }
            (void)hipStreamSynchronize(c->stream);
        }
        return fail(rc ? own_err : "hx_edge_merge: another rank failed in the exchange");
    }
    if (rank == 0) { g->last_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); g->last_bytes = total * rb; }
    const uint8_t* src = rv.p;
    if (!equal) {   // cut the padding out: rank order = ascending read ids, which the stable key sort relies on
        DV<uint8_t>& mg = *g->merged[rank];
        if (mg.reserve(std::max<uint64_t>(1, total * rb)) != hipSuccess) { rc = -1; own_err = "hx_edge_merge: out of device memory for the merged records"; }
        uint64_t off = 0;
        for (int r = 0; r < g->n && !rc; r++) {
            if (g->counts[r] && hipMemcpyAsync(mg.p + off, rv.p + (uint64_t)r * cap, g->counts[r] * rb, hipMemcpyDeviceToDevice, c->stream) != hipSuccess) { rc = -1; own_err = "hx_edge_merge: compaction failed"; }
            off += g->counts[r] * rb;
        }
        if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) { rc = -1; own_err = "hx_edge_merge: compaction failed"; }
        src = mg.p;
    }
    if (!rc && hx_edge_records_import(c, src, total, out) != 0) { rc = -1; own_err = g_err; }
    if (g->rendezvous(rc != 0)) { if (!rc) hx_free_edges(c, out); return fail(rc ? own_err : "hx_edge_merge: another rank failed to import the merged records"); }
    return 0;
}

static int gb_chain(void* p, const hx_params* a, hx_chain_out* o) { GroupRank* q = (GroupRank*)p; return hx_chain_reads(q->g->ctx[q->rank], a, o); }
static int gb_edges(void* p, const hx_params* a, hx_edges_out* o) { GroupRank* q = (GroupRank*)p; return hx_edge_merge(q->g, q->rank, a, o); }
static int gb_coords(void* p, uint32_t n, const uint32_t* s, hx_coords_out* o) { GroupRank* q = (GroupRank*)p; return hx_edge_coords(q->g->ctx[q->rank], n, s, o); }
static int gb_poa(void* p, const hx_poa_params* a, hx_cns_out* o) { GroupRank* q = (GroupRank*)p; return hx_poa_batch(q->g->ctx[q->rank], a, o); }
static void gb_fc(void* p, hx_chain_out* o) { GroupRank* q = (GroupRank*)p; hx_free_chain(q->g->ctx[q->rank], o); }
static void gb_fe(void* p, hx_edges_out* o) { GroupRank* q = (GroupRank*)p; hx_free_edges(q->g->ctx[q->rank], o); }
static void gb_fk(void* p, hx_coords_out* o) { GroupRank* q = (GroupRank*)p; hx_free_coords(q->g->ctx[q->rank], o); }
static void gb_fn(void* p, hx_cns_out* o) { GroupRank* q = (GroupRank*)p; hx_free_cns(q->g->ctx[q->rank], o); }

extern "C" int hx_group_backend_fill(hx_group* g, int rank, void* table) {
    if (rank < 0 || rank >= g->n) return fail("hx_group_backend_fill: rank out of range");
    hx_backend* b = (hx_backend*)table;
    b->ctx = &g->self[rank]; b->chain_reads = gb_chain; b->edge_support = gb_edges; b->edge_coords = gb_coords; b->poa_batch = gb_poa;
    b->free_chain = gb_fc; b->free_edges = gb_fe; b->free_coords = gb_fk; b->free_cns = gb_fn; b->last_error = hx_last_error;
    return 0;
}
