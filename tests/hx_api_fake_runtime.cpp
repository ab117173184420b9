// hx_api_fake_runtime.cpp - everything hx_api.hip (compiled host-only) leaves undefined, so that tests/hx_api_trace_driver.cpp runs the chain,
// edge-support and coordinate operators without a GPU and without a HIP runtime in the link (tests/test_hx_api_trace.py):
//   the HIP calls    hipMalloc is malloc of exactly the bytes asked for (filled with 0xa5), so that a host sanitizer sees every overrun; copies
//                    are memcpy, memsets memset, streams and events tokens. Everything is recorded. A device pointer is shown as buffer index +
//                    byte offset; a buffer gets its index when it is first named by anything but its allocation (buffers first named by
//                    the same line: in the order hipcc's clang evaluates call arguments, left to right). What lies between two stream
//                    operations (allocations, frees, synchronous copies, creations) is printed sorted, equal lines once: its order is free.
//   the launchers    (hxk::, kernels/kernels.h) do the least the host needs to go on. exclusive_scan_u32, iota_u32, radix_sort_pairs,
//                    edge_gather, segment_flags, segment_scatter and coords_compact do what they say; chain_reads, edge_count and edge_coords
//                    write small counts by a fixed formula of the index; edge_emit writes keys that make a few edges, one in five a hairpin.
//                    Every other output column is filled, over its whole length, with (column tag << high bits) | index - the tags are the
//                    enum below - so that a column that ends in the wrong out-field shows in the driver's text.
//   hx_poa_batch, hx_free_cns   (hx_poa.hip) are not part of this test.
#include "hx_api_fake.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "../include/haslr_hip.h"
#include "kernels/kernels.h"

namespace {

struct Buf { char* p; size_t bytes; long index; };
std::vector<Buf> g_bufs;
std::vector<std::string> g_between;   // what was recorded since the last stream operation
long g_next_index = 0, g_next_token = 0;
int g_fail_in = 0;

std::string fmt(const char* f, ...) {
    va_list ap, aq;
    va_start(ap, f);
    va_copy(aq, ap);
    std::string b((size_t)vsnprintf(nullptr, 0, f, ap) + 1, '\0');
    vsnprintf(&b[0], b.size(), f, aq);
    va_end(ap);
    va_end(aq);
    b.pop_back();
    return b;
}
Buf* find(const void* q) {
    const char* p = (const char*)q;
    for (Buf& b : g_bufs) if (p >= b.p && p < b.p + b.bytes) return &b;
    for (Buf& b : g_bufs) if (p == b.p + b.bytes) return &b;
    return nullptr;
}
void between(const std::string& s) { g_between.push_back(s); }
void stream_op(const std::string& s) { fake::flush(); printf("t %s\n", s.c_str()); }
std::string tok(const void* p) { return p ? fmt("#%ld", (long)((uintptr_t)p >> 4)) : std::string("null"); }
void* new_token() { return (void*)(uintptr_t)(++g_next_token << 4); }
#define W(p) fake::where(p).c_str()

// the column tags
enum Tag : unsigned {
    T_CLS = 1,
    S_HIT = 0x10, S_QS, S_QE, S_TS, S_TE, S_NM, S_NB, S_SKF, S_SKB, S_CB, S_CE, S_DP, S_FROM, S_CMP,                  // hxk::ChainScratch
    C_HIT = 0x30, C_QS, C_QE, C_TS, C_TE, C_NM, C_NB, C_SKF, C_SKB, C_CB, C_CE, C_CMP,                                // hxk::ChainFinal
    R_LR = 0x50, R_CH, R_CT, R_HEAD = 0x60, R_TAIL = 0x70,                                                            // hxk::EdgeRecs as emitted (a side: + the member's place in DevSide)
    U_LR = 0x80, U_CH, U_CT, U_HEAD = 0x90, U_TAIL = 0xa0, P_WORD = 0xb0,                                            // ... as unpacked; the packed words
    K_B1 = 0xc0, K_E1, K_B2, K_E2, K_CUR, K_BEST, K_HEAD_END, K_TAIL_BEG, K_LR, K_SP, K_EP,                           // the coordinate scratch and results
    X_TMP = 0xe0,
};
template <class T> void fill(T* p, uint64_t n, unsigned tag) {
    for (uint64_t i = 0; i < n; i++)
        p[i] = sizeof(T) == 1 ? (T)((((tag >> 4 ^ tag) & 7) << 5) | (i & 31)) : (T)(((T)tag << (8 * sizeof(T) - 8)) | (T)(i & 0xffffff));
}
void fill_side(const DevSide& s, uint64_t n, unsigned tag) {
    fill(s.q_start, n, tag + 0); fill(s.q_end, n, tag + 1); fill(s.t_start, n, tag + 2); fill(s.t_end, n, tag + 3); fill(s.is_rev, n, tag + 4);
    fill(s.cg_begin, n, tag + 5); fill(s.cg_end, n, tag + 6); fill(s.cg_skip_front, n, tag + 7); fill(s.cg_skip_back, n, tag + 8);
}
// the members of a kernel's struct, in the struct's order; buffers named one after the other, as by the call that first names them, are "b4..b9"
std::string list(std::initializer_list<const void*> ps) {
    std::vector<std::string> w;
    for (const void* p : ps) w.push_back(fake::where(p));
    std::string out = "{";
    for (size_t i = 0, j; i < w.size(); i = j) {
        for (j = i + 1; j < w.size() && w[j] == fmt("b%ld", atol(w[i].c_str() + 1) + (long)(j - i)) && w[i][0] == 'b' && w[i].find('+') == std::string::npos; j++) {}
        if (j - i < 3) j = i + 1;
        out += (i ? " " : "") + w[i] + (j - i > 1 ? ".." + w[j - 1] : "");
    }
    return out + "}";
}
std::string side(const DevSide& s) { return list({s.q_start, s.q_end, s.t_start, s.t_end, s.is_rev, s.cg_begin, s.cg_end, s.cg_skip_front, s.cg_skip_back}); }
std::string recs(const hxk::EdgeRecs& r) { return list({r.key, r.lr, r.cmp_head, r.cmp_tail}) + " head " + side(r.head) + " tail " + side(r.tail); }
std::string hits(const DevHits& h) {
    return fmt("%llu ", (unsigned long long)h.n) + list({h.q_id, h.q_start, h.q_end, h.t_id, h.t_len, h.t_start, h.t_end, h.n_match, h.n_block, h.is_rev, h.mapq, h.cg_off, h.cg_ops});
}
std::string fin(const hxk::ChainFinal& c) { return list({c.hit, c.qs, c.qe, c.ts, c.te, c.nm, c.nb, c.skf, c.skb, c.cb, c.ce, c.cmp_aln}); }
std::string scr(const hxk::ChainScratch& c) { return list({c.hit, c.qs, c.qe, c.ts, c.te, c.nm, c.nb, c.skf, c.skb, c.cb, c.ce, c.dp, c.from, c.cmp, c.n_aln, c.n_cmp}); }
template <class T> void gather(T* out, const T* in, const uint32_t* perm, uint64_t n) { for (uint64_t i = 0; i < n; i++) out[i] = in[perm[i]]; }
void gather_side(const DevSide& o, const DevSide& i, const uint32_t* perm, uint64_t n) {
    gather(o.q_start, i.q_start, perm, n); gather(o.q_end, i.q_end, perm, n); gather(o.t_start, i.t_start, perm, n); gather(o.t_end, i.t_end, perm, n); gather(o.is_rev, i.is_rev, perm, n);
    gather(o.cg_begin, i.cg_begin, perm, n); gather(o.cg_end, i.cg_end, perm, n); gather(o.cg_skip_front, i.cg_skip_front, perm, n); gather(o.cg_skip_back, i.cg_skip_back, perm, n);
}

}  // namespace

namespace fake {
void flush() {
    std::sort(g_between.begin(), g_between.end());
    for (size_t i = 0, j; i < g_between.size(); i = j) {   // (equal lines once, with their number)
        for (j = i + 1; j < g_between.size() && g_between[j] == g_between[i]; j++) {}
        if (j - i > 1) printf("t   %s x %zu\n", g_between[i].c_str(), j - i);
        else printf("t   %s\n", g_between[i].c_str());
    }
    g_between.clear();
}
void say(const std::string& line) { flush(); printf("%s\n", line.c_str()); }
void fail_memcpy(int k) { g_fail_in = k; }
std::string where(const void* p) {
    if (!p) return "null";
    Buf* b = find(p);
    if (!b) return "host";
    if (b->index < 0) b->index = g_next_index++;
    return p == b->p ? fmt("b%ld", b->index) : fmt("b%ld+%zu", b->index, (size_t)((const char*)p - b->p));
}
}  // namespace fake

// ------------------------------------------------------------------------------------------------ the HIP calls
extern "C" {
hipError_t hipGetDeviceCount(int* n) { *n = 1; return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "fake error"; }
hipError_t hipDeviceGetStreamPriorityRange(int* lo, int* hi) { *lo = 0; *hi = -1; return hipSuccess; }
hipError_t hipStreamCreate(hipStream_t* s) { *s = (hipStream_t)new_token(); between("stream_create"); return hipSuccess; }
hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned int, int) { *s = (hipStream_t)new_token(); return hipSuccess; }   // (the process's pool: made once, not per context)
hipError_t hipStreamDestroy(hipStream_t) { between("stream_destroy"); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t s) { stream_op("stream_synchronize " + tok(s)); return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t* e) { *e = (hipEvent_t)new_token(); between("event_create"); return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { *e = (hipEvent_t)new_token(); between("event_create"); return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t) { between("event_destroy"); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { stream_op("event_record " + tok(e) + " " + tok(s)); return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t e) { stream_op("event_synchronize " + tok(e)); return hipSuccess; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) { *ms = 0; return hipSuccess; }
hipError_t hipHostMalloc(void** p, size_t n, unsigned int) { *p = calloc(1, n); between(fmt("host_alloc %zu", n)); return hipSuccess; }
hipError_t hipHostFree(void* p) { free(p); between("host_free"); return hipSuccess; }
hipError_t hipMalloc(void** p, size_t n) {
    *p = malloc(n);
    memset(*p, 0xa5, n);
    g_bufs.push_back(Buf{(char*)*p, n, -1});
    between(fmt("alloc %zu", n));
    return hipSuccess;
}
hipError_t hipFree(void* p) {
    if (!p) return hipSuccess;
    for (size_t i = 0; i < g_bufs.size(); i++)
        if (g_bufs[i].p == p) {
            between(g_bufs[i].index < 0 ? fmt("free (never named) %zu", g_bufs[i].bytes) : fmt("free b%ld %zu", g_bufs[i].index, g_bufs[i].bytes));
            g_bufs.erase(g_bufs.begin() + (long)i);
            free(p);
            return hipSuccess;
        }
    between("free of an unknown pointer");
    return hipErrorInvalidValue;
}
hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind) {
    if (g_fail_in && --g_fail_in == 0) { between(fmt("copy %s <- %s %zu FAILS", W(d), W(s), n)); return hipErrorUnknown; }
    between(fmt("copy %s <- %s %zu", W(d), W(s), n));
    memcpy(d, s, n);
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind, hipStream_t st) {
    stream_op(fmt("copy_async %s <- %s %zu %s", W(d), W(s), n, tok(st).c_str()));
    memcpy(d, s, n);
    return hipSuccess;
}
hipError_t hipMemsetAsync(void* d, int v, size_t n, hipStream_t st) {
    stream_op(fmt("memset_async %s %d %zu %s", W(d), v, n, tok(st).c_str()));
    memset(d, v, n);
    return hipSuccess;
}

int hx_poa_batch(hx_ctx*, const hx_poa_params*, hx_cns_out*) { return -1; }
void hx_free_cns(hx_ctx*, hx_cns_out*) {}
}

// ------------------------------------------------------------------------------------------------ the launchers
namespace hxk {

void* Workspace::take(size_t) { return nullptr; }
void Workspace::reset(hipStream_t s) { stream_op("ws_reset " + tok(s)); }
void Workspace::release() {}

void exclusive_scan_u32(const uint32_t* in, uint64_t* out, uint64_t n, hipStream_t s, Workspace&) {
    stream_op(fmt("exclusive_scan_u32 in %s out %s n %llu %s", W(in), W(out), (unsigned long long)n, tok(s).c_str()));
    uint64_t sum = 0;
    for (uint64_t i = 0; i < n; i++) { out[i] = sum; sum += in[i]; }
    out[n] = sum;
}
void radix_sort_pairs(uint64_t* key, uint32_t* val, uint64_t* key_tmp, uint32_t* val_tmp, uint64_t n, int bits_lo, int bits_hi, hipStream_t s, Workspace&) {
    stream_op(fmt("radix_sort_pairs key %s val %s key_tmp %s val_tmp %s n %llu bits %d %d %s", W(key), W(val), W(key_tmp), W(val_tmp), (unsigned long long)n, bits_lo, bits_hi, tok(s).c_str()));
    std::vector<uint32_t> at(n);
    for (uint64_t i = 0; i < n; i++) at[i] = (uint32_t)i;
    std::stable_sort(at.begin(), at.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
    for (uint64_t i = 0; i < n; i++) { key_tmp[i] = key[at[i]]; val_tmp[i] = val[at[i]]; }
    for (uint64_t i = 0; i < n; i++) { key[i] = key_tmp[i]; val[i] = val_tmp[i]; }
    fill(key_tmp, n, X_TMP); fill(val_tmp, n, X_TMP + 1);
}

void contig_class(const double* mean_kmer, uint32_t n, double thr_load, double thr_uniq, uint8_t* cls, hipStream_t s) {
    stream_op(fmt("contig_class mean_kmer %s n %u thr %.17g %.17g cls %s %s", W(mean_kmer), n, thr_load, thr_uniq, W(cls), tok(s).c_str()));
    fill(cls, n, T_CLS);
}
// read r keeps min(its hits, 1 + r % 3) alignments, all of them compact elements
void chain_reads(const DevHits& h, const uint64_t* rho, const uint8_t* cls, uint32_t n_contigs, uint32_t lr_begin, uint32_t lr_end, uint32_t min_aln_block, double min_aln_sim,
                 uint32_t min_mapq, const ChainScratch& sc, uint32_t* err, bool prefiltered, hipStream_t s) {
    stream_op(fmt("chain_reads hits %s rho %s cls %s n_contigs %u reads %u %u min %u %.17g %u scratch %s err %s prefiltered %d %s", hits(h).c_str(), W(rho), W(cls), n_contigs, lr_begin, lr_end,
                  min_aln_block, min_aln_sim, min_mapq, scr(sc).c_str(), W(err), (int)prefiltered, tok(s).c_str()));
    const uint64_t nraw = rho[lr_end] - rho[lr_begin];
    fill(sc.hit, nraw, S_HIT); fill(sc.qs, nraw, S_QS); fill(sc.qe, nraw, S_QE); fill(sc.ts, nraw, S_TS); fill(sc.te, nraw, S_TE); fill(sc.nm, nraw, S_NM); fill(sc.nb, nraw, S_NB);
    fill(sc.skf, nraw, S_SKF); fill(sc.skb, nraw, S_SKB); fill(sc.cb, nraw, S_CB); fill(sc.ce, nraw, S_CE); fill(sc.dp, nraw, S_DP); fill(sc.from, nraw, S_FROM); fill(sc.cmp, nraw, S_CMP);
    for (uint32_t r = lr_begin; r < lr_end; r++) {
        const uint64_t nh = rho[r + 1] - rho[r];
        sc.n_aln[r - lr_begin] = sc.n_cmp[r - lr_begin] = (uint32_t)std::min<uint64_t>(nh, 1 + r % 3);
    }
}
void chain_compact(const ChainScratch& sc, const uint64_t* rho, uint32_t lr_begin, uint32_t lr_end, const uint64_t* aln_off, const uint64_t* cmp_off, const ChainFinal& out, hipStream_t s) {
    stream_op(fmt("chain_compact scratch %s rho %s reads %u %u aln_off %s cmp_off %s out %s %s", scr(sc).c_str(), W(rho), lr_begin, lr_end, W(aln_off), W(cmp_off), fin(out).c_str(), tok(s).c_str()));
    const uint64_t na = aln_off[lr_end - lr_begin], nc = cmp_off[lr_end - lr_begin];
    fill(out.hit, na, C_HIT); fill(out.qs, na, C_QS); fill(out.qe, na, C_QE); fill(out.ts, na, C_TS); fill(out.te, na, C_TE); fill(out.nm, na, C_NM); fill(out.nb, na, C_NB);
    fill(out.skf, na, C_SKF); fill(out.skb, na, C_SKB); fill(out.cb, na, C_CB); fill(out.ce, na, C_CE); fill(out.cmp_aln, nc, C_CMP);
}

// a read of k compact elements has k - 1 pairs
void edge_count(const DevHits& h, const uint8_t* cls, const ChainFinal& c, const uint64_t* cmp_off, uint32_t lr_begin, uint32_t lr_end, uint32_t* n_pairs, hipStream_t s) {
    stream_op(fmt("edge_count hits %s cls %s chain %s cmp_off %s reads %u %u n_pairs %s %s", hits(h).c_str(), W(cls), fin(c).c_str(), W(cmp_off), lr_begin, lr_end, W(n_pairs), tok(s).c_str()));
    for (uint32_t r = 0; r < lr_end - lr_begin; r++) { const uint64_t k = cmp_off[r + 1] - cmp_off[r]; n_pairs[r] = k ? (uint32_t)(k - 1) : 0; }
}
// pair j: a forward record and its twin between two contig ends; every fifth pair is a hairpin (both records carry the same key)
void edge_emit(const DevHits& h, const uint8_t* cls, const ChainFinal& c, const uint64_t* cmp_off, uint32_t lr_begin, uint32_t lr_end, const uint64_t* pair_off, const EdgeRecs& out, hipStream_t s) {
    stream_op(fmt("edge_emit hits %s cls %s chain %s cmp_off %s reads %u %u pair_off %s out %s %s", hits(h).c_str(), W(cls), fin(c).c_str(), W(cmp_off), lr_begin, lr_end, W(pair_off),
                  recs(out).c_str(), tok(s).c_str()));
    const uint64_t np = pair_off[lr_end - lr_begin], ends = 6;   // (the driver's data sets have three contigs and more)
    for (uint64_t j = 0; j < np; j++) {
        const uint64_t a = (j * 5 + 1) % ends, b = j % 5 == 4 ? (a ^ 1) : (j * 3 + 2) % ends;
        out.key[2 * j] = a << 32 | b;
        out.key[2 * j + 1] = (b ^ 1) << 32 | (a ^ 1);
    }
    fill(out.lr, 2 * np, R_LR); fill(out.cmp_head, 2 * np, R_CH); fill(out.cmp_tail, 2 * np, R_CT);
    fill_side(out.head, 2 * np, R_HEAD); fill_side(out.tail, 2 * np, R_TAIL);
}
void edge_gather(const EdgeRecs& in, const uint32_t* perm, uint64_t n, const EdgeRecs& out, hipStream_t s) {
    stream_op(fmt("edge_gather in %s perm %s n %llu out %s %s", recs(in).c_str(), W(perm), (unsigned long long)n, recs(out).c_str(), tok(s).c_str()));
    gather(out.lr, in.lr, perm, n); gather(out.cmp_head, in.cmp_head, perm, n); gather(out.cmp_tail, in.cmp_tail, perm, n);   // (the keys were sorted in place)
    gather_side(out.head, in.head, perm, n); gather_side(out.tail, in.tail, perm, n);
}
void edge_pack(const EdgeRecs& r, uint64_t n, uint32_t* dst, hipStream_t s) {   // the keys travel, the rest is the packed words' own pattern
    stream_op(fmt("edge_pack recs %s n %llu dst %s %s", recs(r).c_str(), (unsigned long long)n, W(dst), tok(s).c_str()));
    fill(dst, n * EDGE_REC_WORDS, P_WORD);
    for (uint64_t i = 0; i < n; i++) memcpy(dst + i * EDGE_REC_WORDS, &r.key[i], 8);
}
void edge_unpack(const uint32_t* src, uint64_t n, const EdgeRecs& r, hipStream_t s) {
    stream_op(fmt("edge_unpack src %s n %llu recs %s %s", W(src), (unsigned long long)n, recs(r).c_str(), tok(s).c_str()));
    for (uint64_t i = 0; i < n; i++) memcpy(&r.key[i], src + i * EDGE_REC_WORDS, 8);
    fill(r.lr, n, U_LR); fill(r.cmp_head, n, U_CH); fill(r.cmp_tail, n, U_CT);
    fill_side(r.head, n, U_HEAD); fill_side(r.tail, n, U_TAIL);
}
void iota_u32(uint32_t* p, uint64_t n, hipStream_t s) {
    stream_op(fmt("iota_u32 %s n %llu %s", W(p), (unsigned long long)n, tok(s).c_str()));
    for (uint64_t i = 0; i < n; i++) p[i] = (uint32_t)i;
}
void segment_flags(const uint64_t* key, uint64_t n, uint32_t* flag, hipStream_t s) {
    stream_op(fmt("segment_flags key %s n %llu flag %s %s", W(key), (unsigned long long)n, W(flag), tok(s).c_str()));
    for (uint64_t i = 0; i < n; i++) flag[i] = i == 0 || key[i] != key[i - 1];
}
void segment_scatter(const uint64_t* key, const uint64_t* fs, uint64_t n, uint64_t* edge_key, uint64_t* edge_off, hipStream_t s) {
    stream_op(fmt("segment_scatter key %s flag_scan %s n %llu edge_key %s edge_off %s %s", W(key), W(fs), (unsigned long long)n, W(edge_key), W(edge_off), tok(s).c_str()));
    for (uint64_t i = 0; i < n; i++) if (fs[i + 1] != fs[i]) { edge_key[fs[i]] = key[i]; edge_off[fs[i]] = i; }
    if (n) edge_off[fs[n]] = n;
}

// selected edge e keeps 1 + e % capacity of the supports it has room for
void edge_coords(const EdgeRecs& r, const uint64_t* edge_key, const uint64_t* edge_off, const uint32_t* cg_ops, const uint32_t* contig_len, const uint32_t* read_len, uint32_t n_sel,
                 const uint32_t* sel_edge, const uint64_t* sel_rec_off, const CoordsScratch& sc, uint32_t* head_end, uint32_t* tail_beg, uint32_t* n_supp, uint32_t* supp_lr, uint32_t* spos,
                 uint32_t* epos, int lds_supp, hipStream_t s) {
    stream_op(fmt("edge_coords recs %s edge_key %s edge_off %s cg_ops %s contig_len %s read_len %s n_sel %u sel %s cap_off %s scratch %s head_end %s tail_beg %s n_supp %s "
                  "supp_lr %s spos %s epos %s lds_supp %d %s",
                  recs(r).c_str(), W(edge_key), W(edge_off), W(cg_ops), W(contig_len), W(read_len), n_sel, W(sel_edge), W(sel_rec_off),
                  list({sc.beg1, sc.end1, sc.beg2, sc.end2, sc.cur, sc.best1, sc.best2, sc.best_list}).c_str(), W(head_end), W(tail_beg), W(n_supp), W(supp_lr), W(spos), W(epos), lds_supp,
                  tok(s).c_str()));
    const uint64_t cap = sel_rec_off[n_sel];
    fill(sc.beg1, cap, K_B1); fill(sc.end1, cap, K_E1); fill(sc.beg2, cap, K_B2); fill(sc.end2, cap, K_E2); fill(sc.cur, cap, K_CUR); fill(sc.best_list, cap, K_BEST);
    fill(head_end, n_sel, K_HEAD_END); fill(tail_beg, n_sel, K_TAIL_BEG);
    fill(supp_lr, cap, K_LR); fill(spos, cap, K_SP); fill(epos, cap, K_EP);
    for (uint32_t e = 0; e < n_sel; e++) {
        const uint64_t room = sel_rec_off[e + 1] - sel_rec_off[e];
        n_supp[e] = room ? (uint32_t)(1 + e % room) : 0;
    }
}
void coords_compact(const uint64_t* cap_off, const uint64_t* out_off, uint32_t n_sel, const uint32_t* lr_in, const uint32_t* sp_in, const uint32_t* ep_in, uint32_t* lr_out, uint32_t* sp_out,
                    uint32_t* ep_out, hipStream_t s) {
    stream_op(fmt("coords_compact cap_off %s out_off %s n_sel %u in %s %s %s out %s %s %s %s", W(cap_off), W(out_off), n_sel, W(lr_in), W(sp_in), W(ep_in), W(lr_out), W(sp_out), W(ep_out),
                  tok(s).c_str()));
    for (uint32_t e = 0; e < n_sel; e++)
        for (uint64_t k = 0; k < out_off[e + 1] - out_off[e]; k++) {
            lr_out[out_off[e] + k] = lr_in[cap_off[e] + k]; sp_out[out_off[e] + k] = sp_in[cap_off[e] + k]; ep_out[out_off[e] + k] = ep_in[cap_off[e] + k];
        }
}

}  // namespace hxk
