// hx_api_trace_driver.cpp - runs the chain, edge-support and coordinate operators of hx_api.hip (compiled host-only) on small synthetic data
// sets behind the fake runtime of hx_api_fake_runtime.cpp: no HIP runtime in the link, no GPU (tests/test_hx_api_trace.py). It calls the public
// C-ABI only (include/haslr_hip.h), and prints the fake's trace ("t " lines) and every field of every out-struct ("r " lines).
//   hx_api_trace_driver a|b|c|d|e|f|g|h
//   hx_api_trace_driver fail chain|edges|coords K     the K-th synchronous copy of that operator fails; the call is then repeated
#include <hip/hip_runtime.h>

#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/haslr_hip.h"
#include "hx_api_fake.h"

namespace {

std::string fmt(const char* f, unsigned long long a = 0, unsigned long long b = 0, unsigned long long c = 0) {
    char s[256];
    snprintf(s, sizeof s, f, a, b, c);
    return s;
}

// reads of hits[r] raw records each; every hit column holds (its place in hx_hits << 24) | record
struct Data {
    std::vector<double> km;
    std::vector<uint32_t> clen, rlen, col[9], ops;
    std::vector<uint64_t> roff, cg_off, rho;
    std::vector<uint8_t> packed, is_rev, mapq;
    hx_contigs ctg;
    hx_reads rd;
    hx_hits h;
    Data(uint32_t n_contigs, const std::vector<uint32_t>& hits) {
        for (uint32_t i = 0; i < n_contigs; i++) { km.push_back(10.0 + i); clen.push_back(1000 + i); }
        roff.push_back(0); rho.push_back(0);
        for (uint32_t r = 0; r < hits.size(); r++) {
            rlen.push_back(100 + r);
            roff.push_back(roff.back() + (((100 + r + 3) / 4 + 3) & ~3u));
            rho.push_back(rho.back() + hits[r]);
            for (uint32_t k = 0; k < hits[r]; k++) {
                const uint32_t i = (uint32_t)is_rev.size();
                col[0].push_back(r);
                for (uint32_t j = 1; j < 9; j++) col[j].push_back(j << 24 | i);
                is_rev.push_back(i & 1); mapq.push_back(60);
                cg_off.push_back(2 * (uint64_t)i); ops.push_back(40 << 2); ops.push_back(60 << 2);
            }
        }
        cg_off.push_back(ops.size());
        if (ops.empty()) ops.push_back(0);
        packed.assign(roff.back() + 4, 0x1b);
        ctg = hx_contigs{n_contigs, km.data(), clen.data()};
        rd = hx_reads{(uint32_t)rlen.size(), rlen.data(), roff.data(), packed.data()};
        h = hx_hits{is_rev.size(), col[0].data(), col[1].data(), col[2].data(), col[3].data(), col[4].data(), col[5].data(), col[6].data(), col[7].data(), col[8].data(), is_rev.data(),
                    mapq.data(), cg_off.data(), ops.data()};
    }
};
const std::vector<uint32_t> kSmall{3, 2, 4, 3, 3, 3, 2, 4}, kLarge{3, 2, 4, 3, 3, 3, 2, 4, 5, 5, 5}, kSingle{1, 1, 1, 1};

template <class T> void col(const char* name, const T* p, uint64_t n) {
    if (!p) fake::say(std::string("r   ") + name + " null");
    else if (!n) fake::say(std::string("r   ") + name + " non-null, empty");
    else fake::say(std::string("r   ") + name + fmt(" n %llu first %llx last %llx", n, (unsigned long long)p[0], (unsigned long long)p[n - 1]));
}
void print(const hx_chain_out& o) {
    fake::say(fmt("r chain n_aln %llu n_reads %llu n_cmp %llu", o.n_aln, o.n_reads, o.n_cmp));
    col("hit", o.hit, o.n_aln); col("q_start", o.q_start, o.n_aln); col("q_end", o.q_end, o.n_aln); col("t_start", o.t_start, o.n_aln); col("t_end", o.t_end, o.n_aln);
    col("n_match", o.n_match, o.n_aln); col("n_block", o.n_block, o.n_aln); col("cg_begin", o.cg_begin, o.n_aln); col("cg_end", o.cg_end, o.n_aln);
    col("cg_skip_front", o.cg_skip_front, o.n_aln); col("cg_skip_back", o.cg_skip_back, o.n_aln);
    col("read_off", o.read_off, o.read_off ? (uint64_t)o.n_reads + 1 : 0); col("cmp_off", o.cmp_off, o.cmp_off ? (uint64_t)o.n_reads + 1 : 0); col("cmp_aln", o.cmp_aln, o.n_cmp);
}
void print(const char* which, const hx_rec_side& s, uint64_t n) {
    fake::say(std::string("r  ") + which);
    col("q_start", s.q_start, n); col("q_end", s.q_end, n); col("t_start", s.t_start, n); col("t_end", s.t_end, n); col("is_rev", s.is_rev, n); col("cg_begin", s.cg_begin, n);
    col("cg_end", s.cg_end, n); col("cg_skip_front", s.cg_skip_front, n); col("cg_skip_back", s.cg_skip_back, n);
}
void print(const hx_edges_out& o) {
    fake::say(fmt("r edges n_rec %llu n_edge %llu", o.n_rec, o.n_edge));
    col("key", o.key, o.n_rec); col("lr", o.lr, o.n_rec); col("cmp_head", o.cmp_head, o.n_rec); col("cmp_tail", o.cmp_tail, o.n_rec);
    print("head", o.head, o.n_rec); print("tail", o.tail, o.n_rec);
    col("edge_key", o.edge_key, o.n_edge); col("edge_off", o.edge_off, o.edge_off ? o.n_edge + 1 : 0);
    for (uint64_t e = 0; e < o.n_edge; e++) fake::say(fmt("r   edge %llu key %llx supports %llu", e, o.edge_key[e], o.edge_off[e + 1] - o.edge_off[e]));
}
void print(const hx_coords_out& o) {
    const uint64_t tot = o.supp_off ? o.supp_off[o.n_edge] : 0;
    fake::say(fmt("r coords n_edge %llu supports %llu", o.n_edge, tot));
    col("head_end", o.head_end, o.n_edge); col("tail_beg", o.tail_beg, o.n_edge); col("supp_off", o.supp_off, o.supp_off ? (uint64_t)o.n_edge + 1 : 0);
    col("supp_lr", o.supp_lr, tot); col("spos", o.spos, tot); col("epos", o.epos, tot);
    for (uint64_t i = 0; i < tot; i++) fake::say(fmt("r   support %llu lr %llx", i, o.supp_lr[i]) + fmt(" spos %llx epos %llx", o.spos[i], o.epos[i]));
}
template <class T> bool all_zero(const T& o) {
    const unsigned char* p = (const unsigned char*)&o;
    for (size_t i = 0; i < sizeof o; i++) if (p[i]) return false;
    return true;
}

void die(const char* what) { fake::say(std::string("FAILED ") + what + ": " + hx_last_error()); fake::flush(); exit(1); }
hx_params params() { return hx_params{500, 0.85, 55, 0.15, 3, 20.0}; }

hx_ctx* create() {
    hx_ctx* c = nullptr;
    fake::say("== hx_ctx_create");
    if (hx_ctx_create(0, nullptr, &c)) die("hx_ctx_create");
    return c;
}
void upload(hx_ctx* c, const Data& d) {
    fake::say(fmt("== hx_upload contigs %llu reads %llu hits %llu", d.ctg.n, d.rd.n, d.h.n));
    if (hx_upload(c, &d.ctg, &d.rd, &d.h, d.rho.data())) die("hx_upload");
}
void shard(hx_ctx* c, uint32_t b, uint32_t e) {
    fake::say(fmt("== hx_set_read_shard %llu %llu", b, e));
    if (hx_set_read_shard(c, b, e)) die("hx_set_read_shard");
}
// which operator's K-th synchronous copy fails (0: none); the failed call is checked and repeated
struct Fail { std::string op; int k = 0; };
template <class Out, class Call> void op(const char* name, const Fail& f, Out& out, Call call) {
    if (f.k && f.op == name) {
        fake::say(std::string("== ") + name + fmt(", copy %llu fails", (unsigned long long)f.k));
        memset(&out, 0xff, sizeof out);
        fake::fail_memcpy(f.k);
        const int r = call();
        fake::fail_memcpy(0);
        fake::say(fmt("r failed ret %lld out_all_zero %llu", (unsigned long long)(long long)r, all_zero(out)) + " error: " + hx_last_error());
    }
    fake::say(std::string("== ") + name);
    if (call()) die(name);
    print(out);
}
enum Sel { kAll, kNone, kHairpin };
void stages(hx_ctx* c, Sel sel, const Fail& f = Fail()) {
    const hx_params prm = params();
    hx_chain_out ch;
    hx_edges_out ed;
    hx_coords_out co;
    op("hx_chain_reads", f, ch, [&] { return hx_chain_reads(c, &prm, &ch); });
    op("hx_edge_support", f, ed, [&] { return hx_edge_support(c, &prm, &ed); });
    std::vector<uint32_t> s;
    for (uint32_t e = 0; e < ed.n_edge; e++) {
        const bool hairpin = (((uint32_t)ed.edge_key[e]) ^ 1u) == (uint32_t)(ed.edge_key[e] >> 32);
        if (sel == kAll || (sel == kHairpin && (hairpin || e == 0))) s.push_back(e);
    }
    fake::say(fmt("== selected %llu edges", s.size()));
    op("hx_edge_coords", f, co, [&] { return hx_edge_coords(c, (uint32_t)s.size(), s.data(), &co); });
    fake::say("== hx_free_*");
    hx_free_chain(c, &ch); hx_free_edges(c, &ed); hx_free_coords(c, &co);
    fake::say(fmt("r freed all_zero %llu %llu %llu", all_zero(ch), all_zero(ed), all_zero(co)));
}
void destroy(hx_ctx* c) {
    fake::say("== hx_ctx_destroy");
    hx_ctx_destroy(c);
    fake::flush();
}

// (h) the records of one context, exported as emitted, imported into another
void exchange() {
    const Data d(5, kSmall);
    const hx_params prm = params();
    hx_ctx *c1 = create(), *c2 = create();
    upload(c1, d); upload(c2, d);
    hx_chain_out ch;
    fake::say("== hx_chain_reads");
    if (hx_chain_reads(c1, &prm, &ch)) die("hx_chain_reads");
    print(ch);
    uint64_t n = 0;
    fake::say("== hx_edge_emit");
    if (hx_edge_emit(c1, &prm, &n)) die("hx_edge_emit");
    fake::say(fmt("r emitted %llu records of %llu bytes", n, hx_edge_records_bytes()));
    void* wire = nullptr;
    if (hipMalloc(&wire, n * hx_edge_records_bytes()) != hipSuccess) die("hipMalloc");
    fake::say("== hx_edge_records_export");
    if (hx_edge_records_export(c1, wire, n)) die("hx_edge_records_export");
    hx_edges_out ed;
    fake::say("== hx_edge_records_import");
    if (hx_edge_records_import(c2, wire, n, &ed)) die("hx_edge_records_import");
    print(ed);
    std::vector<uint32_t> s;
    for (uint32_t e = 0; e < ed.n_edge; e++) s.push_back(e);
    hx_coords_out co;
    fake::say("== hx_edge_coords");
    if (hx_edge_coords(c2, (uint32_t)s.size(), s.data(), &co)) die("hx_edge_coords");
    print(co);
    fake::say("== hx_free_*");
    hx_free_chain(c1, &ch); hx_free_edges(c2, &ed); hx_free_coords(c2, &co);
    (void)hipFree(wire);
    destroy(c1); destroy(c2);
}

}  // namespace

int main(int argc, char** argv) {
    const std::string cs = argc > 1 ? argv[1] : "";
    if (cs == "h" && argc == 2) { exchange(); return 0; }
    Fail f;
    if (cs == "fail" && argc == 4) { f.op = std::string("hx_") + (!strcmp(argv[2], "chain") ? "chain_reads" : !strcmp(argv[2], "edges") ? "edge_support" : "edge_coords"); f.k = atoi(argv[3]); }
    else if (argc != 2 || cs.size() != 1 || cs[0] < 'a' || cs[0] > 'g') { fprintf(stderr, "usage: hx_api_trace_driver a|b|c|d|e|f|g|h, or: fail chain|edges|coords K\n"); return 2; }
    hx_ctx* c = create();
    if (cs == "g") {   // the buffers of the larger data set serve the smaller one
        const Data big(7, kLarge), small(5, kSmall);
        upload(c, big); stages(c, kAll);
        upload(c, small); stages(c, kAll);
    } else {
        const Data d(5, cs == "d" ? kSingle : kSmall);
        upload(c, d);
        if (cs == "b") shard(c, 2, 6);
        if (cs == "c") shard(c, 3, 3);
        stages(c, cs == "e" || cs == "c" || cs == "d" ? kNone : cs == "f" ? kHairpin : kAll, f);
    }
    destroy(c);
    return 0;
}
