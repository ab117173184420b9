// poa_modes_plan_text.h - what tests/poa_modes_plan_driver.cpp shares with the harness that printed tests/golden/poa_modes_plan/ (the previous
// poa_modes_run, compiled unchanged and host-only against a fake runtime; DESIGN.md "The general path's round plan and retry rule are pure
// host steps"): the synthetic calls, the rule by which a "launch" answers for a set, the fixed answers of the device queries, and the text.
#ifndef POA_MODES_PLAN_TEXT_H
#define POA_MODES_PLAN_TEXT_H
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "poa_modes.h"

namespace poa_modes_text {

// ---- the fixed answers of the device
constexpr int kCUs = 256;
constexpr uint64_t kFreeBytes = 100000000000ull, kTotalBytes = 288000000000ull;   // hipMemGetInfo: the budget is 40 % of the free bytes
inline int occupancy(int block_threads) { return 1024 / block_threads; }          // workgroups per CU

// ---- what a set "is" on the fake device
constexpr uint32_t KEEP = 0xfffffffeu;
struct Truth {
    uint32_t v = 0;                        // the nodes of its final graph: it needs (v + 1) x (lmax + 1) cells of H
    std::vector<uint32_t> extra;           // per attempt (the last one repeats): the pairs of an alignment beyond its sequence's bases
    std::vector<uint32_t> vseen;           // per attempt: what it reports when its H does not fit (default: the rows that did fit)
    std::vector<uint32_t> force_status;    // per attempt: the status whatever the slot (KEEP: none)
    uint32_t report_pairs = KEEP;          // the pairs it reports in aln_need, whatever its alignments hold
};

struct Case {
    std::vector<uint64_t> set_off{0}, seq_off{0};
    std::string bases;
    std::vector<uint8_t> weights;
    hxk::PoaModesArgs args;
    std::vector<Truth> truth;
    std::vector<uint32_t> runs;            // per set: the launches that took it so far
    uint32_t lcg = 12345;

    void add_set(const std::vector<uint32_t>& lens, Truth t = Truth()) {
        uint64_t sum = 0; uint32_t lmax = 0;
        for (uint32_t L : lens) {
            for (uint32_t j = 0; j < L; j++) { lcg = lcg * 1664525u + 1013904223u; bases.push_back("ACGTacgtNACGTACG"[lcg >> 28]); }
            seq_off.push_back(bases.size());
            sum += L; lmax = std::max(lmax, L);
        }
        set_off.push_back(seq_off.size() - 1);
        if (t.v == 0) t.v = (uint32_t)std::min<uint64_t>(sum, lmax + sum / 16);
        if (t.extra.empty()) t.extra.push_back(1);
        truth.push_back(t);
    }
    // the request as poa_modes_run takes it (call once the sets are in)
    const hxk::PoaModesArgs& view(bool with_weights) {
        if (with_weights) { weights.resize(std::max<size_t>(1, bases.size())); for (size_t k = 0; k < weights.size(); k++) weights[k] = (uint8_t)(1 + (k * 7 + 3) % 60); }
        args.who = "hx_test"; args.n_sets = (uint32_t)set_off.size() - 1; args.set_off = set_off.data(); args.seq_off = seq_off.data(); args.bases = bases.data();
        args.weights = with_weights ? weights.data() : nullptr;
        runs.assign(args.n_sets, 0);
        return args;
    }
};

// ---- the rule: what a workgroup leaves for set i in a slot of `slot` bytes of which its graph pools take `pools`, a cell of H `cell` bytes,
// its share of the alignment pool aln_room pairs
struct SetResult { uint32_t status = 0, vseen = 0, pairs = 0, ncols = 0, cns_len = 0, nv = 0, ne = 0; bool done = false; std::vector<uint32_t> cnt; };
inline SetResult run_set(Case& cs, uint32_t i, uint64_t slot, uint64_t pools, uint64_t cell, uint32_t aln_room) {
    const uint32_t attempt = cs.runs[i]++;
    const Truth& t = cs.truth[i];
    auto at = [&](const std::vector<uint32_t>& v, uint32_t dflt) { return v.empty() ? dflt : v[std::min<size_t>(attempt, v.size() - 1)]; };
    SetResult r;
    uint32_t lmax = 0, non_empty = 0;
    for (uint64_t k = cs.set_off[i]; k < cs.set_off[i + 1]; k++) { const uint32_t L = (uint32_t)(cs.seq_off[k + 1] - cs.seq_off[k]); lmax = std::max(lmax, L); non_empty += L != 0; }
    if (pools > slot) { r.status = 2; return r; }
    const uint64_t hcap = (slot - pools) / cell;
    const uint32_t forced = attempt < t.force_status.size() ? t.force_status[attempt] : KEEP;
    if (forced == 1 || (forced == KEEP && non_empty >= 2 && (uint64_t)(t.v + 1) * (lmax + 1) > hcap)) {
        r.status = 1; r.vseen = at(t.vseen, (uint32_t)std::min<uint64_t>(t.v, hcap / (lmax + 1)));
        return r;
    }
    if (forced != KEEP && forced != 0 && forced != 3) { r.status = forced; return r; }
    r.done = true;
    r.nv = t.v; r.ne = t.v + non_empty - 1; r.ncols = t.v - t.v / 8; r.cns_len = lmax;
    bool seen = false;
    uint64_t pairs = 0;
    for (uint64_t k = cs.set_off[i]; k < cs.set_off[i + 1]; k++) {
        const uint32_t L = (uint32_t)(cs.seq_off[k + 1] - cs.seq_off[k]);
        r.cnt.push_back(L && seen ? L + at(t.extra, 1) : 0);
        pairs += r.cnt.back();
        seen = seen || L;
    }
    r.pairs = t.report_pairs != KEEP ? t.report_pairs : (uint32_t)pairs;
    r.status = forced == 3 || (cs.args.graph && r.pairs > aln_room) ? 3 : 0;
    return r;
}

// ---- the calls
inline bool make_case(const std::string& name, Case& cs) {
    hxk::PoaModesArgs& a = cs.args;
    a.match = 5; a.mismatch = -4; a.gap = -8; a.gap_extend = -6; a.gap_open2 = -10; a.gap_extend2 = -4; a.type = 1;
    bool wts = false;
    auto T = [](uint32_t v, std::vector<uint32_t> vseen = {}, std::vector<uint32_t> force = {}, std::vector<uint32_t> extra = {}, uint32_t report = KEEP) {
        Truth t; t.v = v; t.vseen = vseen; t.force_status = force; t.extra = extra; t.report_pairs = report; return t;
    };
    static const uint32_t max_len[3] = {1024 * 32 - 1, 1024 * 16 - 1, 512 * 16 - 1};
    static const uint32_t cols[3][3] = {{64 * 16, 256 * 16, 256 * 32}, {64 * 16, 256 * 16, 512 * 16}, {64 * 16, 128 * 16, 256 * 16}};   // of the instances below the widest
    const int gm = name.size() > 4 && name.compare(name.size() - 4, 4, "_aff") == 0 ? 1 : name.size() > 4 && name.compare(name.size() - 4, 4, "_cvx") == 0 ? 2 : 0;
    a.gap_model = gm;
    const std::string stem = gm ? name.substr(0, name.size() - 4) : name.size() > 4 && name.compare(name.size() - 4, 4, "_lin") == 0 ? name.substr(0, name.size() - 4) : name;
    if (stem == "edge") {   // lmax + 1 at the columns of an instance, and one more; an empty set, a set of empty sequences, one base
        for (int k = 0; k < 3; k++) { cs.add_set({cols[gm][k] - 1, 7}); cs.add_set({cols[gm][k], 7}); }
        cs.add_set({max_len[gm], 3});
        cs.add_set({}); cs.add_set({0, 0}); cs.add_set({1}); cs.add_set({1, 1, 0, 2});
    } else if (stem == "long") {
        cs.add_set({30, 40}); cs.add_set({10, max_len[gm] + 1});
    } else if (stem == "big_set") {
        cs.add_set({30, 40}); cs.add_set(std::vector<uint32_t>(65, 32767));
    } else if (stem == "cap" || stem == "cap_fail") {
        a.slot_kb_cap = 1;
        const std::vector<uint32_t> ten(10, 100);
        cs.add_set(ten, T(500, {100}));            // comes back once: 2 vest > 2 vseen + 64
        cs.add_set(ten, T(900, {400, 700}));       // ... 2 vseen + 64 > 2 vest; then again, to the worst case
        cs.add_set({1100, 30}, T(1110, {}, stem == "cap_fail" ? std::vector<uint32_t>{KEEP, 1} : std::vector<uint32_t>{}));   // alone in its instance, vest == sum_len from the start: let past while capped; (cap_fail) not after
        cs.add_set({50});                           // no DP: done in the capped slot
    } else if (stem == "status2" || stem == "status3_plain") {   // a status the retry rule has no answer to: MS_GRAPH_OVERFLOW; MS_ALN_OVERFLOW in a call without a graph
        cs.add_set({30, 40}); cs.add_set(std::vector<uint32_t>(10, 100), T(500, {}, {stem == "status2" ? 2u : 3u}));   // (its estimate is below its worst case: an H overflow would be rerun) cs.add_set({12, 12});
    } else if (stem == "graph_aln" || stem == "graph_both" || stem == "graph_aln2" || stem == "graph_ff" || stem == "graph_lie") {
        a.graph = 1; a.aln_cap = 1;
        if (stem == "graph_both") a.slot_kb_cap = 1;
        cs.add_set({4000});                                       // no DP: its share stays in the first round's pool; its slot is the largest of its instance
        cs.add_set({1100, 1100, 1100}, T(2000));                  // fits beside it, comes back for its alignments, then alone for its slot
        cs.add_set({40, 0, 35, 38}, T(60, {}, {}, stem == "graph_aln2" ? std::vector<uint32_t>{1, 2} : std::vector<uint32_t>{1}, stem == "graph_ff" ? 0xffffffffu : KEEP));
        cs.add_set({}); cs.add_set({9});
        if (stem == "graph_lie") { a.aln_cap = 0; cs.add_set({20, 20, 20}, T(30, {}, {}, {40}, 5)); }   // reports fewer pairs than it wrote
    } else if (stem == "budget" || stem == "budget_over") {
        for (int k = 0; k < 40; k++) cs.add_set({300, 300 - (uint32_t)(k % 4), 300, 300});   // (ten sets of every cost: the order among equals shows)
        for (int k = 0; k < 3; k++) cs.add_set({1100, 1100, 1100});
        a.workspace_gb = 0.0095;
        if (stem == "budget_over") { cs.add_set({1500, 1500, 1500, 1500, 1500, 1500}); a.workspace_gb = 0.004; }
    } else if (stem == "msa" || stem == "msa_nocns") {
        a.msa = 1; a.include_consensus = stem == "msa";
        cs.add_set({20, 30, 25}); cs.add_set({}); cs.add_set({0, 0}); cs.add_set({15, 0, 15}); cs.add_set({64, 65, 10}, T(72));
    } else if (stem == "cov" || stem == "cov_prof") {
        a.weighted = 1; a.want_coverage = 1; a.want_profile = stem == "cov_prof"; wts = stem == "cov_prof";
        cs.add_set({1, 20, 1, 20}); cs.add_set({}); cs.add_set({64, 65, 2}, T(72)); cs.add_set({1});
    } else if (stem == "strand" || stem == "strand_w") {
        a.strand = 1; wts = stem == "strand_w";
        a.msa = 1; a.include_consensus = 1; a.want_coverage = wts;
        cs.add_set({12, 9, 0, 5}); cs.add_set({7});
    } else if (stem == "bound_under" || stem == "bound_at") {
        // the score bound of the full matrix (kernels/poa_modes_plan.h, SCORE_BOUND): set 1 has 1 024 bases and runs in the instance of 1 024 columns,
        // so a magnitude of 2^18 makes the product exactly 2^29 and one less stays under it; the magnitude stands in a positive and in a negative score
        cs.add_set({30, 40}); cs.add_set({600, 424});
        if (stem == "bound_under") a.match = (1 << 18) - 1; else a.mismatch = -(1 << 18);
    } else if (stem == "bound_wide") {
        // the columns are the instance's, not the sequence's: 1 024 bases + 1 take the second instance (4 096, 4 096, 2 048 columns by gap model)
        cs.add_set({1024, 1024});
        a.gap = a.gap_open2 = gm == 2 ? -(1 << 17) : -87382;
    } else if (stem == "bound_int8") {
        // the largest set the path takes with the longest sequence of its gap model, every score at an end of int8
        a.match = 127; a.mismatch = a.gap = a.gap_extend = a.gap_open2 = a.gap_extend2 = -128;
        const uint32_t most = (1u << 21) - 2;
        std::vector<uint32_t> lens(most / max_len[gm], max_len[gm]);
        lens.push_back(most % max_len[gm]);
        cs.add_set(lens);
    } else return false;
    cs.view(wts);
    return true;
}
inline const std::vector<std::string>& case_names() {
    static const std::vector<std::string> n = {"edge_lin", "edge_aff", "edge_cvx", "long_lin", "long_aff", "long_cvx", "big_set", "cap", "cap_fail", "status2", "status3_plain", "graph_aln", "graph_both", "graph_aln2",
                                               "graph_ff", "graph_lie", "budget", "budget_over", "msa", "msa_nocns", "cov", "cov_prof", "strand", "strand_w"};
    return n;
}

// ---- the text: one line per fact, printed from plain values
struct Text {
    FILE* f;
    static uint64_t fnv(const uint8_t* p, uint64_t n) { uint64_t h = 1469598103934665603ull; for (uint64_t k = 0; k < n; k++) h = (h ^ p[k]) * 1099511628211ull; return h; }
    void set(uint32_t i, uint64_t seq_begin, uint64_t sum_len, uint64_t cns_off, uint32_t nseq, uint32_t lmax) const {
        fprintf(f, "set %u seq_begin %llu sum_len %llu cns_off %llu nseq %u lmax %u\n", i, (unsigned long long)seq_begin, (unsigned long long)sum_len, (unsigned long long)cns_off, nseq, lmax);
    }
    void bytes(const char* what, const uint8_t* p, uint64_t n) const {   // in full up to 256, else their count and hash
        fprintf(f, "%s n %llu", what, (unsigned long long)n);
        if (n > 256) fprintf(f, " fnv %016llx", (unsigned long long)fnv(p, n));
        else for (uint64_t k = 0; k < n; k++) fprintf(f, " %u", p[k]);
        fprintf(f, "\n");
    }
    void occ(int nt) const { fprintf(f, "occupancy asked for block %d\n", nt); }
    void ws(uint64_t total) const { fprintf(f, "workspace grows to %llu\n", (unsigned long long)total); }
    void round(uint32_t r) const { fprintf(f, "round %u\n", r); }
    void pool(uint64_t alloc_bytes) const { fprintf(f, "pool alloc_bytes %llu\n", (unsigned long long)alloc_bytes); }
    void share(uint32_t set, uint64_t at, uint32_t room) const { fprintf(f, "share set %u at %llu room %u\n", set, (unsigned long long)at, room); }
    void launch(int variant, uint32_t grid, uint32_t block, uint32_t n_items, uint64_t order_at, uint64_t counter_at, uint64_t slot_bytes, const int32_t sc[7]) const {
        fprintf(f, "launch variant %d grid %u block %u n_items %u order_at %llu counter_at %llu slot_bytes %llu m %d n %d g %d type %d e %d q %d c %d\n", variant, grid, block, n_items, (unsigned long long)order_at,
                (unsigned long long)counter_at, (unsigned long long)slot_bytes, sc[0], sc[1], sc[2], sc[3], sc[4], sc[5], sc[6]);
    }
    void order(const uint32_t* p, uint32_t n) const { fprintf(f, "order"); for (uint32_t k = 0; k < n; k++) fprintf(f, " %u", p[k]); fprintf(f, "\n"); }
    void result(uint32_t set, const SetResult& r) const { fprintf(f, "result set %u status %u vseen %u pairs %u done %d\n", set, r.status, r.vseen, r.pairs, (int)r.done); }
    void row(const char* kernel, uint64_t k, uint64_t src, uint64_t dst, uint64_t hoff, uint32_t len, uint32_t ncols, uint32_t kind, long long pool_round) const {
        fprintf(f, "row %s %llu src %llu dst %llu hoff %llu len %u ncols %u kind %u pool %lld\n", kernel, (unsigned long long)k, (unsigned long long)src, (unsigned long long)dst, (unsigned long long)hoff, len, ncols, kind, pool_round);
    }
    void chunk(const char* kernel, uint32_t row, uint32_t first) const { fprintf(f, "chunk %s row %u first %u\n", kernel, row, first); }
    void rows_launch(const char* kernel, uint32_t grid, uint32_t n_chunks, uint32_t stride) const { fprintf(f, "launch %s grid %u n_chunks %u stride %u\n", kernel, grid, n_chunks, stride); }
    void alloc(const char* what, uint64_t bytes) const { fprintf(f, "alloc %s bytes %llu\n", what, (unsigned long long)bytes); }
    template <class V> void list(const char* what, const V& v) const { fprintf(f, "%s", what); for (auto x : v) fprintf(f, " %llu", (unsigned long long)x); fprintf(f, "\n"); }
    void out(const hxk::PoaModesOut& o) const {
        fprintf(f, "out retried %u aln_retried %u seq_bases %llu n_aligned %llu msa_bytes %zu msa_moved %llu cov %zu prof %zu cov_moved %llu gather_moved %llu\n", o.retried, o.aln_retried, (unsigned long long)o.seq_bases,
                (unsigned long long)o.n_aligned, o.msa.size(), (unsigned long long)o.msa_moved_bytes, o.cov.size(), o.prof.size(), (unsigned long long)o.cov_moved_bytes, (unsigned long long)o.gather_moved_bytes);
        list("cns_off", o.cns_off); list("msa_rows", o.msa_rows); list("msa_cols", o.msa_cols); list("msa_off", o.msa_off);
        list("node_off", o.node_off); list("edge_off", o.edge_off); list("aln_off", o.aln_off);
    }
    void error(const std::string& e) const { fprintf(f, "error %s\n", e.c_str()); }
};

}  // namespace poa_modes_text
#endif
