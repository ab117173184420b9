// spoa_hx.hpp — the per-edge POA operator of haslr_assemble behind the reference's own operator API.
//
// The reference computes every gap consensus with five calls of rvaser/spoa 1.1.3 (Assemble.cpp:499-554):
//     auto alignment_engine = spoa::createAlignmentEngine(static_cast<spoa::AlignmentType>(1), 5, -4, -8);   // :499
//     auto graph = spoa::createGraph();                                                                         // :500
//     for every supporting sub-sequence, in stored order:
//         auto alignment = alignment_engine->align_sequence_with_graph(seq, graph);                            // :539
//         graph->add_alignment(alignment, seq);                                                                 // :540
//     std::string consensus = graph->generate_consensus();                                                      // :554
// This header declares exactly those symbols (namespace spoa, the same signatures and ownership: unique_ptr
// engine + graph per edge, strings by const reference, consensus by value) over the C-ABI of haslr_hip.h, so that
// the reference's Assemble.cpp compiles against it unchanged (`#include "spoa_hx.hpp"` in place of "spoa.hpp",
// link -lhaslr_hip instead of libspoa.a) and its consensus runs on the MI355X.
//
// How it maps: a partial-order graph lives on the device only while it is being built, so the calls are recorded and
// the work happens in generate_consensus(): align_sequence_with_graph() returns a token (an Alignment holding one
// (-1, ticket) pair, not a list of node/position pairs), add_alignment() appends the sequence that goes with a token,
// generate_consensus() sends the recorded sequences, in order, through hx_poa_sequences_mode (the engine's alignment type and
// three scores, linear gap; an engine made with five scores, gap open below gap extend, goes through
// hx_poa_sequences_affine, an engine made with seven scores - two gap pieces, a gap of k bases scores max(g + (k-1) e, q + (k-1) c) -
// through hx_poa_sequences_convex) and returns what spoa's generate_consensus returns for them. A graph that was given weights or
// qualities, or is asked for the coverage, goes through hx_poa_weighted instead (below; hx_poa_weighted_convex under a seven-score engine,
// as the MSA goes through hx_poa_msa_convex).
// All three of spoa's alignment types are taken: kNW (global, what the reference uses) runs the tuned global path, kSW (local) and
// kOV (overlap) the general path of the library (DESIGN.md "General POA path"). What is supported beyond that is the reference's call
// pattern: every alignment added to the graph it was computed against, in the order it was computed. spoa 1.1.3 exits on invalid input; this header throws std::runtime_error with the
// library's message instead (there is no CPU fallback: without a HIP device every consensus fails loudly).
//
// Threads: the reference calls from gopt.num_threads pthreads, each with its own engine and graph (asm_cal_cns_seq_MT, Assemble.cpp:562-605).
// All of them share one device context here (created on first use, device HASLR_DEVICE or 0), and their generate_consensus() calls are
// FLAT-COMBINED: a caller queues its sequence set; the first one in becomes the submitter, waits HASLR_SPOA_BATCH_US microseconds (default
// 200) or until HASLR_SPOA_BATCH sets (default 256) are queued - only while it has company: a lone caller (-t 1) submits at once - and sends
// everything queued through ONE hx_poa_sequences_mode / hx_poa_sequences_affine call per alignment type and set of scores; callers that arrive while a call is on the device form the next batch. A set that makes the
// shared call fail is isolated (every set of that call again, on its own): only its caller gets the exception. With -t 64 the reference's own thread fan-out therefore puts ~64 edges into
// every launch instead of one. spoa::hx::consensus_batch() below is the entry to use from new code: all edges in one call (that is what
// haslr_amd's own pipeline does through hx_poa_batch). spoa::hx::stats() tells how many device calls served how many sets.
//
// The second output of a spoa graph, the multiple sequence alignment, is there too: Graph::generate_multiple_sequence_alignment(dst,
// include_consensus) with spoa's signature sends the recorded sequences through hx_poa_msa (every alignment type runs the general path
// there) and replaces dst by one gapped row per added sequence, in the order they were added, plus the consensus as the last row when asked
// for. As in spoa, add_alignment ignores an empty sequence, so it has no row (the C-ABI and spoa::hx::msa_batch give a row of gaps for an
// empty member of a set). An MSA call is NOT flat-combined with other threads' calls: it takes the device's mutex like consensus_batch and
// is one device call of its own; spoa::hx::msa_batch() takes many sets in one call. Like kSW, kOV and the affine engines, the MSA is held to
// a CPU restatement of spoa's rule by the tests, not to spoa itself, which is not available to them.
//
// Base weights and coverage: add_alignment has spoa 1.1.3's three overloads - one weight for every base of the sequence (default 1), a
// quality string (weight = character - 33) and a vector of weights, one per base - and generate_consensus(dst) fills dst with the coverage
// of every consensus base. A weight is 1..255 (include/haslr_hip.h, hx_poa_weighted, says why 0 is refused and not reinterpreted); a size
// that does not match the sequence, a weight of 0 or above 255, and a quality character outside '"'..'~' throw std::invalid_argument.
// Callers with real FASTQ clamp their qualities to '"' or more themselves. A graph that has only seen weight 1 and is asked for the plain
// consensus keeps the route above (flat combining, the tuned kNW path); a graph with any other weight, or a call of
// generate_consensus(dst), is one device call of its own through hx_poa_weighted, as the MSA call is. spoa::hx::weighted_batch() takes
// many sets in one call. Held to a CPU restatement of spoa's rule by the tests, like the MSA.
//
// The graph itself: Graph::print_dot(path) (spoa 1.1.3's signature; an empty path does nothing) and Graph::print_gfa(path) write the
// partial-order graph of the recorded sequences, and Graph::alignment(k) returns the real Alignment of the k-th added sequence - spoa's
// (node id | -1, position | -1) pairs against the graph as it was before that sequence was added. align_sequence_with_graph() keeps
// returning its token: the graph exists on the device only during a call, so the real pairs are available from alignment(k) after the
// device call, not before add_alignment. All three go through hx_poa_graph (every alignment type runs the general path there; the
// graph's weights count): a device call of its own under the device's mutex, not flat-combined, like the MSA. spoa::hx::graph_batch()
// takes many sets in one call and returns a GraphData per set; spoa::hx::to_dot / to_gfa turn one into text (the formats: DESIGN.md
// "Graph and alignment output"; the Python writers haslr_amd.hip.graph_to_dot / graph_to_gfa give the same bytes). The DOT text follows
// spoa's print_dot as published; spoa is not available to the tests, so byte equality with it is not claimed. Held to a CPU restatement.
//
// This is product code. It is never used to build oracle/_ref (a reference build must not be made with stand-in
// headers): tests/test_spoa_header.py compiles a small caller written against the five symbols, nothing else.
#ifndef HASLR_SPOA_HX_HPP
#define HASLR_SPOA_HX_HPP
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstdlib>
#include <fstream>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "haslr_hip.h"

namespace spoa {

enum class AlignmentType { kSW, kNW, kOV };   // values 0, 1, 2 as in spoa 1.1.3 (the reference passes 1)
using Alignment = std::vector<std::pair<std::int32_t, std::int32_t>>;

namespace hx {

struct Device {
    hx_ctx* ctx = nullptr;
    std::mutex mu;                    // guards ctx and every call into it
    // flat combining of concurrent generate_consensus() calls
    struct Request { const std::vector<std::string>* seqs; AlignmentType type; std::int8_t m, n, g, e, q, c; std::string result, error; bool done, answered; };   // answered: result or error is final (an empty consensus is a result)
    std::mutex qmu;
    std::condition_variable qcv;
    std::vector<Request*> queue;
    bool submitting = false;          // a submitter is collecting or has a batch on the device
    bool company = false;             // the previous batch had, or its device call saw, more than one caller: the next submitter waits its window out
    std::size_t arrivals = 0;         // requests queued since the current batch was taken
    std::uint64_t calls = 0, sets = 0;
    // (no destructor: this object is destroyed during static destruction, possibly after the HIP runtime has torn itself down -
    //  the context and its device memory are left to the end of the process; spoa::hx::shutdown() releases them explicitly)
};
inline Device& device() {
    static Device d;
    return d;
}
inline hx_ctx* context_locked(Device& d) {   // call with d.mu held
    if (!d.ctx) {
        // before HIP initialises: the POA launch classes overlap on separate hardware queues (include/haslr_hip.h; an application's own setting wins)
        setenv("GPU_MAX_HW_QUEUES", "8", 0);
        const char* dev = std::getenv("HASLR_DEVICE");
        if (hx_ctx_create(dev ? std::atoi(dev) : 0, nullptr, &d.ctx) != 0) throw std::runtime_error(std::string("spoa_hx: ") + hx_last_error());
    }
    return d.ctx;
}
// releases the shared device context (optional: call it when no Graph is in use any more, before main returns)
inline void shutdown() {
    Device& d = device();
    std::lock_guard<std::mutex> lock(d.mu);
    if (d.ctx) { hx_ctx_destroy(d.ctx); d.ctx = nullptr; }
}
struct Stats { std::uint64_t device_calls, sets; };
inline Stats stats() {
    Device& d = device();
    std::lock_guard<std::mutex> lock(d.qmu);
    return Stats{d.calls, d.sets};
}

namespace detail {
using Sets = std::vector<const std::vector<std::string>*>;
inline Sets pointers(const std::vector<std::vector<std::string>>& sets) {
    Sets p;
    for (const auto& st : sets) p.push_back(&st);
    return p;
}
// the C-ABI's layout of sets of strings (hx_poa_sequences in haslr_hip.h)
struct Flat {
    std::vector<std::uint64_t> set_off{0}, seq_off{0};
    std::string bases;
    explicit Flat(const Sets& sets) {
        for (const auto* st : sets) {
            for (const auto& s : *st) { bases += s; seq_off.push_back(bases.size()); }
            set_off.push_back(seq_off.size() - 1);
        }
    }
    std::uint32_t n_sets() const { return (std::uint32_t)(set_off.size() - 1); }
};
// call(ctx) under the device's mutex; throws the library's message when it fails, else returns take(ctx), still under the mutex
template <class Call, class Take>
auto locked_call(Call call, Take take) -> decltype(take((hx_ctx*)nullptr)) {
    Device& d = device();
    std::lock_guard<std::mutex> lock(d.mu);
    hx_ctx* ctx = context_locked(d);
    if (call(ctx) != 0) throw std::runtime_error(std::string("spoa_hx: ") + hx_last_error());
    return take(ctx);
}
inline std::vector<std::string> strings_of(const hx_cns_out& out) {
    std::vector<std::string> res(out.n_edge);
    for (std::size_t i = 0; i < res.size(); i++) res[i].assign(out.cns + out.cns_off[i], out.cns + out.cns_off[i + 1]);
    return res;
}
// the consensus strings of one hx_poa_sequences* call: call(ctx, &out)
template <class Call>
std::vector<std::string> consensus_call(Call call) {
    hx_cns_out out;
    return locked_call([&](hx_ctx* ctx) { return call(ctx, &out); },
                       [&](hx_ctx* ctx) -> std::vector<std::string> { std::vector<std::string> res = strings_of(out); hx_free_cns(ctx, &out); return res; });
}
}  // namespace detail

// consensus of every set of sequences (set = the sub-sequences of one edge in alignment order) in ONE device call
inline std::vector<std::string> consensus_batch(const std::vector<const std::vector<std::string>*>& sets, std::int8_t m = 5, std::int8_t n = -4, std::int8_t g = -8) {
    const detail::Flat f(sets);
    const hx_poa_params pp{m, n, g};
    return detail::consensus_call([&](hx_ctx* ctx, hx_cns_out* out) { return hx_poa_sequences(ctx, f.n_sets(), f.set_off.data(), f.seq_off.data(), f.bases.c_str(), &pp, out); });
}
inline std::vector<std::string> consensus_batch(const std::vector<std::vector<std::string>>& sets, std::int8_t m = 5, std::int8_t n = -4, std::int8_t g = -8) {
    return consensus_batch(detail::pointers(sets), m, n, g);
}
// ... with spoa's alignment type (the overloads above are kNW)
inline std::vector<std::string> consensus_batch(const std::vector<const std::vector<std::string>*>& sets, AlignmentType type, std::int8_t m = 5, std::int8_t n = -4, std::int8_t g = -8) {
    const detail::Flat f(sets);
    const hx_poa_mode_params mp{m, n, g, static_cast<std::int32_t>(type)};
    return detail::consensus_call([&](hx_ctx* ctx, hx_cns_out* out) { return hx_poa_sequences_mode(ctx, f.n_sets(), f.set_off.data(), f.seq_off.data(), f.bases.c_str(), &mp, out); });
}
inline std::vector<std::string> consensus_batch(const std::vector<std::vector<std::string>>& sets, AlignmentType type, std::int8_t m = 5, std::int8_t n = -4, std::int8_t g = -8) {
    return consensus_batch(detail::pointers(sets), type, m, n, g);
}

// ... with affine gaps: gap open g, gap extend e (g <= e <= 0; e == g is the linear model and takes the overloads above)
inline std::vector<std::string> consensus_batch(const std::vector<const std::vector<std::string>*>& sets, AlignmentType type, std::int8_t m, std::int8_t n, std::int8_t g, std::int8_t e) {
    if (e == g) return consensus_batch(sets, type, m, n, g);
    const detail::Flat f(sets);
    const hx_poa_affine_params ap{m, n, g, e, static_cast<std::int32_t>(type)};
    return detail::consensus_call([&](hx_ctx* ctx, hx_cns_out* out) { return hx_poa_sequences_affine(ctx, f.n_sets(), f.set_off.data(), f.seq_off.data(), f.bases.c_str(), &ap, out); });
}
inline std::vector<std::string> consensus_batch(const std::vector<std::vector<std::string>>& sets, AlignmentType type, std::int8_t m, std::int8_t n, std::int8_t g, std::int8_t e) {
    return consensus_batch(detail::pointers(sets), type, m, n, g, e);
}

// ... with convex gaps: a second piece, gap open q, gap extend c (q <= c <= 0, q <= g); a gap of k bases scores max(g + (k-1) e, q + (k-1) c).
// c <= e: the second piece never wins, the library takes the affine route. Sequences of up to 8 191 bases otherwise.
inline std::vector<std::string> consensus_batch(const std::vector<const std::vector<std::string>*>& sets, AlignmentType type, std::int8_t m, std::int8_t n, std::int8_t g, std::int8_t e,
                                                std::int8_t q, std::int8_t c) {
    if (q == g && c == e) return consensus_batch(sets, type, m, n, g, e);
    const detail::Flat f(sets);
    const hx_poa_convex_params cp{m, n, g, e, q, c, static_cast<std::int32_t>(type)};
    return detail::consensus_call([&](hx_ctx* ctx, hx_cns_out* out) { return hx_poa_sequences_convex(ctx, f.n_sets(), f.set_off.data(), f.seq_off.data(), f.bases.c_str(), &cp, out); });
}
inline std::vector<std::string> consensus_batch(const std::vector<std::vector<std::string>>& sets, AlignmentType type, std::int8_t m, std::int8_t n, std::int8_t g, std::int8_t e, std::int8_t q,
                                                std::int8_t c) {
    return consensus_batch(detail::pointers(sets), type, m, n, g, e, q, c);
}

namespace detail {
inline std::vector<std::vector<std::string>> rows_of(const hx_msa_out& out, std::size_t n_sets) {
    std::vector<std::vector<std::string>> res(n_sets);
    for (std::size_t i = 0; i < n_sets; i++)
        for (std::uint32_t r = 0; r < out.n_rows[i]; r++) {
            const char* p = out.msa + out.msa_off[i] + (std::uint64_t)r * out.n_cols[i];
            res[i].emplace_back(p, p + out.n_cols[i]);
        }
    return res;
}
}  // namespace detail

// the multiple sequence alignment of every set in ONE device call (hx_poa_msa): per set one gapped row per sequence, in order, all of
// the set's column count wide, and with include_consensus the consensus as one more, last row. e == g is the linear gap model. The C-ABI's
// rule holds here: an empty sequence in a set gives a row of gaps (Graph below never records one, as spoa ignores it).
inline std::vector<std::vector<std::string>> msa_batch(const std::vector<const std::vector<std::string>*>& sets, AlignmentType type, std::int8_t m = 5, std::int8_t n = -4, std::int8_t g = -8,
                                                       std::int8_t e = -8, bool include_consensus = false) {
    const detail::Flat f(sets);
    const hx_poa_msa_params mp{m, n, g, e, static_cast<std::int32_t>(type), include_consensus ? 1 : 0};
    hx_msa_out out;
    return detail::locked_call([&](hx_ctx* ctx) { return hx_poa_msa(ctx, f.n_sets(), f.set_off.data(), f.seq_off.data(), f.bases.c_str(), &mp, &out); }, [&](hx_ctx* ctx) -> std::vector<std::vector<std::string>> {
        std::vector<std::vector<std::string>> res = detail::rows_of(out, sets.size());
        hx_free_msa(ctx, &out);
        return res;
    });
}
inline std::vector<std::vector<std::string>> msa_batch(const std::vector<std::vector<std::string>>& sets, AlignmentType type, std::int8_t m = 5, std::int8_t n = -4, std::int8_t g = -8,
                                                       std::int8_t e = -8, bool include_consensus = false) {
    return msa_batch(detail::pointers(sets), type, m, n, g, e, include_consensus);
}
// ... with convex gaps (hx_poa_msa_convex): all six scores are given
inline std::vector<std::vector<std::string>> msa_batch(const std::vector<const std::vector<std::string>*>& sets, AlignmentType type, std::int8_t m, std::int8_t n, std::int8_t g, std::int8_t e,
                                                       std::int8_t q, std::int8_t c, bool include_consensus = false) {
    const detail::Flat f(sets);
    const hx_poa_convex_params cp{m, n, g, e, q, c, static_cast<std::int32_t>(type)};
    hx_msa_out out;
    return detail::locked_call([&](hx_ctx* ctx) { return hx_poa_msa_convex(ctx, f.n_sets(), f.set_off.data(), f.seq_off.data(), f.bases.c_str(), &cp, include_consensus ? 1 : 0, &out); },
                               [&](hx_ctx* ctx) -> std::vector<std::vector<std::string>> {
        std::vector<std::vector<std::string>> res = detail::rows_of(out, sets.size());
        hx_free_msa(ctx, &out);
        return res;
    });
}
inline std::vector<std::vector<std::string>> msa_batch(const std::vector<std::vector<std::string>>& sets, AlignmentType type, std::int8_t m, std::int8_t n, std::int8_t g, std::int8_t e, std::int8_t q,
                                                       std::int8_t c, bool include_consensus = false) {
    return msa_batch(detail::pointers(sets), type, m, n, g, e, q, c, include_consensus);
}

// the consensus of every set under per-base weights in ONE device call (hx_poa_weighted), with the coverage of every consensus base and
// the four letter counts (A, C, G, T) of its column when asked for. weights: one vector per set with one vector per sequence with one
// weight (1..255) per base, or empty: every weight is 1. e == g is the linear gap model.
struct Weighted {
    std::vector<std::string> consensus;
    std::vector<std::vector<std::uint32_t>> coverage;   // per set, one per consensus base (empty unless asked for)
    std::vector<std::vector<std::uint32_t>> profile;    // per set, four per consensus base (empty unless asked for)
};
namespace detail {
// the flattening of the weights, the call and the outputs of both weighted_batch forms: call(ctx, flat sets, weights or null, &out)
template <class Call>
Weighted weighted_call(const std::vector<const std::vector<std::string>*>& sets, const std::vector<const std::vector<std::vector<std::uint8_t>>*>& weights, bool coverage, bool profile, Call call) {
    if (!weights.empty() && weights.size() != sets.size()) throw std::invalid_argument("spoa_hx: weighted_batch needs one set of weights per set of sequences, or none");
    const detail::Flat f(sets);
    std::vector<std::uint8_t> w;
    for (std::size_t i = 0; i < sets.size() && !weights.empty(); i++) {
        const auto& st = *sets[i];
        if (weights[i]->size() != st.size()) throw std::invalid_argument("spoa_hx: weighted_batch: a set has another number of weight vectors than of sequences");
        for (std::size_t k = 0; k < st.size(); k++) {
            const auto& wk = (*weights[i])[k];
            if (wk.size() != st[k].size()) throw std::invalid_argument("spoa_hx: weighted_batch: a sequence has another number of weights than of bases");
            w.insert(w.end(), wk.begin(), wk.end());
        }
    }
    if (!weights.empty() && w.empty()) w.push_back(1);   // (no base at all: a pointer that is not null, nothing behind it is read)
    hx_wcns_out out;
    return locked_call([&](hx_ctx* ctx) { return call(ctx, f, weights.empty() ? nullptr : w.data(), &out); }, [&](hx_ctx* ctx) -> Weighted {
        Weighted res;
        res.consensus.resize(sets.size());
        if (coverage) res.coverage.resize(sets.size());
        if (profile) res.profile.resize(sets.size());
        for (std::size_t i = 0; i < sets.size(); i++) {
            res.consensus[i].assign(out.cns + out.cns_off[i], out.cns + out.cns_off[i + 1]);
            if (coverage) res.coverage[i].assign(out.coverage + out.cns_off[i], out.coverage + out.cns_off[i + 1]);
            if (profile) res.profile[i].assign(out.profile + 4 * out.cns_off[i], out.profile + 4 * out.cns_off[i + 1]);
        }
        hx_free_wcns(ctx, &out);
        return res;
    });
}
inline std::vector<const std::vector<std::vector<std::uint8_t>>*> pointers(const std::vector<std::vector<std::vector<std::uint8_t>>>& weights) {
    std::vector<const std::vector<std::vector<std::uint8_t>>*> p;
    for (const auto& ws : weights) p.push_back(&ws);
    return p;
}
}  // namespace detail
inline Weighted weighted_batch(const std::vector<const std::vector<std::string>*>& sets, const std::vector<const std::vector<std::vector<std::uint8_t>>*>& weights,
                               AlignmentType type, std::int8_t m = 5, std::int8_t n = -4, std::int8_t g = -8, std::int8_t e = -8, bool coverage = true, bool profile = false) {
    const hx_poa_weighted_params wp{m, n, g, e, static_cast<std::int32_t>(type), coverage ? 1 : 0, profile ? 1 : 0};
    return detail::weighted_call(sets, weights, coverage, profile, [&](hx_ctx* ctx, const detail::Flat& f, const std::uint8_t* w, hx_wcns_out* out) {
        return hx_poa_weighted(ctx, f.n_sets(), f.set_off.data(), f.seq_off.data(), f.bases.c_str(), w, &wp, out);
    });
}
inline Weighted weighted_batch(const std::vector<std::vector<std::string>>& sets, const std::vector<std::vector<std::vector<std::uint8_t>>>& weights, AlignmentType type,
                               std::int8_t m = 5, std::int8_t n = -4, std::int8_t g = -8, std::int8_t e = -8, bool coverage = true, bool profile = false) {
    return weighted_batch(detail::pointers(sets), detail::pointers(weights), type, m, n, g, e, coverage, profile);
}
// ... with convex gaps (hx_poa_weighted_convex): all six scores and both flags are given (no defaults: a call of nine arguments stays the
// affine form above)
inline Weighted weighted_batch(const std::vector<const std::vector<std::string>*>& sets, const std::vector<const std::vector<std::vector<std::uint8_t>>*>& weights,
                               AlignmentType type, std::int8_t m, std::int8_t n, std::int8_t g, std::int8_t e, std::int8_t q, std::int8_t c, bool coverage, bool profile) {
    const hx_poa_convex_params cp{m, n, g, e, q, c, static_cast<std::int32_t>(type)};
    return detail::weighted_call(sets, weights, coverage, profile, [&](hx_ctx* ctx, const detail::Flat& f, const std::uint8_t* w, hx_wcns_out* out) {
        return hx_poa_weighted_convex(ctx, f.n_sets(), f.set_off.data(), f.seq_off.data(), f.bases.c_str(), w, &cp, coverage ? 1 : 0, profile ? 1 : 0, out);
    });
}
inline Weighted weighted_batch(const std::vector<std::vector<std::string>>& sets, const std::vector<std::vector<std::vector<std::uint8_t>>>& weights, AlignmentType type,
                               std::int8_t m, std::int8_t n, std::int8_t g, std::int8_t e, std::int8_t q, std::int8_t c, bool coverage, bool profile) {
    return weighted_batch(detail::pointers(sets), detail::pointers(weights), type, m, n, g, e, q, c, coverage, profile);
}

// the partial-order graph of one set (hx_graph_out in haslr_types.h, one set of it): nodes in id order, edges in the order they were first
// made, per GIVEN sequence its path (the node of every base), its alignment against the graph before it was added and the score of that
// alignment's end cell, the consensus and its nodes
struct GraphData {
    std::string node_base;
    std::vector<std::uint32_t> node_rank, node_col, edge_from, edge_to;
    std::vector<std::int32_t> edge_w;
    std::vector<std::vector<std::uint32_t>> paths;
    std::vector<Alignment> alignments;
    std::vector<std::int32_t> scores;
    std::string consensus;
    std::vector<std::uint32_t> consensus_nodes;
};
// many sets in ONE device call (hx_poa_graph). weights as for weighted_batch, or empty: every weight is 1. (q, c) == (g, e) is one gap
// piece, and then e == g the linear model.
inline std::vector<GraphData> graph_batch(const std::vector<const std::vector<std::string>*>& sets, const std::vector<const std::vector<std::vector<std::uint8_t>>*>& weights,
                                          AlignmentType type, std::int8_t m = 5, std::int8_t n = -4, std::int8_t g = -8, std::int8_t e = -8, std::int8_t q = -8, std::int8_t c = -8) {
    if (!weights.empty() && weights.size() != sets.size()) throw std::invalid_argument("spoa_hx: graph_batch needs one set of weights per set of sequences, or none");
    const detail::Flat f(sets);
    std::vector<std::uint8_t> w;
    for (std::size_t i = 0; i < sets.size() && !weights.empty(); i++) {
        const auto& st = *sets[i];
        if (weights[i]->size() != st.size()) throw std::invalid_argument("spoa_hx: graph_batch: a set has another number of weight vectors than of sequences");
        for (std::size_t k = 0; k < st.size(); k++) {
            const auto& wk = (*weights[i])[k];
            if (wk.size() != st[k].size()) throw std::invalid_argument("spoa_hx: graph_batch: a sequence has another number of weights than of bases");
            w.insert(w.end(), wk.begin(), wk.end());
        }
    }
    if (!weights.empty() && w.empty()) w.push_back(1);   // (no base at all: a pointer that is not null, nothing behind it is read)
    const hx_poa_convex_params cp{m, n, g, e, q, c, static_cast<std::int32_t>(type)};
    hx_graph_out out;
    return detail::locked_call([&](hx_ctx* ctx) { return hx_poa_graph(ctx, f.n_sets(), f.set_off.data(), f.seq_off.data(), f.bases.c_str(), weights.empty() ? nullptr : w.data(), &cp, &out); },
                               [&](hx_ctx* ctx) -> std::vector<GraphData> {
        std::vector<GraphData> res(sets.size());
        for (std::size_t i = 0; i < sets.size(); i++) {
            GraphData& d = res[i];
            const std::uint64_t v0 = out.node_off[i], v1 = out.node_off[i + 1], e0 = out.edge_off[i], e1 = out.edge_off[i + 1], c0 = out.cns_off[i], c1 = out.cns_off[i + 1];
            d.node_base.assign(out.node_base + v0, out.node_base + v1);
            d.node_rank.assign(out.node_rank + v0, out.node_rank + v1); d.node_col.assign(out.node_col + v0, out.node_col + v1);
            d.edge_from.assign(out.edge_from + e0, out.edge_from + e1); d.edge_to.assign(out.edge_to + e0, out.edge_to + e1); d.edge_w.assign(out.edge_w + e0, out.edge_w + e1);
            d.consensus.assign(out.cns + c0, out.cns + c1); d.consensus_nodes.assign(out.cns_node + c0, out.cns_node + c1);
            for (std::uint64_t k = f.set_off[i]; k < f.set_off[i + 1]; k++) {
                d.paths.emplace_back(out.base_node + f.seq_off[k], out.base_node + f.seq_off[k + 1]);
                Alignment a;
                for (std::uint64_t p = out.aln_off[k]; p < out.aln_off[k + 1]; p++) a.emplace_back(out.aln_node[p], out.aln_pos[p]);
                d.alignments.push_back(std::move(a));
                d.scores.push_back(out.aln_score[k]);
            }
        }
        hx_free_graph(ctx, &out);
        return res;
    });
}
inline std::vector<GraphData> graph_batch(const std::vector<std::vector<std::string>>& sets, const std::vector<std::vector<std::vector<std::uint8_t>>>& weights, AlignmentType type,
                                          std::int8_t m = 5, std::int8_t n = -4, std::int8_t g = -8, std::int8_t e = -8, std::int8_t q = -8, std::int8_t c = -8) {
    return graph_batch(detail::pointers(sets), detail::pointers(weights), type, m, n, g, e, q, c);
}

// strand-ambiguous sets (spoa's command-line switch -s / --strand-ambiguous) in ONE device call (hx_poa_strand): every sequence after a
// set's first non-empty one is aligned to the graph as given and reverse-complemented, and the orientation with the higher end-cell score
// is added, ties forward. Per set: the consensus; per GIVEN sequence whether its reverse complement was added and the scores of the two
// orientations; with msa the rows (a reversed sequence's row is its gapped reverse complement; with include_consensus the consensus is
// the last row). weights as for weighted_batch (a reversed sequence's weights are reversed with it), or empty: every weight is 1.
// (q, c) == (g, e) is one gap piece, and then e == g the linear model.
struct Stranded {
    std::string consensus;
    std::vector<bool> reversed;
    std::vector<std::int32_t> score_forward, score_reversed;
    std::vector<std::string> rows;   // empty unless asked for
};
inline std::vector<Stranded> strand_batch(const std::vector<const std::vector<std::string>*>& sets, const std::vector<const std::vector<std::vector<std::uint8_t>>*>& weights,
                                          AlignmentType type, std::int8_t m = 5, std::int8_t n = -4, std::int8_t g = -8, std::int8_t e = -8, std::int8_t q = -8, std::int8_t c = -8,
                                          bool msa = false, bool include_consensus = false) {
    if (!weights.empty() && weights.size() != sets.size()) throw std::invalid_argument("spoa_hx: strand_batch needs one set of weights per set of sequences, or none");
    const detail::Flat f(sets);
    std::vector<std::uint8_t> w;
    for (std::size_t i = 0; i < sets.size() && !weights.empty(); i++) {
        const auto& st = *sets[i];
        if (weights[i]->size() != st.size()) throw std::invalid_argument("spoa_hx: strand_batch: a set has another number of weight vectors than of sequences");
        for (std::size_t k = 0; k < st.size(); k++) {
            const auto& wk = (*weights[i])[k];
            if (wk.size() != st[k].size()) throw std::invalid_argument("spoa_hx: strand_batch: a sequence has another number of weights than of bases");
            w.insert(w.end(), wk.begin(), wk.end());
        }
    }
    if (!weights.empty() && w.empty()) w.push_back(1);   // (no base at all: a pointer that is not null, nothing behind it is read)
    const hx_poa_convex_params cp{m, n, g, e, q, c, static_cast<std::int32_t>(type)};
    const hx_poa_strand_want want{msa ? 1 : 0, msa && include_consensus ? 1 : 0, 0, 0};
    hx_strand_out out;
    return detail::locked_call([&](hx_ctx* ctx) { return hx_poa_strand(ctx, f.n_sets(), f.set_off.data(), f.seq_off.data(), f.bases.c_str(), weights.empty() ? nullptr : w.data(), &cp, &want, &out); },
                               [&](hx_ctx* ctx) -> std::vector<Stranded> {
        std::vector<Stranded> res(sets.size());
        for (std::size_t i = 0; i < sets.size(); i++) {
            Stranded& d = res[i];
            d.consensus.assign(out.cns + out.cns_off[i], out.cns + out.cns_off[i + 1]);
            for (std::uint64_t k = f.set_off[i]; k < f.set_off[i + 1]; k++) {
                d.reversed.push_back(out.reversed[k] != 0);
                d.score_forward.push_back(out.score_fwd[k]);
                d.score_reversed.push_back(out.score_rev[k]);
            }
            if (msa)
                for (std::uint32_t r = 0; r < out.n_rows[i]; r++) {
                    const char* p = out.msa + out.msa_off[i] + static_cast<std::uint64_t>(r) * out.n_cols[i];
                    d.rows.emplace_back(p, p + out.n_cols[i]);
                }
        }
        hx_free_strand(ctx, &out);
        return res;
    });
}
inline std::vector<Stranded> strand_batch(const std::vector<std::vector<std::string>>& sets, const std::vector<std::vector<std::vector<std::uint8_t>>>& weights, AlignmentType type,
                                          std::int8_t m = 5, std::int8_t n = -4, std::int8_t g = -8, std::int8_t e = -8, std::int8_t q = -8, std::int8_t c = -8, bool msa = false,
                                          bool include_consensus = false) {
    return strand_batch(detail::pointers(sets), detail::pointers(weights), type, m, n, g, e, q, c, msa, include_consensus);
}

// banded sets in ONE device call (hx_poa_banded): every alignment runs inside an adaptive band of half-width `band` (1..511), a set that
// misses its band is run again with twice the band and at last on the full matrix. Per set: the consensus, the half-width of the attempt
// that gave it (0: the full matrix), and with msa the rows (with include_consensus the consensus is the last row). weights as for
// weighted_batch, or empty: every weight is 1. (q, c) == (g, e) is one gap piece, and then e == g the linear model.
struct Banded {
    std::string consensus;
    std::uint32_t band_used = 0;
    std::vector<std::string> rows;   // empty unless asked for
};
inline std::vector<Banded> banded_batch(const std::vector<const std::vector<std::string>*>& sets, const std::vector<const std::vector<std::vector<std::uint8_t>>*>& weights,
                                        std::uint32_t band, AlignmentType type, std::int8_t m = 5, std::int8_t n = -4, std::int8_t g = -8, std::int8_t e = -8, std::int8_t q = -8,
                                        std::int8_t c = -8, bool msa = false, bool include_consensus = false) {
    if (!weights.empty() && weights.size() != sets.size()) throw std::invalid_argument("spoa_hx: banded_batch needs one set of weights per set of sequences, or none");
    const detail::Flat f(sets);
    std::vector<std::uint8_t> w;
    for (std::size_t i = 0; i < sets.size() && !weights.empty(); i++) {
        const auto& st = *sets[i];
        if (weights[i]->size() != st.size()) throw std::invalid_argument("spoa_hx: banded_batch: a set has another number of weight vectors than of sequences");
        for (std::size_t k = 0; k < st.size(); k++) {
            const auto& wk = (*weights[i])[k];
            if (wk.size() != st[k].size()) throw std::invalid_argument("spoa_hx: banded_batch: a sequence has another number of weights than of bases");
            w.insert(w.end(), wk.begin(), wk.end());
        }
    }
    if (!weights.empty() && w.empty()) w.push_back(1);   // (no base at all: a pointer that is not null, nothing behind it is read)
    const hx_poa_convex_params cp{m, n, g, e, q, c, static_cast<std::int32_t>(type)};
    const hx_poa_band_params bp{band, msa ? 1 : 0, msa && include_consensus ? 1 : 0, 0, 0};
    hx_band_out out;
    return detail::locked_call([&](hx_ctx* ctx) { return hx_poa_banded(ctx, f.n_sets(), f.set_off.data(), f.seq_off.data(), f.bases.c_str(), weights.empty() ? nullptr : w.data(), &cp, &bp, &out); },
                               [&](hx_ctx* ctx) -> std::vector<Banded> {
        std::vector<Banded> res(sets.size());
        for (std::size_t i = 0; i < sets.size(); i++) {
            Banded& d = res[i];
            d.consensus.assign(out.cns + out.cns_off[i], out.cns + out.cns_off[i + 1]);
            d.band_used = out.band_used[i];
            if (msa)
                for (std::uint32_t r = 0; r < out.n_rows[i]; r++) {
                    const char* p = out.msa + out.msa_off[i] + static_cast<std::uint64_t>(r) * out.n_cols[i];
                    d.rows.emplace_back(p, p + out.n_cols[i]);
                }
        }
        hx_free_band(ctx, &out);
        return res;
    });
}
inline std::vector<Banded> banded_batch(const std::vector<std::vector<std::string>>& sets, const std::vector<std::vector<std::vector<std::uint8_t>>>& weights, std::uint32_t band,
                                        AlignmentType type, std::int8_t m = 5, std::int8_t n = -4, std::int8_t g = -8, std::int8_t e = -8, std::int8_t q = -8, std::int8_t c = -8,
                                        bool msa = false, bool include_consensus = false) {
    return banded_batch(detail::pointers(sets), detail::pointers(weights), band, type, m, n, g, e, q, c, msa, include_consensus);
}

// labelled sets in ONE device call (hx_poa_labelled): every sequence carries a label 0 .. n_labels - 1 (or 255: none), the graph of a set
// is built from all of its sequences as weighted_batch builds it, and every label gets the consensus of the edges its own sequences walk,
// weighed by those sequences alone. Per set and label: the consensus and the MSA column of every one of its bases (the columns are the
// set's, shared by its labels); with msa the rows (with include_consensus one consensus row per label behind the sequences' rows).
// weights as for weighted_batch, or empty: every weight is 1. (q, c) == (g, e) is one gap piece, and then e == g the linear model.
struct Labelled {
    std::vector<std::string> consensus;                 // one per label
    std::vector<std::vector<std::uint32_t>> columns;    // one per label: the column of every consensus base
    std::vector<std::string> rows;                      // empty unless asked for
};
inline std::vector<Labelled> labelled_batch(const std::vector<const std::vector<std::string>*>& sets, const std::vector<const std::vector<std::vector<std::uint8_t>>*>& weights,
                                            const std::vector<std::vector<std::uint8_t>>& labels, std::uint32_t n_labels, AlignmentType type, std::int8_t m = 5, std::int8_t n = -4,
                                            std::int8_t g = -8, std::int8_t e = -8, std::int8_t q = -8, std::int8_t c = -8, bool msa = false, bool include_consensus = false) {
    if (!weights.empty() && weights.size() != sets.size()) throw std::invalid_argument("spoa_hx: labelled_batch needs one set of weights per set of sequences, or none");
    if (labels.size() != sets.size()) throw std::invalid_argument("spoa_hx: labelled_batch needs one set of labels per set of sequences");
    const detail::Flat f(sets);
    std::vector<std::uint8_t> w, lb;
    for (std::size_t i = 0; i < sets.size(); i++) {
        const auto& st = *sets[i];
        if (labels[i].size() != st.size()) throw std::invalid_argument("spoa_hx: labelled_batch: a set has another number of labels than of sequences");
        lb.insert(lb.end(), labels[i].begin(), labels[i].end());
        if (weights.empty()) continue;
        if (weights[i]->size() != st.size()) throw std::invalid_argument("spoa_hx: labelled_batch: a set has another number of weight vectors than of sequences");
        for (std::size_t k = 0; k < st.size(); k++) {
            const auto& wk = (*weights[i])[k];
            if (wk.size() != st[k].size()) throw std::invalid_argument("spoa_hx: labelled_batch: a sequence has another number of weights than of bases");
            w.insert(w.end(), wk.begin(), wk.end());
        }
    }
    if (!weights.empty() && w.empty()) w.push_back(1);   // (no base at all: a pointer that is not null, nothing behind it is read)
    if (lb.empty()) lb.push_back(255);                   // (no sequence at all: the same)
    const hx_poa_convex_params cp{m, n, g, e, q, c, static_cast<std::int32_t>(type)};
    const hx_poa_label_params lp{n_labels, msa ? 1 : 0, msa && include_consensus ? 1 : 0, 0, 0};
    hx_label_out out;
    return detail::locked_call([&](hx_ctx* ctx) { return hx_poa_labelled(ctx, f.n_sets(), f.set_off.data(), f.seq_off.data(), f.bases.c_str(), weights.empty() ? nullptr : w.data(), lb.data(), &cp, &lp, &out); },
                               [&](hx_ctx* ctx) -> std::vector<Labelled> {
        std::vector<Labelled> res(sets.size());
        for (std::size_t i = 0; i < sets.size(); i++) {
            Labelled& d = res[i];
            for (std::uint32_t l = 0; l < n_labels; l++) {
                const std::uint64_t a = out.cns_off[i * n_labels + l], b = out.cns_off[i * n_labels + l + 1];
                d.consensus.emplace_back(out.cns + a, out.cns + b);
                d.columns.emplace_back(out.cns_col + a, out.cns_col + b);
            }
            if (msa)
                for (std::uint32_t r = 0; r < out.n_rows[i]; r++) {
                    const char* p = out.msa + out.msa_off[i] + static_cast<std::uint64_t>(r) * out.n_cols[i];
                    d.rows.emplace_back(p, p + out.n_cols[i]);
                }
        }
        hx_free_label(ctx, &out);
        return res;
    });
}
inline std::vector<Labelled> labelled_batch(const std::vector<std::vector<std::string>>& sets, const std::vector<std::vector<std::vector<std::uint8_t>>>& weights,
                                            const std::vector<std::vector<std::uint8_t>>& labels, std::uint32_t n_labels, AlignmentType type, std::int8_t m = 5, std::int8_t n = -4,
                                            std::int8_t g = -8, std::int8_t e = -8, std::int8_t q = -8, std::int8_t c = -8, bool msa = false, bool include_consensus = false) {
    return labelled_batch(detail::pointers(sets), detail::pointers(weights), labels, n_labels, type, m, n, g, e, q, c, msa, include_consensus);
}

// two-haplotype consensus in ONE device call (hx_poa_phased): the graph of a set is built from all of its sequences as weighted_batch
// builds it, the call itself splits the reads on the heterozygous MSA columns (min_count, min_pct: how often and in what share of a
// column's depth the second allele must be seen) and every haplotype gets labelled_batch's consensus for its reads. Per set: the haplotype
// of every read (0, 1, 255: none), n_haps (1: left unphased, everything in haplotype 0), the voting rounds, the sites, and per haplotype
// what Labelled holds. weights as for weighted_batch, or empty: every weight is 1. (q, c) == (g, e) is one gap piece, and then e == g the
// linear model.
struct PhaseSite { std::uint32_t column; std::uint8_t a1, a2; std::int8_t phase; };   // alleles 0..3 A C G T, 4 a gap; phase +1: haplotype 0 carries a1
struct Phased {
    std::vector<std::uint8_t> hap;                      // one per sequence
    std::uint32_t n_haps = 0, rounds = 0;
    std::vector<PhaseSite> sites;
    std::vector<std::string> consensus;                 // one per haplotype (two entries; the second empty in an unphased set)
    std::vector<std::vector<std::uint32_t>> columns;    // one per haplotype: the column of every consensus base
    std::vector<std::string> rows;                      // empty unless asked for
};
inline std::vector<Phased> phased_batch(const std::vector<const std::vector<std::string>*>& sets, const std::vector<const std::vector<std::vector<std::uint8_t>>*>& weights,
                                        AlignmentType type, std::int8_t m = 5, std::int8_t n = -4, std::int8_t g = -8, std::int8_t e = -8, std::int8_t q = -8, std::int8_t c = -8,
                                        std::uint32_t min_count = 2, std::uint32_t min_pct = 25, bool msa = false, bool include_consensus = false) {
    if (!weights.empty() && weights.size() != sets.size()) throw std::invalid_argument("spoa_hx: phased_batch needs one set of weights per set of sequences, or none");
    const detail::Flat f(sets);
    std::vector<std::uint8_t> w;
    for (std::size_t i = 0; i < sets.size() && !weights.empty(); i++) {
        const auto& st = *sets[i];
        if (weights[i]->size() != st.size()) throw std::invalid_argument("spoa_hx: phased_batch: a set has another number of weight vectors than of sequences");
        for (std::size_t k = 0; k < st.size(); k++) {
            const auto& wk = (*weights[i])[k];
            if (wk.size() != st[k].size()) throw std::invalid_argument("spoa_hx: phased_batch: a sequence has another number of weights than of bases");
            w.insert(w.end(), wk.begin(), wk.end());
        }
    }
    if (!weights.empty() && w.empty()) w.push_back(1);   // (no base at all: a pointer that is not null, nothing behind it is read)
    const hx_poa_convex_params cp{m, n, g, e, q, c, static_cast<std::int32_t>(type)};
    const hx_poa_phase_params pp{min_count, min_pct, msa ? 1 : 0, msa && include_consensus ? 1 : 0, 0, 0};
    hx_phase_out out;
    return detail::locked_call([&](hx_ctx* ctx) { return hx_poa_phased(ctx, f.n_sets(), f.set_off.data(), f.seq_off.data(), f.bases.c_str(), weights.empty() ? nullptr : w.data(), &cp, &pp, &out); },
                               [&](hx_ctx* ctx) -> std::vector<Phased> {
        std::vector<Phased> res(sets.size());
        for (std::size_t i = 0; i < sets.size(); i++) {
            Phased& d = res[i];
            d.hap.assign(out.hap + f.set_off[i], out.hap + f.set_off[i + 1]);
            d.n_haps = out.n_haps[i]; d.rounds = out.rounds[i];
            for (std::uint64_t s = out.site_off[i]; s < out.site_off[i + 1]; s++) d.sites.push_back(PhaseSite{out.site_col[s], out.site_a1[s], out.site_a2[s], out.site_phase[s]});
            for (std::uint32_t l = 0; l < 2; l++) {
                const std::uint64_t a = out.cns_off[i * 2 + l], b = out.cns_off[i * 2 + l + 1];
                d.consensus.emplace_back(out.cns + a, out.cns + b);
                d.columns.emplace_back(out.cns_col + a, out.cns_col + b);
            }
            if (msa)
                for (std::uint32_t r = 0; r < out.n_rows[i]; r++) {
                    const char* p = out.msa + out.msa_off[i] + static_cast<std::uint64_t>(r) * out.n_cols[i];
                    d.rows.emplace_back(p, p + out.n_cols[i]);
                }
        }
        hx_free_phase(ctx, &out);
        return res;
    });
}
inline std::vector<Phased> phased_batch(const std::vector<std::vector<std::string>>& sets, const std::vector<std::vector<std::vector<std::uint8_t>>>& weights, AlignmentType type,
                                        std::int8_t m = 5, std::int8_t n = -4, std::int8_t g = -8, std::int8_t e = -8, std::int8_t q = -8, std::int8_t c = -8,
                                        std::uint32_t min_count = 2, std::uint32_t min_pct = 25, bool msa = false, bool include_consensus = false) {
    return phased_batch(detail::pointers(sets), detail::pointers(weights), type, m, n, g, e, q, c, min_count, min_pct, msa, include_consensus);
}

// Graphviz text of a graph, after spoa's Graph::print_dot: per node `id [label = "id - LETTER"]`, filled for the nodes of the consensus;
// per out-edge, in out-list order, `from -> to [label = "weight"]`; one dotted line without arrowhead per pair of aligned nodes (nodes that
// share a column), from the smaller to the larger id
inline std::string to_dot(const GraphData& d) {
    const std::size_t V = d.node_base.size();
    std::vector<char> in_cns(V, 0);
    for (std::uint32_t nd : d.consensus_nodes) in_cns[nd] = 1;
    std::vector<std::vector<std::size_t>> outs(V);
    for (std::size_t e = 0; e < d.edge_from.size(); e++) outs[d.edge_from[e]].push_back(e);
    std::map<std::uint32_t, std::vector<std::size_t>> by_col;
    for (std::size_t nd = 0; nd < V; nd++) by_col[d.node_col[nd]].push_back(nd);
    std::size_t n_seq = 0;
    for (const auto& p : d.paths) n_seq += !p.empty();
    std::string s = "digraph " + std::to_string(n_seq) + " {\n    graph [rankdir = LR]\n";
    for (std::size_t nd = 0; nd < V; nd++) {
        s += "    " + std::to_string(nd) + " [label = \"" + std::to_string(nd) + " - " + d.node_base[nd] + "\"" + (in_cns[nd] ? ", style = filled, fillcolor = goldenrod1]\n" : "]\n");
        for (std::size_t e : outs[nd]) s += "    " + std::to_string(nd) + " -> " + std::to_string(d.edge_to[e]) + " [label = \"" + std::to_string(d.edge_w[e]) + "\"]\n";
        for (std::size_t a : by_col[d.node_col[nd]]) if (a > nd) s += "    " + std::to_string(nd) + " -> " + std::to_string(a) + " [style = dotted, arrowhead = none]\n";
    }
    return s + "}\n";
}
// GFA 1 text of a graph: `H VN:Z:1.0`; one S line per node (name = id + 1, the letter, tags rk:i: rank and cl:i: column); one L line per
// edge in edge-id order (+ / +, overlap 0M, tag ew:i: weight); one P line per non-empty sequence, named by names[k] or s<k> (k counts the
// given sequences from 0), and one P line `consensus`
inline std::string to_gfa(const GraphData& d, const std::vector<std::string>& names = std::vector<std::string>()) {
    std::string s = "H\tVN:Z:1.0\n";
    for (std::size_t nd = 0; nd < d.node_base.size(); nd++)
        s += "S\t" + std::to_string(nd + 1) + "\t" + d.node_base[nd] + "\trk:i:" + std::to_string(d.node_rank[nd]) + "\tcl:i:" + std::to_string(d.node_col[nd]) + "\n";
    for (std::size_t e = 0; e < d.edge_from.size(); e++)
        s += "L\t" + std::to_string(d.edge_from[e] + 1) + "\t+\t" + std::to_string(d.edge_to[e] + 1) + "\t+\t0M\tew:i:" + std::to_string(d.edge_w[e]) + "\n";
    auto p_line = [&s](const std::string& name, const std::vector<std::uint32_t>& nodes) {
        s += "P\t" + name + "\t";
        for (std::size_t i = 0; i < nodes.size(); i++) s += (i ? "," : "") + std::to_string(nodes[i] + 1) + "+";
        s += "\t";
        for (std::size_t i = 1; i < nodes.size(); i++) s += i > 1 ? ",0M" : "0M";
        s += nodes.size() < 2 ? "*\n" : "\n";
    };
    for (std::size_t k = 0; k < d.paths.size(); k++)
        if (!d.paths[k].empty()) p_line(k < names.size() ? names[k] : "s" + std::to_string(k), d.paths[k]);
    if (!d.consensus_nodes.empty()) p_line("consensus", d.consensus_nodes);
    return s;
}

// one set on behalf of one caller thread, combined with whatever other threads have queued (see "Threads" above)
inline std::string consensus_combined(const std::vector<std::string>& seqs, AlignmentType type, std::int8_t m, std::int8_t n, std::int8_t g, std::int8_t e, std::int8_t q, std::int8_t c) {
    Device& d = device();
    static const long window_us = std::getenv("HASLR_SPOA_BATCH_US") ? std::atol(std::getenv("HASLR_SPOA_BATCH_US")) : 200;
    static const std::size_t batch_max = std::getenv("HASLR_SPOA_BATCH") ? (std::size_t)std::max(1L, std::atol(std::getenv("HASLR_SPOA_BATCH"))) : 256;
    Device::Request me{&seqs, type, m, n, g, e, q, c, std::string(), std::string(), false, false};
    std::unique_lock<std::mutex> lk(d.qmu);
    d.queue.push_back(&me);
    d.arrivals++;
    d.qcv.notify_all();                                        // (a submitter that is collecting counts the queue)
    while (!me.done) {
        if (d.submitting) { d.qcv.wait(lk); continue; }         // somebody else submits: my request rides along, or waits for the next batch
        d.submitting = true;                                    // I submit: collect for the window, then take everything queued
        std::vector<Device::Request*> batch;
        // Whatever goes wrong from here on (an allocation that throws as well), `submitting` is reset, the requests taken so far are answered (with
        // the error) and the waiters are woken: no thread may be left waiting on a submitter that is gone.
        try {
            // The window is for company: a lone caller (the reference with -t 1, or the only thread that still has edges) would sit through it on
            // every call for nothing. It is waited out only when somebody else has been seen since the previous batch closed (d.company), or is
            // queued right now.
            if (d.company || d.queue.size() > 1) {
                const auto until = std::chrono::steady_clock::now() + std::chrono::microseconds(window_us);
                while (d.queue.size() < batch_max && d.qcv.wait_until(lk, until) != std::cv_status::timeout) { }
            }
            batch.swap(d.queue);
            if (batch.size() > batch_max) { d.queue.assign(batch.begin() + (std::ptrdiff_t)batch_max, batch.end()); batch.resize(batch_max); }
            d.arrivals = d.queue.size();                           // arrivals from here on = company for the next submitter
            lk.unlock();
            // one device call per (alignment type, six scores) in the batch (the reference uses one of each)
            std::vector<char> served(batch.size(), 0);
            std::uint64_t calls = 0;
            for (std::size_t i = 0; i < batch.size(); i++) {
                if (served[i]) continue;
                std::vector<std::size_t> idx;
                std::vector<const std::vector<std::string>*> sets;
                for (std::size_t j = i; j < batch.size(); j++)
                    if (!served[j] && batch[j]->type == batch[i]->type && batch[j]->m == batch[i]->m && batch[j]->n == batch[i]->n && batch[j]->g == batch[i]->g && batch[j]->e == batch[i]->e && batch[j]->q == batch[i]->q && batch[j]->c == batch[i]->c) { idx.push_back(j); sets.push_back(batch[j]->seqs); served[j] = 1; }
                try {
                    std::vector<std::string> res = consensus_batch(sets, batch[i]->type, batch[i]->m, batch[i]->n, batch[i]->g, batch[i]->e, batch[i]->q, batch[i]->c);
                    for (std::size_t q = 0; q < idx.size(); q++) { batch[idx[q]]->result.swap(res[q]); batch[idx[q]]->answered = true; }
                    calls++;
                } catch (const std::exception& e) {
                    // one bad set must not fail the callers that happened to share its launch: every set of the group again, on its own - until two in a
                    // row have failed the way the whole group did (a device fault is sticky: the other 250 sets would fail one call at a time)
                    const std::string group_error = e.what();
                    if (idx.size() == 1) { batch[idx[0]]->error = group_error; batch[idx[0]]->answered = true; }
                    else {
                        int same = 0;
                        for (std::size_t q = 0; q < idx.size(); q++) {
                            Device::Request* r = batch[idx[q]];
                            if (same >= 2) { r->error = group_error; r->answered = true; continue; }
                            try { r->result = consensus_batch(std::vector<const std::vector<std::string>*>{sets[q]}, batch[i]->type, batch[i]->m, batch[i]->n, batch[i]->g, batch[i]->e, batch[i]->q, batch[i]->c)[0]; same = 0; }
                            catch (const std::exception& e1) { r->error = e1.what(); same = r->error == group_error ? same + 1 : 0; }
                            r->answered = true;
                            calls++;
                        }
                    }
                    calls++;
                }
            }
            lk.lock();
            d.calls += calls; d.sets += batch.size();
        } catch (...) {
            if (!lk.owns_lock()) lk.lock();
            // requests of the batch that have no answer yet get the error (an EMPTY consensus that was served is an answer and stays)
            for (Device::Request* r : batch) if (!r->answered) { r->error = "spoa_hx: the submitting thread failed before the device call (out of memory?)"; r->answered = true; }
            if (batch.empty()) {   // failed while collecting: nothing was taken - this caller gets the error and leaves the queue
                me.error = "spoa_hx: the submitting thread failed while collecting a batch (out of memory?)";
                for (std::size_t q = 0; q < d.queue.size(); q++) if (d.queue[q] == &me) { d.queue.erase(d.queue.begin() + (std::ptrdiff_t)q); break; }
                me.done = true;
            }
            // (a batch cut at batch_max may have left this caller's own request in the queue: it stays there for the next submitter - possibly this thread)
        }
        for (Device::Request* r : batch) r->done = true;
        d.company = batch.size() > 1 || d.arrivals > 0;         // did this batch have, or did its device call see, anybody else?
        d.submitting = false;
        d.qcv.notify_all();
    }
    lk.unlock();
    if (!me.error.empty()) throw std::runtime_error(me.error);
    return me.result;
}

inline std::string consensus_combined(const std::vector<std::string>& seqs, AlignmentType type, std::int8_t m, std::int8_t n, std::int8_t g, std::int8_t e) {
    return consensus_combined(seqs, type, m, n, g, e, g, e);   // one gap piece
}
inline std::string consensus_combined(const std::vector<std::string>& seqs, AlignmentType type, std::int8_t m, std::int8_t n, std::int8_t g) {
    return consensus_combined(seqs, type, m, n, g, g);   // linear gap
}

}  // namespace hx

class Graph {
public:
    // spoa::Graph::add_alignment(alignment, sequence, weight = 1): the same weight for every base
    void add_alignment(const Alignment& alignment, const std::string& sequence, std::uint32_t weight = 1) {
        if (weight < 1 || weight > 255) throw std::invalid_argument("spoa_hx: a weight must be 1..255, not " + std::to_string(weight));
        record(alignment, sequence, std::vector<std::uint8_t>(sequence.size(), (std::uint8_t)weight));
    }
    // spoa::Graph::add_alignment(alignment, sequence, quality): weight = quality character - 33
    void add_alignment(const Alignment& alignment, const std::string& sequence, const std::string& quality) {
        if (quality.size() != sequence.size()) throw std::invalid_argument("spoa_hx: the quality string has " + std::to_string(quality.size()) + " characters, the sequence " + std::to_string(sequence.size()) + " bases");
        std::vector<std::uint8_t> w(quality.size());
        for (std::size_t i = 0; i < quality.size(); i++) {
            const int v = (int)(unsigned char)quality[i] - 33;
            if (v < 1 || v > 93) throw std::invalid_argument("spoa_hx: the quality character at position " + std::to_string(i) + " gives the weight " + std::to_string(v) + " (accepted: '\"'..'~', weights 1..93)");
            w[i] = (std::uint8_t)v;
        }
        record(alignment, sequence, w);
    }
    // spoa::Graph::add_alignment(alignment, sequence, weights): one weight per base
    void add_alignment(const Alignment& alignment, const std::string& sequence, const std::vector<std::uint32_t>& weights) {
        if (weights.size() != sequence.size()) throw std::invalid_argument("spoa_hx: " + std::to_string(weights.size()) + " weights for a sequence of " + std::to_string(sequence.size()) + " bases");
        std::vector<std::uint8_t> w(weights.size());
        for (std::size_t i = 0; i < weights.size(); i++) {
            if (weights[i] < 1 || weights[i] > 255) throw std::invalid_argument("spoa_hx: the weight at position " + std::to_string(i) + " is " + std::to_string(weights[i]) + " (accepted: 1..255)");
            w[i] = (std::uint8_t)weights[i];
        }
        record(alignment, sequence, w);
    }
    // spoa::Graph::generate_consensus()
    std::string generate_consensus() {
        if (sequences_.empty()) return std::string();
        if (!weighted_) return hx::consensus_combined(sequences_, type_, m_, n_, g_, e_, q_, c_);
        return weighted(true, false).consensus[0];
    }
    // spoa::Graph::generate_consensus(dst): dst is replaced by the coverage of every consensus base. A device call of its own.
    std::string generate_consensus(std::vector<std::uint32_t>& dst) {
        dst.clear();
        if (sequences_.empty()) return std::string();
        hx::Weighted r = weighted(weighted_, true);
        dst.swap(r.coverage[0]);
        return r.consensus[0];
    }
    // spoa::Graph::generate_multiple_sequence_alignment(dst, include_consensus = false): dst is replaced by one row per added sequence
    // (and the consensus row). A device call of its own, not combined with other threads' calls.
    void generate_multiple_sequence_alignment(std::vector<std::string>& dst, bool include_consensus = false) {
        dst.clear();
        if (sequences_.empty()) return;
        const std::vector<const std::vector<std::string>*> one{&sequences_};
        dst = std::move((convex() ? hx::msa_batch(one, type_, m_, n_, g_, e_, q_, c_, include_consensus) : hx::msa_batch(one, type_, m_, n_, g_, e_, include_consensus))[0]);
    }

    // the graph of the recorded sequences (their weights count): a device call of its own, like the MSA. A graph without sequences needs no device.
    hx::GraphData data() const {
        if (sequences_.empty()) return hx::GraphData();
        const std::vector<const std::vector<std::string>*> one{&sequences_};
        const std::vector<const std::vector<std::vector<std::uint8_t>>*> w = weighted_ ? std::vector<const std::vector<std::vector<std::uint8_t>>*>{&weights_} : std::vector<const std::vector<std::vector<std::uint8_t>>*>{};
        return std::move(hx::graph_batch(one, w, type_, m_, n_, g_, e_, q_, c_)[0]);
    }
    // spoa::Graph::print_dot(path): the graph as Graphviz text (hx::to_dot); an empty path does nothing, as in spoa
    void print_dot(const std::string& path) const {
        if (path.empty()) return;
        write(path, hx::to_dot(data()));
    }
    // the graph as GFA 1 (hx::to_gfa; the sequences are named s0, s1, ... in the order they were added)
    void print_gfa(const std::string& path) const {
        if (path.empty()) return;
        write(path, hx::to_gfa(data()));
    }
    // the real Alignment of the k-th added sequence (empty ones, which add_alignment ignores, do not count): spoa's pairs against the graph
    // as it was before that sequence was added. The first sequence has none.
    Alignment alignment(std::size_t k) const {
        if (k >= sequences_.size()) throw std::out_of_range("spoa_hx: alignment(" + std::to_string(k) + ") of a graph with " + std::to_string(sequences_.size()) + " sequences");
        return data().alignments[k];
    }

private:
    friend class AlignmentEngine;
    static void write(const std::string& path, const std::string& text) {
        std::ofstream out(path.c_str(), std::ios::binary);
        out << text;
        if (!out) throw std::runtime_error("spoa_hx: cannot write " + path);
    }
    bool convex() const { return q_ != g_ || c_ != e_; }   // a seven-score engine whose second piece is not the first again
    // this graph's one set through the weighted entry of its gap model (with its weights, or on unit weights)
    hx::Weighted weighted(bool with_weights, bool coverage) const {
        const std::vector<const std::vector<std::string>*> one{&sequences_};
        const std::vector<const std::vector<std::vector<std::uint8_t>>*> w = with_weights ? std::vector<const std::vector<std::vector<std::uint8_t>>*>{&weights_} : std::vector<const std::vector<std::vector<std::uint8_t>>*>{};
        return convex() ? hx::weighted_batch(one, w, type_, m_, n_, g_, e_, q_, c_, coverage, false) : hx::weighted_batch(one, w, type_, m_, n_, g_, e_, coverage, false);
    }
    void record(const Alignment& alignment, const std::string& sequence, const std::vector<std::uint8_t>& w) {
        if (alignment.size() != 1 || alignment[0].first != -1 || (std::uint32_t)alignment[0].second != ticket_)
            throw std::invalid_argument("spoa_hx: add_alignment needs the alignment that align_sequence_with_graph last returned for this graph");
        ticket_++;
        if (sequence.empty()) return;   // spoa ignores an empty sequence (the reference never passes one, Assemble.cpp:537)
        sequences_.push_back(sequence);
        weights_.push_back(w);
        for (std::uint8_t v : w) if (v != 1) weighted_ = true;
    }
    std::vector<std::string> sequences_;
    std::vector<std::vector<std::uint8_t>> weights_;   // parallel to sequences_
    bool weighted_ = false;                            // some base has another weight than 1
    std::uint32_t ticket_ = 0;
    AlignmentType type_ = AlignmentType::kNW;
    std::int8_t m_ = 5, n_ = -4, g_ = -8, e_ = -8, q_ = -8, c_ = -8;   // (q, c) == (g, e): one gap piece
};

class AlignmentEngine {
public:
    // spoa::AlignmentEngine::align_sequence_with_graph(sequence, graph): a token for add_alignment (see the header comment)
    Alignment align_sequence_with_graph(const std::string& /*sequence*/, const std::unique_ptr<Graph>& graph) {
        graph->type_ = type_; graph->m_ = m_; graph->n_ = n_; graph->g_ = g_; graph->e_ = e_; graph->q_ = q_; graph->c_ = c_;
        return Alignment{{-1, (std::int32_t)graph->ticket_}};
    }

private:
    friend std::unique_ptr<AlignmentEngine> createAlignmentEngine(AlignmentType, std::int8_t, std::int8_t, std::int8_t);
    friend std::unique_ptr<AlignmentEngine> createAlignmentEngine(AlignmentType, std::int8_t, std::int8_t, std::int8_t, std::int8_t);
    friend std::unique_ptr<AlignmentEngine> createAlignmentEngine(AlignmentType, std::int8_t, std::int8_t, std::int8_t, std::int8_t, std::int8_t, std::int8_t);
    AlignmentEngine(AlignmentType type, std::int8_t m, std::int8_t n, std::int8_t g, std::int8_t e, std::int8_t q, std::int8_t c) : type_(type), m_(m), n_(n), g_(g), e_(e), q_(q), c_(c) {}
    AlignmentType type_;
    std::int8_t m_, n_, g_, e_, q_, c_;
};

// spoa::createAlignmentEngine(type, match, mismatch, gap) — linear gap penalties, as spoa 1.1.3 has them
inline std::unique_ptr<AlignmentEngine> createAlignmentEngine(AlignmentType type, std::int8_t m, std::int8_t n, std::int8_t g) {
    if (type != AlignmentType::kSW && type != AlignmentType::kNW && type != AlignmentType::kOV) throw std::invalid_argument("spoa_hx: unknown AlignmentType");
    if (g >= 0) throw std::invalid_argument("spoa_hx: the gap penalty must be negative");
    return std::unique_ptr<AlignmentEngine>(new AlignmentEngine(type, m, n, g, g, g, g));
}
// spoa::createAlignmentEngine(type, match, mismatch, gap_open, gap_extend) — affine gap penalties: a gap of k bases costs g + (k - 1) e.
// e == g is the linear engine above. e < g is refused: what spoa does with such scores cannot be checked here, so nothing is guessed.
inline std::unique_ptr<AlignmentEngine> createAlignmentEngine(AlignmentType type, std::int8_t m, std::int8_t n, std::int8_t g, std::int8_t e) {
    if (type != AlignmentType::kSW && type != AlignmentType::kNW && type != AlignmentType::kOV) throw std::invalid_argument("spoa_hx: unknown AlignmentType");
    if (g >= 0) throw std::invalid_argument("spoa_hx: the gap open penalty must be negative");
    if (e > 0) throw std::invalid_argument("spoa_hx: the gap extend penalty must not be positive");
    if (e < g) throw std::invalid_argument("spoa_hx: the gap extend penalty must not be below the gap open penalty");
    return std::unique_ptr<AlignmentEngine>(new AlignmentEngine(type, m, n, g, e, g, e));
}
// spoa::createAlignmentEngine(type, match, mismatch, gap_open, gap_extend, gap_open2, gap_extend2) - two-piece affine (convex) gap
// penalties: a gap of k bases costs max(g + (k - 1) e, q + (k - 1) c). Each piece is a valid affine one and q <= g (the first piece is the
// one that opens no dearer); anything else is refused, not reinterpreted. c <= e: the second piece never wins, the engine is the
// five-score one with (g, e).
inline std::unique_ptr<AlignmentEngine> createAlignmentEngine(AlignmentType type, std::int8_t m, std::int8_t n, std::int8_t g, std::int8_t e, std::int8_t q, std::int8_t c) {
    if (type != AlignmentType::kSW && type != AlignmentType::kNW && type != AlignmentType::kOV) throw std::invalid_argument("spoa_hx: unknown AlignmentType");
    if (g >= 0) throw std::invalid_argument("spoa_hx: the gap open penalty must be negative, not " + std::to_string((int)g));
    if (e > 0) throw std::invalid_argument("spoa_hx: the gap extend penalty must not be positive, not " + std::to_string((int)e));
    if (e < g) throw std::invalid_argument("spoa_hx: the gap extend penalty " + std::to_string((int)e) + " must not be below the gap open penalty " + std::to_string((int)g));
    if (q >= 0) throw std::invalid_argument("spoa_hx: the second gap open penalty must be negative, not " + std::to_string((int)q));
    if (c > 0) throw std::invalid_argument("spoa_hx: the second gap extend penalty must not be positive, not " + std::to_string((int)c));
    if (c < q) throw std::invalid_argument("spoa_hx: the second gap extend penalty " + std::to_string((int)c) + " must not be below the second gap open penalty " + std::to_string((int)q));
    if (q > g) throw std::invalid_argument("spoa_hx: the second gap open penalty " + std::to_string((int)q) + " must not be above the first gap open penalty " + std::to_string((int)g));
    if (c <= e) return std::unique_ptr<AlignmentEngine>(new AlignmentEngine(type, m, n, g, e, g, e));
    return std::unique_ptr<AlignmentEngine>(new AlignmentEngine(type, m, n, g, e, q, c));
}
inline std::unique_ptr<Graph> createGraph() { return std::unique_ptr<Graph>(new Graph()); }

}  // namespace spoa
#endif
