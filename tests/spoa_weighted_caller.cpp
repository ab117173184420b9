// Test program for the weights and coverage side of include/spoa_hx.hpp: a caller in spoa's own call pattern (one engine + one graph per
// edge, sequences aligned and added one after the other) that uses the three add_alignment overloads and generate_consensus(dst), mixed
// with plain unit-weight graphs in one process.
// Input: edges separated by blank lines; the first line of an edge is "type" (a four-score engine with 5 -4 -8) or
// "type match mismatch gap_open gap_extend" (a five-score engine), type = sw, nw or ov, optionally followed by "+cov" (ask for the
// coverage: generate_consensus(dst)); every other line is a sequence ("-": an empty one), alone (add_alignment(alignment, sequence)) or
// followed by "w N" (one weight), "q QUALITIES" (a quality string) or "v w1,w2,.." (a vector of weights).
// Output per edge: its consensus, then its coverage (numbers separated by blanks; "-" when it was not asked for), then a line "=".
// --threads N deals the edges to N threads (default 1); --batch sends the edges of each kind through spoa::hx::weighted_batch instead
// (empty members dropped; the coverage of every edge is printed); --throws checks what the header refuses and prints "throws ok".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#include "spoa_hx.hpp"

struct Kind {
    std::string type;
    bool affine = false, cov = false;
    int m = 5, n = -4, g = -8, e = -8;
    bool operator<(const Kind& o) const { return std::tie(type, m, n, g, e) < std::tie(o.type, o.m, o.n, o.g, o.e); }
};
struct Member { std::string seq, how, arg; };   // how: "" (plain), "w", "q" or "v"

static spoa::AlignmentType type_of(const std::string& t) {
    if (t == "sw") return spoa::AlignmentType::kSW;
    if (t == "ov") return spoa::AlignmentType::kOV;
    if (t == "nw") return spoa::AlignmentType::kNW;
    throw std::invalid_argument("unknown type " + t);
}

static Kind kind_of(std::string line) {
    Kind k;
    if (line.size() >= 5 && line.compare(line.size() - 5, 5, " +cov") == 0) { k.cov = true; line.resize(line.size() - 5); }
    std::istringstream in(line);
    in >> k.type;
    if (in >> k.m >> k.n >> k.g >> k.e) k.affine = true;
    else { k.m = 5; k.n = -4; k.g = -8; k.e = -8; }
    return k;
}

static std::vector<std::uint32_t> vector_of(const Member& mb) {
    std::vector<std::uint32_t> w;
    if (mb.how == "w") w.assign(mb.seq.size(), (std::uint32_t)atoi(mb.arg.c_str()));
    else if (mb.how == "q") for (char c : mb.arg) w.push_back((std::uint32_t)(c - 33));
    else if (mb.how == "v") { std::istringstream in(mb.arg); std::string tok; while (std::getline(in, tok, ',')) w.push_back((std::uint32_t)atoi(tok.c_str())); }
    else w.assign(mb.seq.size(), 1);
    return w;
}

template <class F> static bool throws_invalid(F f) {
    try { f(); } catch (const std::invalid_argument&) { return true; } catch (...) { return false; }
    return false;
}

static int check_throws() {
    auto engine = spoa::createAlignmentEngine(spoa::AlignmentType::kNW, 5, -4, -8);
    const std::string s = "ACGT";
    int bad = 0;
    auto expect = [&](bool ok, const char* what) { if (!ok) { fprintf(stderr, "no std::invalid_argument: %s\n", what); bad++; } };
    auto fresh = [&](const std::function<void(std::unique_ptr<spoa::Graph>&, const spoa::Alignment&)>& f) {
        return throws_invalid([&] { auto graph = spoa::createGraph(); auto a = engine->align_sequence_with_graph(s, graph); f(graph, a); });
    };
    expect(fresh([&](std::unique_ptr<spoa::Graph>& gr, const spoa::Alignment& a) { gr->add_alignment(a, s, 0u); }), "weight 0");
    expect(fresh([&](std::unique_ptr<spoa::Graph>& gr, const spoa::Alignment& a) { gr->add_alignment(a, s, 256u); }), "weight 256");
    expect(fresh([&](std::unique_ptr<spoa::Graph>& gr, const spoa::Alignment& a) { gr->add_alignment(a, s, std::string("III")); }), "quality length");
    expect(fresh([&](std::unique_ptr<spoa::Graph>& gr, const spoa::Alignment& a) { gr->add_alignment(a, s, std::string("II!I")); }), "quality that gives 0");
    expect(fresh([&](std::unique_ptr<spoa::Graph>& gr, const spoa::Alignment& a) { gr->add_alignment(a, s, std::string("II I")); }), "quality below '!'");
    expect(fresh([&](std::unique_ptr<spoa::Graph>& gr, const spoa::Alignment& a) { gr->add_alignment(a, s, std::vector<std::uint32_t>{1, 2, 3}); }), "vector length");
    expect(fresh([&](std::unique_ptr<spoa::Graph>& gr, const spoa::Alignment& a) { gr->add_alignment(a, s, std::vector<std::uint32_t>{1, 0, 3, 4}); }), "vector with 0");
    expect(fresh([&](std::unique_ptr<spoa::Graph>& gr, const spoa::Alignment& a) { gr->add_alignment(a, s, std::vector<std::uint32_t>{1, 2, 300, 4}); }), "vector with 300");
    // what is accepted: the ends of the ranges (no device is needed to record them)
    expect(!fresh([&](std::unique_ptr<spoa::Graph>& gr, const spoa::Alignment& a) { gr->add_alignment(a, s, 255u); }), "weight 255 refused");
    expect(!fresh([&](std::unique_ptr<spoa::Graph>& gr, const spoa::Alignment& a) { gr->add_alignment(a, s, std::string("\"~II")); }), "qualities \" and ~ refused");
    expect(!fresh([&](std::unique_ptr<spoa::Graph>& gr, const spoa::Alignment& a) { gr->add_alignment(a, s, std::vector<std::uint32_t>{1, 255, 3, 4}); }), "vector 1..255 refused");
    if (bad) return 1;
    printf("throws ok\n");
    return 0;
}

int main(int argc, char** argv) {
    int nthreads = 1;
    bool batch = false;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "--threads") && i + 1 < argc) nthreads = std::max(1, atoi(argv[++i]));
        else if (!strcmp(argv[i], "--batch")) batch = true;
        else if (!strcmp(argv[i], "--throws")) return check_throws();
    }
    try {
        std::vector<Kind> kinds;
        std::vector<std::vector<Member>> edges;
        std::string line;
        bool fresh = true;
        while (std::getline(std::cin, line)) {
            if (line.empty()) { fresh = true; continue; }
            if (fresh) { kinds.push_back(kind_of(line)); edges.emplace_back(); fresh = false; continue; }
            Member mb;
            std::istringstream in(line);
            in >> mb.seq >> mb.how;
            if (!mb.how.empty()) { in >> std::ws; std::getline(in, mb.arg); }
            if (mb.seq == "-") mb.seq.clear();
            edges.back().push_back(mb);
        }
        std::vector<std::string> cns(edges.size());
        std::vector<std::vector<std::uint32_t>> cov(edges.size());
        std::vector<char> has_cov(edges.size(), 0);
        std::vector<std::string> errs((size_t)nthreads);
        if (batch) {
            std::map<Kind, std::vector<size_t>> groups;
            for (size_t e = 0; e < edges.size(); e++) groups[kinds[e]].push_back(e);
            for (const auto& gr : groups) {
                const Kind& k = gr.first;
                std::vector<std::vector<std::string>> seqs;
                std::vector<std::vector<std::vector<std::uint8_t>>> wts;
                for (size_t e : gr.second) {
                    seqs.emplace_back(); wts.emplace_back();
                    for (const Member& mb : edges[e]) {
                        if (mb.seq.empty()) continue;
                        const std::vector<std::uint32_t> w = vector_of(mb);
                        seqs.back().push_back(mb.seq);
                        wts.back().emplace_back(w.begin(), w.end());
                    }
                }
                const spoa::hx::Weighted r = spoa::hx::weighted_batch(seqs, wts, type_of(k.type), (std::int8_t)k.m, (std::int8_t)k.n, (std::int8_t)k.g, (std::int8_t)k.e, true, false);
                for (size_t q = 0; q < gr.second.size(); q++) { cns[gr.second[q]] = r.consensus[q]; cov[gr.second[q]] = r.coverage[q]; has_cov[gr.second[q]] = 1; }
            }
        } else {
            auto work = [&](int t) {
                try {
                    for (size_t e = (size_t)t; e < edges.size(); e += (size_t)nthreads) {
                        const Kind& k = kinds[e];
                        auto engine = k.affine ? spoa::createAlignmentEngine(type_of(k.type), (std::int8_t)k.m, (std::int8_t)k.n, (std::int8_t)k.g, (std::int8_t)k.e)
                                               : spoa::createAlignmentEngine(type_of(k.type), (std::int8_t)k.m, (std::int8_t)k.n, (std::int8_t)k.g);
                        auto graph = spoa::createGraph();
                        for (const Member& mb : edges[e]) {
                            auto alignment = engine->align_sequence_with_graph(mb.seq, graph);
                            if (mb.how.empty()) graph->add_alignment(alignment, mb.seq);
                            else if (mb.how == "w") graph->add_alignment(alignment, mb.seq, (std::uint32_t)atoi(mb.arg.c_str()));
                            else if (mb.how == "q") graph->add_alignment(alignment, mb.seq, mb.arg);
                            else graph->add_alignment(alignment, mb.seq, vector_of(mb));
                        }
                        if (k.cov) { cov[e].assign(3, 77u); cns[e] = graph->generate_consensus(cov[e]); has_cov[e] = 1; }   // dst is replaced, not appended to
                        else cns[e] = graph->generate_consensus();
                    }
                } catch (const std::exception& ex) { errs[(size_t)t] = ex.what(); }
            };
            std::vector<std::thread> th;
            for (int t = 1; t < nthreads; t++) th.emplace_back(work, t);
            work(0);
            for (auto& t : th) t.join();
            for (const std::string& e : errs) if (!e.empty()) throw std::runtime_error(e);
        }
        for (size_t e = 0; e < edges.size(); e++) {
            printf("%s\n", cns[e].c_str());
            if (!has_cov[e]) printf("-");
            for (size_t i = 0; i < cov[e].size(); i++) printf(i ? " %u" : "%u", cov[e][i]);
            printf("\n=\n");
        }
        spoa::hx::shutdown();
    } catch (const std::exception& e) {
        fprintf(stderr, "[ERROR] %s\n", e.what());
        return 1;
    }
    return 0;
}
