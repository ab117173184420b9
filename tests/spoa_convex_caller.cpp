// Test program for the seven-score (convex gap) engines of include/spoa_hx.hpp: a caller in spoa's own call pattern (one engine + one graph
// per edge, sequences aligned and added one after the other, consensus at the end) whose edges use linear, affine and convex engines of
// different types. Input: edges separated by blank lines; the first line of an edge is "type" (a four-score engine with 5 -4 -8),
// "type match mismatch gap_open gap_extend" (a five-score engine) or "type match mismatch gap_open gap_extend gap_open2 gap_extend2" (a
// seven-score engine), type = sw, nw or ov; the other lines are its sequences. Output: one consensus per line. --threads N deals the edges
// to N threads (default 1); --batch sends the edges of each engine kind through spoa::hx::consensus_batch instead; --outputs prints per
// edge, instead of the consensus alone, "consensus|coverage,...|row|row|..." from generate_consensus(dst) and
// generate_multiple_sequence_alignment(dst, true); --construct creates a seven-score engine of every type, checks that bad scores throw,
// and prints "ok".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
    int scores = 4;   // of the engine: 4, 5 or 7
    int m = 5, n = -4, g = -8, e = -8, q = -8, c = -8;
    bool operator<(const Kind& o) const { return std::tie(type, scores, m, n, g, e, q, c) < std::tie(o.type, o.scores, o.m, o.n, o.g, o.e, o.q, o.c); }
};

static spoa::AlignmentType type_of(const std::string& t) {
    if (t == "sw") return spoa::AlignmentType::kSW;
    if (t == "ov") return spoa::AlignmentType::kOV;
    if (t == "nw") return spoa::AlignmentType::kNW;
    throw std::invalid_argument("unknown type " + t);
}

static Kind kind_of(const std::string& line) {
    std::istringstream in(line);
    Kind k;
    in >> k.type;
    if (in >> k.m >> k.n >> k.g >> k.e) {
        k.scores = 5;
        if (in >> k.q >> k.c) k.scores = 7;
    } else { k.m = 5; k.n = -4; k.g = -8; k.e = -8; }
    return k;
}

static std::unique_ptr<spoa::AlignmentEngine> engine_of(const Kind& k) {
    if (k.scores == 7) return spoa::createAlignmentEngine(type_of(k.type), (std::int8_t)k.m, (std::int8_t)k.n, (std::int8_t)k.g, (std::int8_t)k.e, (std::int8_t)k.q, (std::int8_t)k.c);
    if (k.scores == 5) return spoa::createAlignmentEngine(type_of(k.type), (std::int8_t)k.m, (std::int8_t)k.n, (std::int8_t)k.g, (std::int8_t)k.e);
    return spoa::createAlignmentEngine(type_of(k.type), (std::int8_t)k.m, (std::int8_t)k.n, (std::int8_t)k.g);
}

static bool throws(spoa::AlignmentType t, int g, int e, int q, int c) {
    try { spoa::createAlignmentEngine(t, 5, -4, (std::int8_t)g, (std::int8_t)e, (std::int8_t)q, (std::int8_t)c); } catch (const std::invalid_argument&) { return true; }
    return false;
}

int main(int argc, char** argv) {
    int nthreads = 1;
    bool batch = false, construct = false, outputs = false;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "--threads") && i + 1 < argc) nthreads = std::max(1, atoi(argv[++i]));
        else if (!strcmp(argv[i], "--batch")) batch = true;
        else if (!strcmp(argv[i], "--construct")) construct = true;
        else if (!strcmp(argv[i], "--outputs")) outputs = true;
    }
    try {
        if (construct) {
            for (const char* t : {"sw", "nw", "ov"}) {
                for (int c : {-8, -6, -4, -1, 0}) {   // (c <= e = -6: the second piece never wins, the engine is the five-score one)
                    auto engine = spoa::createAlignmentEngine(type_of(t), 5, -4, -8, -6, -10, (std::int8_t)c);
                    auto graph = spoa::createGraph();
                    auto alignment = engine->align_sequence_with_graph("ACGT", graph);
                    graph->add_alignment(alignment, "ACGT");
                }
                // first piece: gap open >= 0, gap extend > 0, gap extend below gap open; the same for the second piece; the second piece opens cheaper
                if (!throws(type_of(t), 0, 0, -10, -4) || !throws(type_of(t), -8, 1, -10, -4) || !throws(type_of(t), -2, -8, -10, -4) || !throws(type_of(t), -8, -6, 0, 0) ||
                    !throws(type_of(t), -8, -6, -10, 1) || !throws(type_of(t), -8, -6, -10, -12) || !throws(type_of(t), -8, -6, -7, -4) || throws(type_of(t), -8, -6, -8, -4)) {
                    fprintf(stderr, "bad scores were accepted (%s)\n", t);
                    return 2;
                }
            }
            if (!throws(static_cast<spoa::AlignmentType>(3), -8, -6, -10, -4)) { fprintf(stderr, "an unknown type was accepted\n"); return 2; }
            printf("ok\n");
            return 0;
        }
        std::vector<Kind> kinds;
        std::vector<std::vector<std::string>> edges;
        std::string line;
        bool fresh = true;
        while (std::getline(std::cin, line)) {
            if (line.empty()) { fresh = true; continue; }
            if (fresh) { kinds.push_back(kind_of(line)); edges.emplace_back(); fresh = false; }
            else edges.back().push_back(line == "-" ? std::string() : line);
        }
        std::vector<std::string> cns(edges.size()), errs((size_t)nthreads);
        if (batch) {
            std::map<Kind, std::vector<size_t>> groups;
            for (size_t e = 0; e < edges.size(); e++) groups[kinds[e]].push_back(e);
            for (const auto& gr : groups) {
                const Kind& k = gr.first;
                std::vector<std::vector<std::string>> clean;   // (empty members are skipped, as add_alignment does)
                for (size_t e : gr.second) { clean.emplace_back(); for (const auto& s : edges[e]) if (!s.empty()) clean.back().push_back(s); }
                const std::vector<std::string> r = k.scores == 7
                    ? spoa::hx::consensus_batch(clean, type_of(k.type), (std::int8_t)k.m, (std::int8_t)k.n, (std::int8_t)k.g, (std::int8_t)k.e, (std::int8_t)k.q, (std::int8_t)k.c)
                    : k.scores == 5 ? spoa::hx::consensus_batch(clean, type_of(k.type), (std::int8_t)k.m, (std::int8_t)k.n, (std::int8_t)k.g, (std::int8_t)k.e)
                                    : spoa::hx::consensus_batch(clean, type_of(k.type), (std::int8_t)k.m, (std::int8_t)k.n, (std::int8_t)k.g);
                for (size_t q = 0; q < gr.second.size(); q++) cns[gr.second[q]] = r[q];
            }
        } else {
            auto work = [&](int t) {
                try {
                    for (size_t e = (size_t)t; e < edges.size(); e += (size_t)nthreads) {
                        auto engine = engine_of(kinds[e]);
                        auto graph = spoa::createGraph();
                        for (const std::string& s : edges[e]) {
                            if (s.empty()) continue;
                            auto alignment = engine->align_sequence_with_graph(s, graph);
                            graph->add_alignment(alignment, s);
                        }
                        if (!outputs) { cns[e] = graph->generate_consensus(); continue; }
                        std::vector<std::uint32_t> cov;
                        std::vector<std::string> rows;
                        std::string line = graph->generate_consensus(cov) + "|";
                        for (size_t q = 0; q < cov.size(); q++) line += (q ? "," : "") + std::to_string(cov[q]);
                        graph->generate_multiple_sequence_alignment(rows, true);
                        for (const std::string& r : rows) line += "|" + r;
                        cns[e] = line;
                    }
                } catch (const std::exception& ex) { errs[(size_t)t] = ex.what(); }
            };
            std::vector<std::thread> th;
            for (int t = 1; t < nthreads; t++) th.emplace_back(work, t);
            work(0);
            for (auto& t : th) t.join();
            for (const std::string& e : errs) if (!e.empty()) throw std::runtime_error(e);
        }
        for (const std::string& c : cns) printf("%s\n", c.c_str());
        const spoa::hx::Stats st = spoa::hx::stats();
        fprintf(stderr, "device_calls=%llu sets=%llu\n", (unsigned long long)st.device_calls, (unsigned long long)st.sets);
        spoa::hx::shutdown();
    } catch (const std::exception& e) {
        fprintf(stderr, "[ERROR] %s\n", e.what());
        return 1;
    }
    return 0;
}
