// Test program for the alignment types of include/spoa_hx.hpp: a caller in spoa's own call pattern (one engine + one graph per edge,
// sequences aligned and added one after the other, consensus at the end) whose edges use engines of different types.
// Input: edges separated by blank lines; the first line of an edge is its type (sw, nw or ov), the others its sequences. Output: one
// consensus per line. --threads N deals the edges to N threads (default 1); --batch sends each type's edges through
// spoa::hx::consensus_batch(sets, type) instead; --construct only creates an engine of every type and a graph, and prints "ok".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <thread>
#include <vector>

#include "spoa_hx.hpp"

static spoa::AlignmentType type_of(const std::string& t) {
    if (t == "sw") return spoa::AlignmentType::kSW;
    if (t == "ov") return spoa::AlignmentType::kOV;
    if (t == "nw") return spoa::AlignmentType::kNW;
    throw std::invalid_argument("unknown type " + t);
}

int main(int argc, char** argv) {
    int nthreads = 1;
    bool batch = false, construct = false;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "--threads") && i + 1 < argc) nthreads = std::max(1, atoi(argv[++i]));
        else if (!strcmp(argv[i], "--batch")) batch = true;
        else if (!strcmp(argv[i], "--construct")) construct = true;
    }
    try {
        if (construct) {
            for (const char* t : {"sw", "nw", "ov"}) {
                auto engine = spoa::createAlignmentEngine(type_of(t), 5, -4, -8);
                auto graph = spoa::createGraph();
                auto alignment = engine->align_sequence_with_graph("ACGT", graph);
                graph->add_alignment(alignment, "ACGT");
            }
            printf("ok\n");
            return 0;
        }
        std::vector<std::string> types;
        std::vector<std::vector<std::string>> edges;
        std::string line;
        bool fresh = true;
        while (std::getline(std::cin, line)) {
            if (line.empty()) { fresh = true; continue; }
            if (fresh) { types.push_back(line); edges.emplace_back(); fresh = false; }
            else edges.back().push_back(line == "-" ? std::string() : line);
        }
        std::vector<std::string> cns(edges.size()), errs((size_t)nthreads);
        if (batch) {
            for (const char* t : {"sw", "nw", "ov"}) {
                std::vector<const std::vector<std::string>*> sets;
                std::vector<size_t> idx;
                for (size_t e = 0; e < edges.size(); e++) if (types[e] == t) { sets.push_back(&edges[e]); idx.push_back(e); }
                std::vector<std::vector<std::string>> clean;   // (empty members are skipped, as add_alignment does)
                for (const auto* st : sets) { clean.emplace_back(); for (const auto& s : *st) if (!s.empty()) clean.back().push_back(s); }
                const std::vector<std::string> r = spoa::hx::consensus_batch(clean, type_of(t));
                for (size_t q = 0; q < idx.size(); q++) cns[idx[q]] = r[q];
            }
        } else {
            auto work = [&](int t) {
                try {
                    for (size_t e = (size_t)t; e < edges.size(); e += (size_t)nthreads) {
                        auto engine = spoa::createAlignmentEngine(type_of(types[e]), 5, -4, -8);
                        auto graph = spoa::createGraph();
                        for (const std::string& s : edges[e]) {
                            if (s.empty()) continue;
                            auto alignment = engine->align_sequence_with_graph(s, graph);
                            graph->add_alignment(alignment, s);
                        }
                        cns[e] = graph->generate_consensus();
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
