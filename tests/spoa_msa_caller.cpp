// Test program for the MSA side of include/spoa_hx.hpp: a caller in spoa's own call pattern (one engine + one graph per edge, sequences
// aligned and added one after the other) that asks the graph for generate_multiple_sequence_alignment instead of the consensus.
// Input: edges separated by blank lines; the first line of an edge is "type" (a four-score engine with 5 -4 -8) or
// "type match mismatch gap_open gap_extend" (a five-score engine), type = sw, nw or ov, optionally followed by "+c" (include the
// consensus row); the other lines are its sequences ("-": an empty one). Output per edge: its rows, one per line, then a line "=".
// --threads N deals the edges to N threads (default 1); --batch sends the edges of each kind through spoa::hx::msa_batch instead (empty
// members dropped, so that both ways print what spoa prints).
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
    bool affine = false, cns = false;
    int m = 5, n = -4, g = -8, e = -8;
    bool operator<(const Kind& o) const { return std::tie(type, affine, cns, m, n, g, e) < std::tie(o.type, o.affine, o.cns, o.m, o.n, o.g, o.e); }
};

static spoa::AlignmentType type_of(const std::string& t) {
    if (t == "sw") return spoa::AlignmentType::kSW;
    if (t == "ov") return spoa::AlignmentType::kOV;
    if (t == "nw") return spoa::AlignmentType::kNW;
    throw std::invalid_argument("unknown type " + t);
}

static Kind kind_of(std::string line) {
    Kind k;
    if (line.size() >= 3 && line.compare(line.size() - 3, 3, " +c") == 0) { k.cns = true; line.resize(line.size() - 3); }
    std::istringstream in(line);
    in >> k.type;
    if (in >> k.m >> k.n >> k.g >> k.e) k.affine = true;
    else { k.m = 5; k.n = -4; k.g = -8; k.e = -8; }
    return k;
}

int main(int argc, char** argv) {
    int nthreads = 1;
    bool batch = false;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "--threads") && i + 1 < argc) nthreads = std::max(1, atoi(argv[++i]));
        else if (!strcmp(argv[i], "--batch")) batch = true;
    }
    try {
        std::vector<Kind> kinds;
        std::vector<std::vector<std::string>> edges;
        std::string line;
        bool fresh = true;
        while (std::getline(std::cin, line)) {
            if (line.empty()) { fresh = true; continue; }
            if (fresh) { kinds.push_back(kind_of(line)); edges.emplace_back(); fresh = false; }
            else edges.back().push_back(line == "-" ? std::string() : line);
        }
        std::vector<std::vector<std::string>> msa(edges.size());
        std::vector<std::string> errs((size_t)nthreads);
        if (batch) {
            std::map<Kind, std::vector<size_t>> groups;
            for (size_t e = 0; e < edges.size(); e++) groups[kinds[e]].push_back(e);
            for (const auto& gr : groups) {
                const Kind& k = gr.first;
                std::vector<std::vector<std::string>> clean;
                for (size_t e : gr.second) { clean.emplace_back(); for (const auto& s : edges[e]) if (!s.empty()) clean.back().push_back(s); }
                const std::vector<std::vector<std::string>> r = spoa::hx::msa_batch(clean, type_of(k.type), (std::int8_t)k.m, (std::int8_t)k.n, (std::int8_t)k.g, (std::int8_t)k.e, k.cns);
                for (size_t q = 0; q < gr.second.size(); q++) msa[gr.second[q]] = r[q];
            }
        } else {
            auto work = [&](int t) {
                try {
                    for (size_t e = (size_t)t; e < edges.size(); e += (size_t)nthreads) {
                        const Kind& k = kinds[e];
                        auto engine = k.affine ? spoa::createAlignmentEngine(type_of(k.type), (std::int8_t)k.m, (std::int8_t)k.n, (std::int8_t)k.g, (std::int8_t)k.e)
                                               : spoa::createAlignmentEngine(type_of(k.type), (std::int8_t)k.m, (std::int8_t)k.n, (std::int8_t)k.g);
                        auto graph = spoa::createGraph();
                        for (const std::string& s : edges[e]) {
                            auto alignment = engine->align_sequence_with_graph(s, graph);
                            graph->add_alignment(alignment, s);   // (an empty one is ignored, as in spoa)
                        }
                        msa[e].assign(1, "stale");   // dst is replaced, not appended to
                        if (k.cns) graph->generate_multiple_sequence_alignment(msa[e], true);
                        else graph->generate_multiple_sequence_alignment(msa[e]);
                    }
                } catch (const std::exception& ex) { errs[(size_t)t] = ex.what(); }
            };
            std::vector<std::thread> th;
            for (int t = 1; t < nthreads; t++) th.emplace_back(work, t);
            work(0);
            for (auto& t : th) t.join();
            for (const std::string& e : errs) if (!e.empty()) throw std::runtime_error(e);
        }
        for (const auto& rows : msa) {
            for (const std::string& r : rows) printf("%s\n", r.c_str());
            printf("=\n");
        }
        spoa::hx::shutdown();
    } catch (const std::exception& e) {
        fprintf(stderr, "[ERROR] %s\n", e.what());
        return 1;
    }
    return 0;
}
