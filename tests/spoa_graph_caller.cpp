// Test program for the graph side of include/spoa_hx.hpp: a caller in spoa's own call pattern (one engine + one graph per edge, sequences
// aligned and added one after the other) that asks the graph for print_dot, print_gfa and alignment(k).
// Input: edges separated by blank lines; the first line of an edge is "type" (a four-score engine with 5 -4 -8), "type match mismatch
// gap_open gap_extend" (a five-score engine) or "type m n g e q c" (a seven-score engine), type = sw, nw or ov; the other lines are its
// sequences ("-": an empty one). --out DIR: edge k's graph goes to DIR/k.dot and DIR/k.gfa. Output per edge: one line per added sequence
// with its alignment as node:pos pairs ("." for none), then a line "=".
// --threads N deals the edges to N threads (default 1); --batch sends the edges of each kind through spoa::hx::graph_batch instead (empty
// members dropped, so that both ways write what spoa would).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
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
    int scores = 3;
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
    Kind k;
    std::istringstream in(line);
    in >> k.type;
    int v[6], nv = 0;
    while (nv < 6 && in >> v[nv]) nv++;
    if (nv >= 4) { k.m = v[0]; k.n = v[1]; k.g = v[2]; k.e = v[3]; k.q = k.g; k.c = k.e; k.scores = 4; }
    if (nv == 6) { k.q = v[4]; k.c = v[5]; k.scores = 6; }
    return k;
}

static std::string pairs_text(const spoa::Alignment& a) {
    if (a.empty()) return ".";
    std::string s;
    for (std::size_t i = 0; i < a.size(); i++) s += (i ? " " : "") + std::to_string(a[i].first) + ":" + std::to_string(a[i].second);
    return s;
}

static void write_file(const std::string& path, const std::string& text) {
    std::ofstream out(path.c_str(), std::ios::binary);
    out << text;
}

int main(int argc, char** argv) {
    int nthreads = 1;
    bool batch = false;
    std::string dir;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "--threads") && i + 1 < argc) nthreads = std::max(1, atoi(argv[++i]));
        else if (!strcmp(argv[i], "--batch")) batch = true;
        else if (!strcmp(argv[i], "--out") && i + 1 < argc) dir = argv[++i];
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
        std::vector<std::vector<std::string>> alns(edges.size());
        std::vector<std::string> errs((size_t)nthreads);
        auto file = [&](size_t e, const char* ext) { return dir.empty() ? std::string() : dir + "/" + std::to_string(e) + ext; };
        if (batch) {
            std::map<Kind, std::vector<size_t>> groups;
            for (size_t e = 0; e < edges.size(); e++) groups[kinds[e]].push_back(e);
            for (const auto& gr : groups) {
                const Kind& k = gr.first;
                std::vector<std::vector<std::string>> clean;
                for (size_t e : gr.second) { clean.emplace_back(); for (const auto& s : edges[e]) if (!s.empty()) clean.back().push_back(s); }
                const std::vector<spoa::hx::GraphData> r = spoa::hx::graph_batch(clean, std::vector<std::vector<std::vector<std::uint8_t>>>(), type_of(k.type), (std::int8_t)k.m, (std::int8_t)k.n,
                                                                                 (std::int8_t)k.g, (std::int8_t)k.e, (std::int8_t)k.q, (std::int8_t)k.c);
                for (size_t q = 0; q < gr.second.size(); q++) {
                    const size_t e = gr.second[q];
                    for (const auto& a : r[q].alignments) alns[e].push_back(pairs_text(a));
                    if (!dir.empty()) { write_file(file(e, ".dot"), spoa::hx::to_dot(r[q])); write_file(file(e, ".gfa"), spoa::hx::to_gfa(r[q])); }
                }
            }
        } else {
            auto work = [&](int t) {
                try {
                    for (size_t e = (size_t)t; e < edges.size(); e += (size_t)nthreads) {
                        const Kind& k = kinds[e];
                        auto engine = k.scores == 6 ? spoa::createAlignmentEngine(type_of(k.type), (std::int8_t)k.m, (std::int8_t)k.n, (std::int8_t)k.g, (std::int8_t)k.e, (std::int8_t)k.q, (std::int8_t)k.c)
                                      : k.scores == 4 ? spoa::createAlignmentEngine(type_of(k.type), (std::int8_t)k.m, (std::int8_t)k.n, (std::int8_t)k.g, (std::int8_t)k.e)
                                                      : spoa::createAlignmentEngine(type_of(k.type), (std::int8_t)k.m, (std::int8_t)k.n, (std::int8_t)k.g);
                        auto graph = spoa::createGraph();
                        size_t added = 0;
                        for (const std::string& s : edges[e]) {
                            auto alignment = engine->align_sequence_with_graph(s, graph);
                            graph->add_alignment(alignment, s);   // (an empty one is ignored, as in spoa)
                            added += !s.empty();
                        }
                        graph->print_dot(std::string());   // (an empty path: nothing happens, no device call)
                        graph->print_dot(file(e, ".dot"));
                        graph->print_gfa(file(e, ".gfa"));
                        if (dir.empty()) graph->print_dot("/dev/null");   // (without --out: still one call that needs the graph)
                        for (size_t q = 0; q < added; q++) if (q == 0 || q + 1 == added) alns[e].push_back(pairs_text(graph->alignment(q)));
                    }
                } catch (const std::exception& ex) { errs[(size_t)t] = ex.what(); }
            };
            std::vector<std::thread> th;
            for (int t = 1; t < nthreads; t++) th.emplace_back(work, t);
            work(0);
            for (auto& t : th) t.join();
            for (const std::string& e : errs) if (!e.empty()) throw std::runtime_error(e);
        }
        for (const auto& a : alns) {
            for (const std::string& r : a) printf("%s\n", r.c_str());
            printf("=\n");
        }
        spoa::hx::shutdown();
    } catch (const std::exception& e) {
        fprintf(stderr, "[ERROR] %s\n", e.what());
        return 1;
    }
    return 0;
}
