// make_spoa_vectors — produces tests/golden/spoa/*.json from the REAL rvaser/spoa 1.1.3 (the version the reference pins,
// /root/reference/src/haslr_assemble/Makefile:1). NOT built in this repository's image (spoa is not available here, there is no
// network): a maintainer builds it on any networked machine against a genuine libspoa.a and commits the JSON it prints.
//
//   g++ -O2 -std=c++11 -I<spoa>/include make_spoa_vectors.cpp <spoa>/build/lib/libspoa.a -o make_spoa_vectors
//   ./make_spoa_vectors [match mismatch gap [type [gap_extend [gap_open2 gap_extend2]]]] < sequences.txt > tests/golden/spoa/<name>.json
//
// type: sw, nw or ov (spoa::AlignmentType kSW / kNW / kOV; default nw, the reference's). Vectors of the other two types pin the
// general POA path (hx_poa_sequences_mode, DESIGN.md "General POA path"): they go to tests/golden/spoa_modes/<type>_<name>.json.
// With a gap_extend the engine is spoa's five-score one (gap = gap open; affine gaps, hx_poa_sequences_affine): those vectors go to
// tests/golden/spoa_affine/<type>_<name>.json and carry "gap_extend".
// With gap_open2 and gap_extend2 as well the engine is the seven-score one (two gap pieces, convex gaps: hx_poa_sequences_convex,
// DESIGN.md "Convex gaps"). spoa 1.1.3 has no such engine, so that call is compiled only with -DSPOA_HAS_CONVEX=\"<version>\" against a
// later spoa that has createAlignmentEngine(type, m, n, g, e, q, c); the version given is what the vectors carry as "spoa_version". Without
// the macro the tool builds against 1.1.3 as before and refuses the two extra scores. Those vectors go to
// tests/golden/spoa_convex/<type>_<name>.json and carry "gap_open2" and "gap_extend2" too; tests/test_spoa_convex_golden.py picks them
// up. Nothing is committed into that directory yet.
// A sequence line may carry weights after a blank: "ACGT q IIII" (a quality string: add_alignment(alignment, sequence, quality)) or
// "ACGT v 3,1,40,2" (a vector of weights: add_alignment(alignment, sequence, weights)). Vectors of a run in which some line does pin base
// weights and coverage (hx_poa_weighted, DESIGN.md "Base weights and coverage"): they go to tests/golden/spoa_weighted/<type>_<name>.json
// and carry per case the "weights" of every sequence (numbers, 1 where the line had none) and the "coverage" of every consensus base
// (generate_consensus(dst)). The directory is the slot for them; nothing is committed into it yet.
//
// Input: one case per paragraph - ">name", then one ACGT sequence per line (alignment order), a blank line between cases.
// The five calls are exactly the reference's (Assemble.cpp:499,500,539,540,554): kNW unless a type is given, linear gap, sequences added
// in order, unit weights unless a line gives others.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "spoa/spoa.hpp"

struct Weights { char how = 0; std::string quality; std::vector<uint32_t> values; };   // how: 0 (none), 'q' or 'v'

static std::string consensus_of(const std::vector<std::string>& seqs, const std::vector<Weights>& wts, int type, int m, int n, int g, bool affine, int e, bool convex, int q, int c, std::vector<uint32_t>* coverage) {
#ifdef SPOA_HAS_CONVEX
    auto engine = convex ? spoa::createAlignmentEngine(static_cast<spoa::AlignmentType>(type), (int8_t)m, (int8_t)n, (int8_t)g, (int8_t)e, (int8_t)q, (int8_t)c)
                  : affine ?
#else
    (void)convex; (void)q; (void)c;   // (main has refused them)
    auto engine = affine ?
#endif
                   spoa::createAlignmentEngine(static_cast<spoa::AlignmentType>(type), (int8_t)m, (int8_t)n, (int8_t)g, (int8_t)e)
                         : spoa::createAlignmentEngine(static_cast<spoa::AlignmentType>(type), (int8_t)m, (int8_t)n, (int8_t)g);
    auto graph = spoa::createGraph();
    size_t used = 0;
    for (const std::string& s : seqs) {
        if (s.empty()) continue;   // Assemble.cpp:537 skips empty sub-sequences
        auto alignment = engine->align_sequence_with_graph(s, graph);
        const Weights& w = wts[(size_t)(&s - &seqs[0])];
        if (w.how == 'q') graph->add_alignment(alignment, s, w.quality);
        else if (w.how == 'v') graph->add_alignment(alignment, s, w.values);
        else graph->add_alignment(alignment, s);
        used++;
    }
    if (!used) return std::string();   // Assemble.cpp:544-551
    return coverage ? graph->generate_consensus(*coverage) : graph->generate_consensus();
}

int main(int argc, char** argv) {
    const int m = argc > 3 ? atoi(argv[1]) : 5, n = argc > 3 ? atoi(argv[2]) : -4, g = argc > 3 ? atoi(argv[3]) : -8;
    const std::string tname = argc > 4 ? argv[4] : "nw";
    const int type = tname == "sw" ? 0 : tname == "nw" ? 1 : tname == "ov" ? 2 : -1;
    if (type < 0) { fprintf(stderr, "unknown alignment type '%s' (sw, nw, ov)\n", tname.c_str()); return 2; }
    const bool affine = argc > 5;
    const int e = affine ? atoi(argv[5]) : g;
    if (argc == 7) { fprintf(stderr, "gap_open2 needs gap_extend2 (the second gap piece is two scores)\n"); return 2; }
    const bool convex = argc > 7;
#ifdef SPOA_HAS_CONVEX
    const char* version = convex ? SPOA_HAS_CONVEX : "1.1.3";
#else
    const char* version = "1.1.3";
    if (convex) { fprintf(stderr, "built without -DSPOA_HAS_CONVEX: spoa 1.1.3 has no seven-score engine\n"); return 2; }
#endif
    const int q = convex ? atoi(argv[6]) : g, c = convex ? atoi(argv[7]) : e;
    const char* algo[3] = {"kSW", "kNW", "kOV"};
    std::vector<std::pair<std::string, std::vector<std::string>>> cases;
    std::vector<std::vector<Weights>> weights;   // parallel to cases
    bool weighted = false;
    std::string line;
    while (std::getline(std::cin, line)) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty()) continue;
        if (line[0] == '>') { cases.push_back({line.substr(1), {}}); weights.emplace_back(); }
        else if (!cases.empty()) {
            std::istringstream in(line);
            std::string seq, how, arg;
            in >> seq >> how >> arg;
            Weights w;
            if (how == "q") { w.how = 'q'; w.quality = arg; weighted = true; }
            else if (how == "v") { w.how = 'v'; std::istringstream v(arg); std::string tok; while (std::getline(v, tok, ',')) w.values.push_back((uint32_t)atoi(tok.c_str())); weighted = true; }
            cases.back().second.push_back(seq == "-" ? std::string() : seq);   // "-" = an empty sequence
            weights.back().push_back(w);
        }
    }
    printf("{\"spoa_version\": \"%s\", \"match\": %d, \"mismatch\": %d, \"gap\": %d, ", version, m, n, g);
    if (affine) printf("\"gap_extend\": %d, ", e);
    if (convex) printf("\"gap_open2\": %d, \"gap_extend2\": %d, ", q, c);
    printf("\"algorithm\": \"%s\",\n \"cases\": [", algo[type]);
    for (size_t i = 0; i < cases.size(); i++) {
        printf("%s\n  {\"name\": \"%s\", \"sequences\": [", i ? "," : "", cases[i].first.c_str());
        for (size_t k = 0; k < cases[i].second.size(); k++) printf("%s\"%s\"", k ? ", " : "", cases[i].second[k].c_str());
        if (weighted) {
            printf("], \"weights\": [");
            for (size_t k = 0; k < cases[i].second.size(); k++) {
                const Weights& w = weights[i][k];
                printf("%s[", k ? ", " : "");
                for (size_t q = 0; q < cases[i].second[k].size(); q++)
                    printf("%s%u", q ? ", " : "", w.how == 'q' ? (unsigned)(w.quality[q] - 33) : w.how == 'v' ? (unsigned)w.values[q] : 1u);
                printf("]");
            }
        }
        std::vector<uint32_t> coverage;
        const std::string cns = consensus_of(cases[i].second, weights[i], type, m, n, g, affine, e, convex, q, c, weighted ? &coverage : nullptr);
        printf("], \"consensus\": \"%s\"", cns.c_str());
        if (weighted) {
            printf(", \"coverage\": [");
            for (size_t q = 0; q < coverage.size(); q++) printf("%s%u", q ? ", " : "", (unsigned)coverage[q]);
            printf("]");
        }
        printf("}");
    }
    printf("\n ]}\n");
    return 0;
}
