// make_spoa_vectors — produces tests/golden/spoa/*.json from the REAL rvaser/spoa 1.1.3 (the version the reference pins,
// /root/reference/src/haslr_assemble/Makefile:1). NOT built in this repository's image (spoa is not available here, there is no
// network): a maintainer builds it on any networked machine against a genuine libspoa.a and commits the JSON it prints.
//
//   g++ -O2 -std=c++11 -I<spoa>/include make_spoa_vectors.cpp <spoa>/build/lib/libspoa.a -o make_spoa_vectors
//   ./make_spoa_vectors [match mismatch gap [type [gap_extend]]] < sequences.txt > tests/golden/spoa/<name>.json
//
// type: sw, nw or ov (spoa::AlignmentType kSW / kNW / kOV; default nw, the reference's). Vectors of the other two types pin the
// general POA path (hx_poa_sequences_mode, DESIGN.md "General POA path"): they go to tests/golden/spoa_modes/<type>_<name>.json.
// With a gap_extend the engine is spoa's five-score one (gap = gap open; affine gaps, hx_poa_sequences_affine): those vectors go to
// tests/golden/spoa_affine/<type>_<name>.json and carry "gap_extend".
//
// Input: one case per paragraph - ">name", then one ACGT sequence per line (alignment order), a blank line between cases.
// The five calls are exactly the reference's (Assemble.cpp:499,500,539,540,554): kNW unless a type is given, linear gap, sequences added
// in order, unit weights.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "spoa/spoa.hpp"

static std::string consensus_of(const std::vector<std::string>& seqs, int type, int m, int n, int g, bool affine, int e) {
    auto engine = affine ? spoa::createAlignmentEngine(static_cast<spoa::AlignmentType>(type), (int8_t)m, (int8_t)n, (int8_t)g, (int8_t)e)
                         : spoa::createAlignmentEngine(static_cast<spoa::AlignmentType>(type), (int8_t)m, (int8_t)n, (int8_t)g);
    auto graph = spoa::createGraph();
    size_t used = 0;
    for (const std::string& s : seqs) {
        if (s.empty()) continue;   // Assemble.cpp:537 skips empty sub-sequences
        auto alignment = engine->align_sequence_with_graph(s, graph);
        graph->add_alignment(alignment, s);
        used++;
    }
    return used ? graph->generate_consensus() : std::string();   // Assemble.cpp:544-551
}

int main(int argc, char** argv) {
    const int m = argc > 3 ? atoi(argv[1]) : 5, n = argc > 3 ? atoi(argv[2]) : -4, g = argc > 3 ? atoi(argv[3]) : -8;
    const std::string tname = argc > 4 ? argv[4] : "nw";
    const int type = tname == "sw" ? 0 : tname == "nw" ? 1 : tname == "ov" ? 2 : -1;
    if (type < 0) { fprintf(stderr, "unknown alignment type '%s' (sw, nw, ov)\n", tname.c_str()); return 2; }
    const bool affine = argc > 5;
    const int e = affine ? atoi(argv[5]) : g;
    const char* algo[3] = {"kSW", "kNW", "kOV"};
    std::vector<std::pair<std::string, std::vector<std::string>>> cases;
    std::string line;
    while (std::getline(std::cin, line)) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty()) continue;
        if (line[0] == '>') cases.push_back({line.substr(1), {}});
        else if (!cases.empty()) cases.back().second.push_back(line == "-" ? std::string() : line);   // "-" = an empty sequence
    }
    printf("{\"spoa_version\": \"1.1.3\", \"match\": %d, \"mismatch\": %d, \"gap\": %d, ", m, n, g);
    if (affine) printf("\"gap_extend\": %d, ", e);
    printf("\"algorithm\": \"%s\",\n \"cases\": [", algo[type]);
    for (size_t i = 0; i < cases.size(); i++) {
        printf("%s\n  {\"name\": \"%s\", \"sequences\": [", i ? "," : "", cases[i].first.c_str());
        for (size_t k = 0; k < cases[i].second.size(); k++) printf("%s\"%s\"", k ? ", " : "", cases[i].second[k].c_str());
        printf("], \"consensus\": \"%s\"}", consensus_of(cases[i].second, type, m, n, g, affine, e).c_str());
    }
    printf("\n ]}\n");
    return 0;
}
