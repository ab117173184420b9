// Test program for spoa::hx::banded_batch of include/spoa_hx.hpp. Input: sets separated by blank lines; the first line of a set is
// "type band match mismatch gap_open gap_extend gap_open2 gap_extend2", type = sw, nw or ov, optionally followed by "+c" (rows with the
// consensus row last); the other lines are its sequences ("-": an empty one). The sets of one first line go through ONE banded_batch call.
// Output per set: the consensus; band_used; its rows, one per line; then a line "=".
#include <cstdio>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "spoa_hx.hpp"

static spoa::AlignmentType type_of(const std::string& t) {
    if (t == "sw") return spoa::AlignmentType::kSW;
    if (t == "ov") return spoa::AlignmentType::kOV;
    if (t == "nw") return spoa::AlignmentType::kNW;
    throw std::invalid_argument("unknown type " + t);
}

int main() {
    try {
        std::vector<std::string> heads;
        std::vector<std::vector<std::string>> sets;
        std::string line;
        bool fresh = true;
        while (std::getline(std::cin, line)) {
            if (line.empty()) { fresh = true; continue; }
            if (fresh) { heads.push_back(line); sets.emplace_back(); fresh = false; }
            else sets.back().push_back(line == "-" ? std::string() : line);
        }
        std::map<std::string, std::vector<size_t>> groups;
        for (size_t i = 0; i < sets.size(); i++) groups[heads[i]].push_back(i);
        std::vector<spoa::hx::Banded> res(sets.size());
        for (const auto& gr : groups) {
            std::string head = gr.first;
            bool cns = false;
            if (head.size() >= 3 && head.compare(head.size() - 3, 3, " +c") == 0) { cns = true; head.resize(head.size() - 3); }
            std::istringstream in(head);
            std::string type;
            unsigned band;
            int m, n, g, e, q, c;
            if (!(in >> type >> band >> m >> n >> g >> e >> q >> c)) throw std::invalid_argument("bad first line: " + gr.first);
            std::vector<std::vector<std::string>> part;
            for (size_t i : gr.second) part.push_back(sets[i]);
            const std::vector<spoa::hx::Banded> r = spoa::hx::banded_batch(part, {}, band, type_of(type), (std::int8_t)m, (std::int8_t)n, (std::int8_t)g, (std::int8_t)e, (std::int8_t)q, (std::int8_t)c, true, cns);
            for (size_t k = 0; k < gr.second.size(); k++) res[gr.second[k]] = r[k];
        }
        for (const spoa::hx::Banded& d : res) {
            printf("%s\n%u\n", d.consensus.c_str(), d.band_used);
            for (const std::string& row : d.rows) printf("%s\n", row.c_str());
            printf("=\n");
        }
        spoa::hx::shutdown();
    } catch (const std::exception& e) {
        fprintf(stderr, "[ERROR] %s\n", e.what());
        return 1;
    }
    return 0;
}
