// Test program for spoa::hx::labelled_batch of include/spoa_hx.hpp. Input: sets separated by blank lines; the first line of a set is
// "type n_labels match mismatch gap_open gap_extend gap_open2 gap_extend2", type = sw, nw or ov; the other lines are its sequences, each
// as "label sequence" ("-": an empty sequence). The sets of one first line go through ONE labelled_batch call, with the consensus rows.
// Output per set: per label its consensus and a line with the columns of its bases; the rows, one per line; then a line "=".
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
        std::vector<std::vector<std::uint8_t>> labels;
        std::string line;
        bool fresh = true;
        while (std::getline(std::cin, line)) {
            if (line.empty()) { fresh = true; continue; }
            if (fresh) { heads.push_back(line); sets.emplace_back(); labels.emplace_back(); fresh = false; continue; }
            std::istringstream in(line);
            unsigned lb;
            std::string q;
            if (!(in >> lb >> q)) throw std::invalid_argument("bad sequence line: " + line);
            labels.back().push_back((std::uint8_t)lb);
            sets.back().push_back(q == "-" ? std::string() : q);
        }
        std::map<std::string, std::vector<size_t>> groups;
        for (size_t i = 0; i < sets.size(); i++) groups[heads[i]].push_back(i);
        std::vector<spoa::hx::Labelled> res(sets.size());
        for (const auto& gr : groups) {
            std::istringstream in(gr.first);
            std::string type;
            unsigned nl;
            int m, n, g, e, q, c;
            if (!(in >> type >> nl >> m >> n >> g >> e >> q >> c)) throw std::invalid_argument("bad first line: " + gr.first);
            std::vector<std::vector<std::string>> part;
            std::vector<std::vector<std::uint8_t>> lpart;
            for (size_t i : gr.second) { part.push_back(sets[i]); lpart.push_back(labels[i]); }
            const std::vector<spoa::hx::Labelled> r = spoa::hx::labelled_batch(part, {}, lpart, nl, type_of(type), (std::int8_t)m, (std::int8_t)n, (std::int8_t)g, (std::int8_t)e, (std::int8_t)q, (std::int8_t)c, true, true);
            for (size_t k = 0; k < gr.second.size(); k++) res[gr.second[k]] = r[k];
        }
        for (const spoa::hx::Labelled& d : res) {
            for (size_t l = 0; l < d.consensus.size(); l++) {
                printf("%s\n", d.consensus[l].c_str());
                for (size_t i = 0; i < d.columns[l].size(); i++) printf(i ? " %u" : "%u", d.columns[l][i]);
                printf("\n");
            }
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
