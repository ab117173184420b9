// Test program for spoa::hx::phased_batch of include/spoa_hx.hpp. Input: sets separated by blank lines; the first line of a set is
// "type min_count min_pct match mismatch gap_open gap_extend gap_open2 gap_extend2", type = sw, nw or ov; the other lines are its
// sequences ("-": an empty sequence). The sets of one first line go through ONE phased_batch call, with the consensus rows.
// Output per set: "n_haps rounds"; the haplotypes of its sequences; its sites, four numbers each (column a1 a2 phase); per haplotype its
// consensus and a line with the columns of its bases; the rows, one per line; then a line "=".
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
            if (fresh) { heads.push_back(line); sets.emplace_back(); fresh = false; continue; }
            sets.back().push_back(line == "-" ? std::string() : line);
        }
        std::map<std::string, std::vector<size_t>> groups;
        for (size_t i = 0; i < sets.size(); i++) groups[heads[i]].push_back(i);
        std::vector<spoa::hx::Phased> res(sets.size());
        for (const auto& gr : groups) {
            std::istringstream in(gr.first);
            std::string type;
            unsigned mc, mp;
            int m, n, g, e, q, c;
            if (!(in >> type >> mc >> mp >> m >> n >> g >> e >> q >> c)) throw std::invalid_argument("bad first line: " + gr.first);
            std::vector<std::vector<std::string>> part;
            for (size_t i : gr.second) part.push_back(sets[i]);
            const std::vector<spoa::hx::Phased> r = spoa::hx::phased_batch(part, {}, type_of(type), (std::int8_t)m, (std::int8_t)n, (std::int8_t)g, (std::int8_t)e, (std::int8_t)q, (std::int8_t)c, mc, mp, true, true);
            for (size_t k = 0; k < gr.second.size(); k++) res[gr.second[k]] = r[k];
        }
        for (const spoa::hx::Phased& d : res) {
            printf("%u %u\n", d.n_haps, d.rounds);
            for (size_t k = 0; k < d.hap.size(); k++) printf(k ? " %u" : "%u", (unsigned)d.hap[k]);
            printf("\n");
            for (size_t j = 0; j < d.sites.size(); j++) printf(j ? " %u %u %u %d" : "%u %u %u %d", d.sites[j].column, (unsigned)d.sites[j].a1, (unsigned)d.sites[j].a2, (int)d.sites[j].phase);
            printf("\n");
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
