/* spoa.hpp - TEST INFRASTRUCTURE. Lets the reference's Assemble.cpp link into oracle/_ref/ref_back.
 *
 * The shim exists only so that Assemble.cpp links. It computes nothing of its own: add_alignment records the sequences in
 * call order and generate_consensus hands them to orc_poa_consensus in liboracle.so, with the scores the engine was created
 * with. Nothing it returns is ever cited as evidence about SPOA: the consensus stage stays unpinned.
 * What ref_back pins is everything in Assemble.cpp AROUND the consensus strings: the edge coordinates, the sub-sequence
 * rule, path extraction and stitching, given those strings.
 *
 * Written from the five symbols Assemble.cpp:499-554 uses. It is not include/spoa_hx.hpp (product code that runs the GPU)
 * and does not include it.
 */
#ifndef HASLR_ORACLE_SPOA_SHIM_HPP
#define HASLR_ORACLE_SPOA_SHIM_HPP
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "oracle.h"

namespace spoa {

enum class AlignmentType { kSW, kNW, kOV };   /* local, global, overlap */

using Alignment = std::vector<std::pair<std::int32_t, std::int32_t>>;

class Graph {
public:
    void add_alignment(const Alignment&, const std::string& sequence) { seqs_.push_back(sequence); }

    std::string generate_consensus() {
        std::vector<const char*> p;
        for (const std::string& s : seqs_) p.push_back(s.c_str());
        char* c = orc_poa_consensus(p.data(), (uint32_t)p.size(), &scores_);
        if (!c) {
            fprintf(stderr, "spoa shim: orc_poa_consensus failed: %s\n", orc_last_error());
            abort();
        }
        std::string out(c);
        orc_free_str(c);
        return out;
    }

    hx_poa_params scores_{5, -4, -8};   /* set by align_sequence_with_graph from the engine that is used with this graph */
private:
    std::vector<std::string> seqs_;
};

class AlignmentEngine {
public:
    AlignmentEngine(std::int8_t m, std::int8_t n, std::int8_t g) : scores_{m, n, g} {}

    /* no alignment is computed here: the oracle aligns when the consensus is asked for */
    Alignment align_sequence_with_graph(const std::string&, const std::unique_ptr<Graph>& graph) {
        graph->scores_ = scores_;
        return Alignment();
    }

private:
    hx_poa_params scores_;
};

inline std::unique_ptr<AlignmentEngine> createAlignmentEngine(AlignmentType type, std::int8_t m, std::int8_t n, std::int8_t g) {
    if (type != AlignmentType::kNW) {
        fprintf(stderr, "spoa shim: only the global alignment type is stood in for (got type %d)\n", (int)type);
        abort();
    }
    return std::unique_ptr<AlignmentEngine>(new AlignmentEngine(m, n, g));
}

inline std::unique_ptr<Graph> createGraph() { return std::unique_ptr<Graph>(new Graph()); }

}  // namespace spoa
#endif
