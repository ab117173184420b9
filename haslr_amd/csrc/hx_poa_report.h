// hx_poa_report.h - the report over the diagnostic words of a consensus call (kernels/poa_phase_words.h): what hx_poa_phase_cycles and
// hx_poa_prune_stats return and what options `debug` / `prof` print. Host-only C++ without the HIP headers and without the context: its input is a view.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "kernels/poa_phase_words.h"

namespace hxi {

constexpr int POA_NO_CLASS = 11;   // launch classes are 0-10; an edge without a launch counts here
struct PoaReportView {
    unsigned long long* words;    // POA_PHASE_WORDS per edge (a negative phase counter is set to 0 in place)
    size_t n_edges;
    const uint32_t *lmax, *nseq;  // per edge: longest sequence, sequences
    const uint8_t* cls;           // per edge with a launch (the first n_launched): its launch class; the others count as class 11
    const uint32_t* shape;        // ... lanes of its workgroup | column passes << 16 | members << 24
    size_t n_launched;
    const uint32_t* ring;         // per launch class (11): kept rows of its LDS ring
    int debug, prof;              // options: 0 silent, 1 the summary, 2 also a line per edge; which development build wrote words 6-11 (0: the default build)
    FILE* out;
    const unsigned long long* edge(size_t e) const { return words + e * hxk::POA_PHASE_WORDS; }
    int cls_of(size_t e) const { return e < n_launched ? cls[e] : POA_NO_CLASS; }
    uint32_t shape_of(size_t e) const { return e < n_launched ? shape[e] : 0; }
};
struct PoaReport { uint32_t edges, slowest; };   // slowest: the edge with the most phase cycles (max6 is its breakdown)

PoaReport poa_phase_report(const PoaReportView& v, uint64_t* sum6, uint64_t* max6);
void poa_prune_sums(const unsigned long long* words, size_t n_edges, uint64_t* out4);

}  // namespace hxi
