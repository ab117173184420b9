// poa_phase_report_driver.cpp - feeds haslr_amd/csrc/hx_poa_report.cpp (linked alone: no HIP, no GPU) synthetic phase words and prints what it reports:
// tests/test_poa_phase_report.py holds the text to literal strings. The words are laid out HERE by bare position, on purpose: this file is the second
// statement of the layout that kernels/poa_phase_words.h names, so a renumbered word or a moved bit split there changes the text.
// Usage: poa_phase_report_driver <debug> <prof>   ->   the report on stdout, then one line with the returned figures
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../haslr_amd/csrc/hx_poa_report.h"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    typedef unsigned long long W;
    const int NW = 21, NE = 8;
    std::vector<W> words((size_t)NE * NW);
    for (int e = 0; e < NE; e++) {
        W* w = &words[(size_t)e * NW];
        // every word of every edge another value; the order of the edges by total cycles is neither that of their indices nor its reverse
        for (int k = 0; k < 6; k++) w[k] = 1000ull * ((e * 5 + 3) % NE + 1) * (k + 1) + 13 * e + k;
        // words 6-11: nonzero bits 0-31, 32-39 and 40-63, so both halves of a 40 | 24 and of a 32 | 32 split are nonzero
        for (int k = 6; k < 12; k++) w[k] = (W)(700 + 50 * e + k) | (W)(3 + 6 * e + (k - 6)) << 32 | (W)(100 + 10 * e + k) << 40;
        for (int k = 12; k < 16; k++) w[k] = 90000ull + 400 * e + 7 * k;
        w[16] = (W)(5000000 + 1234 * ((e * 3 + 2) % NE)) | (W)(0x1100 + 37 * e) << 44;   // begin: wall clock | where
        w[17] = (W)(5000000 + 1234 * NE + 999 * e);                                        // end
        w[18] = 4100 + e; w[19] = 60 + e; w[20] = 80000 + 31 * e;
    }
    words[3 * NW + 2] = (W)-12345ll;   // a phase counter that is negative as long long (edge 3, traceback): reported as 0
    words[5 * NW + 16] = 0;            // an edge that never began: no [hx-edge] line
    std::vector<uint32_t> lmax, nseq, shape;
    for (int e = 0; e < NE; e++) { lmax.push_back(300 + 17 * e); nseq.push_back(3 + e); }
    const std::vector<uint8_t> cls = {0, 0, 2, 2, 7, 7, 2};   // three launch classes; the last edge is beyond the vector: class 11
    for (size_t e = 0; e < cls.size(); e++) shape.push_back((64u << (e % 4)) | (uint32_t)(1 + e % 3) << 16 | (uint32_t)(1 + e % 2) << 24);
    const uint32_t ring[11] = {8, 0, 4, 0, 0, 0, 0, 2, 0, 0, 0};
    const hxi::PoaReportView v{words.data(), (size_t)NE, lmax.data(), nseq.data(), cls.data(), shape.data(), cls.size(), ring, atoi(argv[1]), atoi(argv[2]), stdout};
    uint64_t sum6[6], max6[6];
    const hxi::PoaReport r = hxi::poa_phase_report(v, sum6, max6);
    uint64_t pr[4];
    hxi::poa_prune_sums(words.data(), NE, pr);
    printf("edges %u sum6", r.edges);
    for (int k = 0; k < 6; k++) printf(" %llu", (W)sum6[k]);
    printf(" max6");
    for (int k = 0; k < 6; k++) printf(" %llu", (W)max6[k]);
    printf(" prune");
    for (int k = 0; k < 4; k++) printf(" %llu", (W)pr[k]);
    printf("\n");
    return 0;
}
