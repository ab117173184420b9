// poa_phase_words.h - the diagnostic words k_poa leaves per edge (PoaLaunch::phase): the one description of their layout, for the kernel that writes
// them (kernels/poa.hip, poa_dp.inl, poa_update.inl) and the report that reads them (hx_poa_report.cpp). Plain C++: part of kernels.h, and the only
// part of it that host code without the HIP headers can include.
#ifndef HX_POA_PHASE_WORDS_H
#define HX_POA_PHASE_WORDS_H

namespace hxk {

// Per edge POA_PHASE_WORDS words of 64 bits, written by lane 0 of the edge's workgroup (member 0 of a shared edge) when the edge ends:
//
//   word   name               what
//   0-5    PW_DECODE..PW_CSR  cycles of lane 0 per phase: decode, DP, traceback, graph update + final consensus, order update, CSR rebuild
//   6-11   (by build)         the default build: row statistics of the DP, summed over the edge's sequences
//     6    PW_ROWS              DP rows
//     7    PW_MULTI             rows with more than one predecessor
//     8    PW_RING_FIFTH        low 40: predecessor rows read from the LDS ring | high 24: fifth-and-later predecessor entries
//     9    PW_FAR_WIDE          low 40: predecessor rows read back from HBM     | high 24: rows with more than 4 predecessors
//     10   PW_KEPT              rows kept for a non-adjacent reader (+ 1 per alignment whose end-node tie took the reference's order: PW_P2_TIES)
//     11   PW_SEQS_NODES        low 32: sequences                               | high 32: nodes of the finished graph
//          a development build gives the six words another meaning (POA_PHASE_FLAVOUR below): the row segments of wave 0 (PW_SEG0 + j),
//          the DP's sub-phases (PW_P2_*), per member DP and wait kilocycles (PW_P3_MEMBER0 + member, 32 | 32), the graph update's stages (PW_GU_*),
//          the head of a carry batch (PW_BH_*)
//   12-15  PW_PRUNE_*         the pruning: wave-rows, wave-rows skipped, attempts repeated, alignments with a threshold
//   16     PW_BEGIN           low 44: the edge's begin on the 100 MHz wall clock | high 20: where (HW_ID bits 0-14 and the XCC)
//   17     PW_END             the edge's end on the wall clock (44 bits)
//   18     PW_CNS             cycles of the final consensus
//   19     PW_REFCNS          1: the consensus took the reference's topological order
//   20     PW_PRUNE_BULK      wave-rows skipped a batch at a time
enum PoaPhaseWord : int {
    PW_DECODE = 0, PW_DP = 1, PW_TRACEBACK = 2, PW_GRAPH = 3, PW_ORDER = 4, PW_CSR = 5,
    PW_N_PHASES = 6,      // the phase counters are the first words: hx_poa_phase_cycles' sum6 / max6
    PW_BUILD0 = 6,        // the six words whose meaning the build chooses (dp_rows' `prof` points here)
    PW_N_BUILD = 6,
    // POA_PHASE_ROWSTATS (the default build)
    PW_ROWS = 6, PW_MULTI = 7, PW_RING_FIFTH = 8, PW_FAR_WIDE = 9, PW_KEPT = 10, PW_SEQS_NODES = 11,
    // POA_PHASE_ROWSEG (-DHX_DP_PROF): cycles of wave 0's rows by segment - decode, predecessors + cells + chain, wave scan, carry, carry applied + ring, stores
    PW_SEG0 = 6,
    // POA_PHASE_DPSUB (-DHX_DP_PROF -DHX_DP_PROF2): member 0's DP phase - publish, own columns, wait for the members, end node; alignments with a tie, cycles of the toposort
    PW_P2_PUBLISH = 6, PW_P2_OWN = 7, PW_P2_WAIT = 8, PW_P2_END = 9, PW_P2_TIES = 10, PW_P2_TOPO = 11,
    // POA_PHASE_MEMBERS (-DHX_DP_PROF3): word PW_P3_MEMBER0 + min(member, 5) of the GLOBAL array = wait kilocycles << 32 | DP kilocycles, added by every member;
    // in LDS word PW_P3_WAIT collects the member's wait cycles of one DP
    PW_P3_MEMBER0 = 6, PW_P3_WAIT = 6,
    // POA_PHASE_GUSTAGES (-DHX_GU_PROF): stages of the graph update, the first half of the CSR rebuild
    PW_GU_STAGE0 = 6, PW_GU_CSR = 11,
    // POA_PHASE_BATCHHEAD (-DHX_DP_PROF4): the carry hand-over of the waves that have a left neighbour in their workgroup, added by every such wave of every member - lane 0's
    // cycles in the head of a carry batch and batches, apart for the batches whose carries were there at the first look and for those that polled; the rows of those batches;
    // low 32: cycles of two clock reads back to back, one sample per wave and DP (what a timed interval holds besides its code) | high 32: those samples
    PW_BH_READY_CYCLES = 6, PW_BH_READY = 7, PW_BH_POLLED_CYCLES = 8, PW_BH_POLLED = 9, PW_BH_ROWS = 10, PW_BH_CLOCK = 11,
    PW_PRUNE0 = 12,       // (dp_rows' `pstat` points here)
    PW_PRUNE_ROWS = 12, PW_PRUNE_SKIPPED = 13, PW_PRUNE_REPEATED = 14, PW_PRUNE_THRESHOLDS = 15,
    PW_N_PRUNE = 4,       // ... the four that hx_poa_prune_stats returns
    PW_BEGIN = 16, PW_END = 17, PW_CNS = 18, PW_REFCNS = 19, PW_PRUNE_BULK = 20
};
constexpr int POA_PHASE_WORDS = 21;
static_assert(PW_PRUNE_BULK + 1 == POA_PHASE_WORDS && PW_BUILD0 + PW_N_BUILD == PW_PRUNE0 && PW_PRUNE0 + PW_N_PRUNE == PW_BEGIN, "the phase words are dense");

// Which meaning of words 6-11 is compiled in (one at a time; of several flags the first of PROF4, PROF3, PROF2, PROF, GU_PROF holds). The kernel files test
// POA_PHASE_FLAVOUR, nothing else: the row statistics are written only by POA_PHASE_ROWSTATS, each set of timers only by its own flavour.
#define POA_PHASE_ROWSTATS 0
#define POA_PHASE_ROWSEG 1
#define POA_PHASE_DPSUB 2
#define POA_PHASE_MEMBERS 3
#define POA_PHASE_GUSTAGES 4
#define POA_PHASE_BATCHHEAD 5
#if defined(HX_DP_PROF2) && !defined(HX_DP_PROF) && !defined(HX_DP_PROF3)
#error "HX_DP_PROF2 refines HX_DP_PROF: define both"
#endif
#if defined(HX_DP_PROF4)
#define POA_PHASE_FLAVOUR POA_PHASE_BATCHHEAD
#elif defined(HX_DP_PROF3)
#define POA_PHASE_FLAVOUR POA_PHASE_MEMBERS
#elif defined(HX_DP_PROF2)
#define POA_PHASE_FLAVOUR POA_PHASE_DPSUB
#elif defined(HX_DP_PROF)
#define POA_PHASE_FLAVOUR POA_PHASE_ROWSEG
#elif defined(HX_GU_PROF)
#define POA_PHASE_FLAVOUR POA_PHASE_GUSTAGES
#else
#define POA_PHASE_FLAVOUR POA_PHASE_ROWSTATS
#endif

// The packed words. pw_lo / pw_hi split a word at bit `lo_bits`; pw_pack puts the two halves together (it does not mask the low half: the counts
// fit, and the wall clock goes through pw_lo first).
constexpr int PW_SPLIT_CLOCK = 44;   // PW_BEGIN: wall clock | HW_ID
constexpr int PW_SPLIT_REFS = 40;    // PW_RING_FIFTH, PW_FAR_WIDE
constexpr int PW_SPLIT_HALF = 32;    // PW_SEQS_NODES, PW_P3_MEMBER0 + m, PW_BH_CLOCK
constexpr unsigned long long pw_lo(unsigned long long w, int lo_bits) { return w & ((1ull << lo_bits) - 1); }
constexpr unsigned long long pw_hi(unsigned long long w, int lo_bits) { return w >> lo_bits; }
constexpr unsigned long long pw_pack(unsigned long long lo, unsigned long long hi, int lo_bits) { return lo | (hi << lo_bits); }

}  // namespace hxk
#endif
