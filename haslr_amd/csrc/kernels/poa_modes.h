// poa_modes.h — host side of the general POA path (kernels/poa_modes.hip): spoa's linear-gap, affine-gap and convex-gap engines in their three
// alignment modes (kSW local, kNW global, kOV overlap) for caller-given sequence sets, one workgroup per set. DESIGN.md "General POA path".
#ifndef HX_POA_MODES_H
#define HX_POA_MODES_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

namespace hxk {

struct PoaModesWs {   // the path's workspace: one device allocation, grows to the largest call, lives as long as its owner (the context)
    void* p = nullptr;
    size_t cap = 0;
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    ~PoaModesWs() { release(); }
};

// a base as the POA kernels take it: A 0, C 1, G 2, T 3 in either case, anything else A
inline uint8_t base_code(char c) { return c == 'C' || c == 'c' ? 1 : c == 'G' || c == 'g' ? 2 : c == 'T' || c == 't' ? 3 : 0; }
// what the debug lines call a gap model (PoaModesArgs::gap_model)
inline const char* gap_model_label(int gm) { return gm == 2 ? " (convex)" : gm == 1 ? " (affine)" : ""; }

constexpr uint32_t MAX_BAND = 511;   // the widest half-width of a band (PoaModesArgs::band): 2 x 511 + 1 columns are one wavefront's

struct PoaModesArgs {
    const char* who = "";                // the entry point of the C-ABI that asks: the name every error text begins with
    uint32_t n_sets = 0;
    const uint64_t *set_off = nullptr, *seq_off = nullptr;   // hx_poa_sequences' layout
    const char* bases = nullptr;
    int32_t match = 0, mismatch = 0, gap = 0, type = 0;      // type: 0 kSW, 1 kNW, 2 kOV (spoa::AlignmentType)
    uint32_t slot_kb_cap = 0;            // first round only: workspace slots of at most this many KB (0: no cap); sets that overflow are rerun in larger slots
    double workspace_gb = 0;             // cap of the workspace (0: 40 % of the free device memory)
    int debug = 0;
    int32_t gap_extend = 0;              // affine and convex calls: gap is the gap open score, this the gap extend score (gap <= gap_extend <= 0)
    int32_t gap_open2 = 0, gap_extend2 = 0;   // convex calls: the second piece (gap_open2 <= gap_extend2 <= 0, gap_open2 <= gap)
    int gap_model = 0;                   // 0: the linear instances; 1: the affine ones (a cell is an (H, F) pair, sequences of up to 16383 bases); 2: the
                                         // convex ones (a cell is (H, F, O), 12 bytes, sequences of up to 8191 bases)
    int msa = 0;                         // 1: the MSA instances, and the alignment text in PoaModesOut (hx_poa_msa)
    int include_consensus = 0;           // MSA calls: the consensus is the last row of every set
    int weighted = 0;                    // 1: hx_poa_weighted (the instances that keep the node of every base)
    const uint8_t* weights = nullptr;    // weighted calls: a weight per base of `bases`, 1..255 (the caller has checked), or null: all 1
    int want_coverage = 0;               // weighted calls: the coverage of every consensus base in PoaModesOut
    int want_profile = 0;                // weighted calls: and the four letter counts of its column
    int graph = 0;                       // 1: hx_poa_graph (the graph instances; weights as for a weighted call, or null), and the graph and the alignments in PoaModesOut
    int strand = 0;                      // 1: hx_poa_strand (the strand instances: every sequence is aligned forward and reverse-complemented and the better
                                         // one is added; weights as for a weighted call, or null). msa / include_consensus and want_coverage / want_profile
                                         // say what PoaModesOut holds beside the flags and the scores
    uint32_t band = 0;                   // hx_poa_banded: the half-width w of the adaptive band, 1..511 (0: no band). A set whose alignment misses the band is run
                                         // again with 2 w, at last on the full matrix; not with graph or strand
    const uint8_t* labels = nullptr;     // hx_poa_labelled (the label instances; weights as for a weighted call, or null): a label per sequence of the call,
    uint32_t n_labels = 0;               // 0 .. n_labels - 1 or 255 for none (the caller has checked; n_labels 1..16). PoaModesOut then holds n_labels consensus
                                         // strings per set, label after label (cns_off: n_sets x n_labels + 1), their columns, and with include_consensus one row
                                         // per label behind the sequences' rows; msa / include_consensus and want_coverage / want_profile as for a strand call.
                                         // Not with graph, strand or band
    int phase = 0;                       // 1: hx_poa_phased (the phase instances: the label instances with the phasing of the set's reads in front of the views).
    uint32_t phase_min_count = 0;        // The call derives the label of every sequence itself (0, 1, or 255), on the device, and is in everything else a labelled
    uint32_t phase_min_pct = 0;          // call with n_labels = 2: labels stays null. A site's second allele is seen phase_min_count times (1..255) and in
                                         // phase_min_pct per cent (1..50) of the column's depth (the caller has checked). PoaModesOut holds the labels and the sites
    uint32_t aln_cap = 0;                // graph calls, first round only: a set's share of the alignment pool holds at most this many pairs (0: no cap); sets whose
                                         // alignments outgrow it are rerun once with exactly the room they need
};

struct PoaModesOut {
    std::vector<uint64_t> cns_off;       // n_sets + 1 (labelled calls: n_sets x n_labels + 1)
    std::string cns;
    std::vector<uint32_t> cns_col;       // labelled calls: the MSA column of every consensus base (cns's layout)
    uint64_t cells = 0, seq_bases = 0, n_aligned = 0;
    double kernel_ms = 0;                // hipEvents around the launches
    uint32_t launches = 0, retried = 0;  // kernel launches, sets rerun in a larger slot
    // MSA calls: per set its rows (one per given sequence, + 1 with the consensus row) and columns; set i is the rows x columns
    // characters at msa_off[i], row-major, no terminators
    std::vector<uint32_t> msa_rows, msa_cols;
    std::vector<uint64_t> msa_off;       // n_sets + 1
    std::string msa;
    double msa_rows_ms = 0;              // the row-writing kernel alone (it is part of kernel_ms)
    uint64_t msa_moved_bytes = 0;        // what it has to move: the text + 4 bytes per base read
    // weighted calls: per consensus base (cns's layout) its coverage, and four letter counts (A, C, G, T) when asked for
    std::vector<uint32_t> cov, prof;
    double cov_ms = 0;                   // the coverage kernels alone, with the clearing of their counters (part of kernel_ms)
    uint64_t cov_moved_bytes = 0;        // what they have to move
    // graph calls: hx_graph_out's arrays (include/haslr_types.h)
    std::vector<uint64_t> node_off, edge_off, aln_off;   // n_sets + 1, n_sets + 1, sequences + 1
    std::string node_base;
    std::vector<uint32_t> node_rank, node_col, edge_from, edge_to, base_node, cns_node;
    std::vector<int32_t> edge_w, aln_node, aln_pos, aln_score;
    uint32_t aln_retried = 0;            // sets rerun because their alignments outgrew their share of the pool
    double gather_ms = 0;                // the gather kernel alone (part of kernel_ms)
    uint64_t gather_moved_bytes = 0;     // what it has to move: every dense element read once and written once
    // strand calls: per given sequence whether its reverse complement was added, and the end-cell scores of its two orientations
    std::vector<uint8_t> reversed;
    std::vector<int32_t> score_fwd, score_rev;
    uint64_t third_passes = 0;           // sequences whose reverse complement won: each cost a third DP pass
    // banded calls: per set the half-width of the attempt that gave its result (0: the full matrix), the reruns after a band miss, and the
    // largest workspace a round of the call asked for
    std::vector<uint32_t> band_used;
    uint32_t band_reruns = 0;
    uint64_t workspace_bytes = 0;
    // phased calls: per given sequence its haplotype (0, 1, 255: none); per set its haplotypes (1: unphased, or 2) and the voting rounds run;
    // the sites of set i are entries site_off[i] .. site_off[i + 1]: column, the two alleles (0..3 a letter, 4 a gap) and the phase (-1, 0, +1)
    std::vector<uint8_t> hap;
    std::vector<uint32_t> n_haps, phase_rounds;
    std::vector<uint64_t> site_off;      // n_sets + 1
    std::vector<uint32_t> site_col;
    std::vector<uint8_t> site_a1, site_a2;
    std::vector<int8_t> site_phase;
};

// 0 = ok, else -1 with the reason in err
int poa_modes_run(hipStream_t s, PoaModesWs& ws, const PoaModesArgs& a, PoaModesOut& o, std::string& err);

}  // namespace hxk
#endif
