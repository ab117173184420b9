/* haslr_hip.h — C-ABI of the MI355X (gfx950) implementation of haslr_assemble's hot path.
 *
 * Plain C: opaque context, caller-visible PODs from haslr_types.h, `int` results (0 = ok, <0 = error,
 * text via hx_last_error()), no exceptions and no C++/torch types across the boundary. One context per GPU,
 * one host thread per context. The library fails loudly (error return) when no HIP device is usable;
 * there is no CPU fallback behind these symbols.
 *
 * What each entry point replaces in the reference (paths under /root/reference/src/haslr_assemble/src/):
 *
 *   hx_upload          the in-memory products of load_contig_compressed (Contig.cpp:43-117),
 *                      load_longread_compressed (Longread.cpp:109-162) and the record parse of
 *                      load_alignment (Longread.cpp:250-289), copied once to HBM
 *   hx_chain_reads     filters 1-4 of load_alignment (Longread.cpp:262-272) + per-read sort (:256) +
 *                      process_lr_alignment_group (:182-232) + fix_alignments (:626-635, :430-512) +
 *                      build_compact_longreads (:612-624, :524-610); called from main.cpp:98,116,124
 *   hx_edge_support    bbg_build_graph / bbg_add_edge (Backbone_graph.cpp:148-171, :10-25); main.cpp:131.
 *                      (bbg_remove_weak_edges :348-375 is a count test the host applies to the result.)
 *   hx_edge_coords     asm_calc_edge_coordinates_MT (Assemble.cpp:453-477 -> :157-363); main.cpp:203
 *   hx_poa_batch       asm_cal_cns_seq_MT (Assemble.cpp:580-605 -> :479-560), i.e. the five SPOA 1.1.3 calls
 *                      createAlignmentEngine/createGraph/align_sequence_with_graph/add_alignment/
 *                      generate_consensus at Assemble.cpp:499,500,539,540,554; main.cpp:207
 *
 * The four operators have the signature of the host pipeline's `hx_backend` table
 * (haslr_amd/csrc/host/haslr_host.h); hx_backend_fill() wires them.
 */
#ifndef HASLR_HIP_H
#define HASLR_HIP_H
#include "haslr_types.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct hx_ctx hx_ctx;

const char* hx_last_error(void);
int hx_device_count(void); /* number of HIP devices, <0 on error */

/* stream: a hipStream_t to launch on (e.g. torch's current stream), or NULL to create one.
 * Process environment: the library never modifies it. hx_poa_batch launches its lane-count classes on separate streams; they run side
 * by side only if the HIP runtime was initialised with GPU_MAX_HW_QUEUES >= 8 (the runtime's default is 4), so an application that wants
 * the measured POA throughput exports that variable before its first HIP call (haslr_assemble, haslr_amd/hip.py and bench.py do).
 * Results do not depend on it. */
int hx_ctx_create(int device, void* stream, hx_ctx** out);
void hx_ctx_destroy(hx_ctx*);

/* Tuning and test switches of a context: what used to be HX_* environment variables read inside the library (31 of them, on every call) is
 * state of the context. The library reads NO environment variable; applications that want the old behaviour copy the HX_* variables of their
 * environment in when they create a context (haslr_assemble and haslr_amd/hip.py do, bench.py through hip.py). The reference keeps its knobs in
 * one options struct filled by its command line (Common.hpp:44-65, Commandline.cpp:46-66); these are the knobs it does not have.
 *   hx_set_option    name = an entry of hx_option_names() (the old spelling works too: "HX_POA_SLOTS" = "poa_slots"), value = a number as text;
 *                    NULL or "" = back to the default. Unknown name or malformed value: error. Takes effect with the next operator call.
 *   hx_get_option    current value as a double
 *   hx_option_names  comma-separated list: debug, prof, poa_workspace_gb (cap of the consensus workspace, GB; 0 = 90 % of the free memory),
 *                    poa_prune (exact score-bound pruning of the DP: -1 automatic = calls of thousands of edges, 0 never, else the threshold as a
 *                    percentage of the previous alignment's score per base), launch-shape knobs (poa_cols, poa_cols2_top, poa_member_lanes, poa_cluster_min /
 *                    _max / _topk / _cols, poa_wide_members, poa_wave_max, poa_ring_kb, poa_balance, poa_balance_pct, poa_balance_lanes, poa_streams,
 *                    poa_wide_delay_us, poa_prune_lanes, poa_prune_shared, poa_prune_lazy, poa_pass_lanes, poa_chain_ms, poa_chain_pct,
 *                    poa_own_bucket_first, poa_resident_first, poa_far_shift) and test switches that force rare paths (poa_poll_limit, poa_max_indeg, poa_node_est_pct,
 *                    poa_far_rows, poa_ring_zero, poa_slots, poa_slots_pct, poa_batches, poa_force_cm, coords_lds_supp), and two of the
 *                    general POA path (hx_poa_sequences_mode): poa_general (1: HX_POA_NW runs the general path too) and poa_modes_slot_kb (cap of
 *                    its first round of workspace slots, forcing the rerun of sets in larger ones), poa_affine (1: hx_poa_sequences_affine
 *                    with gap_extend == gap_open runs the affine kernel instead of the linear paths), poa_weighted (1: hx_poa_weighted
 *                    without weights runs the weighted kernels on weights of 1 instead of the unit-weight ones), poa_convex (1: the convex
 *                    entries with gap_extend2 <= gap_extend run the convex kernel instead of the affine entries), poa_graph_aln_cap
 *                    (hx_poa_graph: cap, in pairs, of a set's first share of the alignment pool, forcing its rerun with the exact room), and
 *                    poa_strand_one_h (hx_poa_strand: 1, the default, keeps one score matrix per slot; the only route built).
 *                    Results never depend on any of them. */
int hx_set_option(hx_ctx*, const char* name, const char* value);
int hx_get_option(const hx_ctx*, const char* name, double* value);
const char* hx_option_names(void);

/* copy inputs to HBM; they stay resident for the life of the context (replicated on every GPU in a
 * multi-GPU run). Read shard defaults to all reads. */
int hx_upload(hx_ctx*, const hx_contigs*, const hx_reads*, const hx_hits*, const uint64_t* read_hit_off);
int hx_set_read_shard(hx_ctx*, uint32_t lr_begin, uint32_t lr_end);
/* the uploaded records are the reference's FILTERED set, read back from an index.longread (Longread.cpp:341-372): hx_chain_reads then takes
 * them as they are - no filters 1-5, no sort, no group / palindrome rule - and goes straight to trim + chain, like main.cpp:90-116 does
 * after read_longread_index. Reset by hx_upload. */
void hx_set_prefiltered(hx_ctx*, int on);

int hx_chain_reads(hx_ctx*, const hx_params*, hx_chain_out* out);
int hx_edge_support(hx_ctx*, const hx_params*, hx_edges_out* out);
int hx_edge_coords(hx_ctx*, uint32_t n_sel, const uint32_t* sel_edge, hx_coords_out* out);
int hx_poa_batch(hx_ctx*, const hx_poa_params*, hx_cns_out* out);
/* The consensus operator on its own (what stands where the five SPOA calls stand, Assemble.cpp:499-554), for callers that hold the
 * support lists themselves:
 *   hx_poa_supports   consensus of caller-given edges: `sup` has hx_edge_coords' layout (n_edge, supp_off, supp_lr = read id |
 *                     strand << 31, spos, epos; head_end / tail_beg are not read) and points into the resident reads. The sub-sequence
 *                     rule is the reference's: epos - spos + 1 in 32 bits, clamped to the read like std::string::substr
 *                     (Assemble.cpp:530-532), empty ones skipped (:537), no sequence at all -> empty consensus (:544-551).
 *   hx_poa_sequences  consensus of caller-given sequence sets (plain ACGT text, set i = sequences [set_off[i], set_off[i+1]), sequence
 *                     k = bases[seq_off[k] .. seq_off[k+1])), aligned in the given order; nothing has to be resident. This is the
 *                     entry include/spoa_hx.hpp (the spoa.hpp-shaped C++ header over this library) calls. */
int hx_poa_supports(hx_ctx*, const hx_coords_out* sup, const hx_poa_params*, hx_cns_out* out);
int hx_poa_sequences(hx_ctx*, uint32_t n_sets, const uint64_t* set_off, const uint64_t* seq_off, const char* bases, const hx_poa_params*, hx_cns_out* out);
/*   hx_poa_sequences_mode  hx_poa_sequences with spoa's alignment type: HX_POA_NW is hx_poa_sequences itself (the tuned global path; option
 *                     poa_general sends it through the general path instead, same results); HX_POA_SW (local) and HX_POA_OV (overlap) run the
 *                     general path (kernels/poa_modes.hip, DESIGN.md "General POA path"): one workgroup per set, the full int32 score matrix,
 *                     sequences of up to 32767 bases, sets of up to 2^21 - 2 bases in all. gap >= 0 or an unknown type: error. An alignment that
 *                     holds no sequence position counts as empty (spoa leaves that case undefined): the sequence becomes a new chain. */
int hx_poa_sequences_mode(hx_ctx*, uint32_t n_sets, const uint64_t* set_off, const uint64_t* seq_off, const char* bases, const hx_poa_mode_params*, hx_cns_out* out);
/*   hx_poa_sequences_affine  the same with affine gaps (spoa's five-score engine; DESIGN.md "General POA path", "Affine gaps"): a gap of k bases
 *                     costs gap_open + (k - 1) gap_extend. gap_extend == gap_open is the linear model and goes to hx_poa_sequences_mode (option
 *                     poa_affine sends it through the affine kernel instead, same results); gap_open < gap_extend runs the affine instances of
 *                     the general path: a cell holds H and F, sequences of up to 16383 bases. Errors: gap_open >= 0, gap_extend > 0,
 *                     gap_extend < gap_open (refused, not reinterpreted: what spoa does with such scores cannot be checked here), unknown type. */
int hx_poa_sequences_affine(hx_ctx*, uint32_t n_sets, const uint64_t* set_off, const uint64_t* seq_off, const char* bases, const hx_poa_affine_params*, hx_cns_out* out);
/*   hx_poa_msa        the multiple sequence alignment of every set beside its consensus (spoa's generate_multiple_sequence_alignment; DESIGN.md
 *                     "General POA path", "MSA output"): one gapped row per GIVEN sequence, in the given order, all of the set's n_cols columns
 *                     wide, and with include_consensus the consensus as one more, last row. Columns are spoa's: the nodes in rank order, aligned
 *                     nodes sharing one. An empty sequence gives a row of gaps; a set without a non-empty sequence has n_cols = 0. Lower case is read as
 *                     upper case and letters other than ACGT as A, as everywhere, and rows show what was read. Scores, types, errors and limits are
 *                     hx_poa_sequences_affine's (gap_extend == gap_open: the linear instances, sequences of up to 32767 bases); every type,
 *                     HX_POA_NW too, runs the general path (the tuned global path keeps no node per base). Options poa_modes_slot_kb and
 *                     poa_workspace_gb act as on the other entries. Like the rest of the general path it is NOT pinned against spoa itself
 *                     (the library is not available to the tests): the tests hold it to a CPU restatement of spoa's rule. */
int hx_poa_msa(hx_ctx*, uint32_t n_sets, const uint64_t* set_off, const uint64_t* seq_off, const char* bases, const hx_poa_msa_params*, hx_msa_out* out);
/*   hx_poa_weighted   the consensus under per-base weights, and the coverage of every consensus base (spoa's add_alignment with a weight, a
 *                     quality string or a vector of weights, and generate_consensus(dst); DESIGN.md "General POA path", "Base weights and
 *                     coverage"). weights has one byte per base, parallel to bases, or is NULL (every weight 1). A sequence adds
 *                     w[i-1] + w[i] to every graph edge it walks between its bases i-1 and i, so with weights of 1 every edge gains the 2 of
 *                     the other entries. Weights change nothing but the edge weights the heaviest bundle reads: the alignments, the nodes and
 *                     the columns of the set are those of unit weights. A weight is 1..255: (i) the score of a consensus path is at most the
 *                     sum of all edge weights, at most 2 x 255 x (2^21 - 2) = 1 069 546 500, so the int32 scores of the consensus code stay
 *                     exact for every set the path accepts; (ii) a weight of 0 is refused, not reinterpreted: a zero-weight edge out of a
 *                     source node gives a real node the score -1 that marks "not visited", branch completion then takes it for dead, and with
 *                     all weights 0 spoa's own loop does not end. The error names set, sequence and position. Coverage and profile:
 *                     haslr_types.h; a sequence of one base counts nowhere, as in spoa (it has no edge to carry its label). Scores, types,
 *                     errors and length limits are hx_poa_sequences_affine's; every type, HX_POA_NW too, runs the general path. Options
 *                     poa_modes_slot_kb and poa_workspace_gb act as on the other entries; option poa_weighted (1) sends a call without
 *                     weights through the weighted instances on weights of 1 (same results). Not pinned against spoa, like the rest of the
 *                     general path: the tests hold it to a CPU restatement of spoa's rule. */
int hx_poa_weighted(hx_ctx*, uint32_t n_sets, const uint64_t* set_off, const uint64_t* seq_off, const char* bases, const uint8_t* weights, const hx_poa_weighted_params*, hx_wcns_out* out);
/*   hx_poa_sequences_convex, hx_poa_msa_convex, hx_poa_weighted_convex  the three entries above under two-piece affine ("convex") gaps (spoa's
 *                     seven-score engine, minimap2's gap model; DESIGN.md "General POA path", "Convex gaps"): a gap of k bases scores
 *                     max(gap_open + (k - 1) gap_extend, gap_open2 + (k - 1) gap_extend2), so short gaps pay the first piece and long ones the
 *                     second. Outputs, weight rules, include_consensus, want_coverage and want_profile are those of hx_poa_sequences_affine,
 *                     hx_poa_msa and hx_poa_weighted. gap_extend2 <= gap_extend: the second piece never wins, and the call IS the affine-form
 *                     entry with (gap_open, gap_extend), which sends gap_extend == gap_open on to the linear paths (option poa_convex keeps such
 *                     a call on the convex kernel instead, same results). Otherwise the convex instances of the general path run: a cell holds
 *                     H, F and O (12 bytes), sequences of up to 8191 bases; a longer one is an error that names its set. Errors, each naming the
 *                     score and its value: those of hx_poa_sequences_affine for the first piece, the same three for the second piece
 *                     (gap_open2 >= 0, gap_extend2 > 0, gap_extend2 < gap_open2), gap_open2 > gap_open, an unknown type. Refused, not
 *                     reinterpreted. Scores are int32 in this ABI and the matrices are int32 too, with -2^29 as "minus infinity": for every
 *                     set (its bases + the columns of the kernel instance it runs in, the first of 1 024, 4 096, 8 192, 32 768 (linear), 1 024,
 *                     4 096, 8 192, 16 384 (affine), 1 024, 2 048, 4 096, 8 192 (convex) that holds its longest sequence + 1) x the largest
 *                     score magnitude must stay below 2^29, which every int8 score does for every set the path accepts (2^21 nodes, 32 768
 *                     columns). A set that reaches it is refused by every entry of the general path, hx_poa_sequences_mode to
 *                     hx_poa_labelled, with an error that names the set, its bases, the columns, the magnitude and the product (DESIGN.md
 *                     "Score range of the full matrix" has the derivation; hx_poa_banded has a tighter bound of its own beside it). Not pinned against spoa, like the rest of the general path: the tests hold it to a CPU restatement. */
int hx_poa_sequences_convex(hx_ctx*, uint32_t n_sets, const uint64_t* set_off, const uint64_t* seq_off, const char* bases, const hx_poa_convex_params*, hx_cns_out* out);
int hx_poa_msa_convex(hx_ctx*, uint32_t n_sets, const uint64_t* set_off, const uint64_t* seq_off, const char* bases, const hx_poa_convex_params*, int include_consensus, hx_msa_out* out);
int hx_poa_weighted_convex(hx_ctx*, uint32_t n_sets, const uint64_t* set_off, const uint64_t* seq_off, const char* bases, const uint8_t* weights, const hx_poa_convex_params*, int want_coverage, int want_profile, hx_wcns_out* out);
/*   hx_poa_graph      the partial-order graph itself, the path of every sequence through it and the alignment of every sequence (spoa's
 *                     Graph and its Alignment pairs; DESIGN.md "General POA path", "Graph and alignment output"; the arrays: haslr_types.h,
 *                     hx_graph_out). One entry over the convex parameters, by the rules of hx_poa_msa_convex: gap_extend2 <= gap_extend is the
 *                     affine model of the first piece, and then gap_extend == gap_open the linear one (sequences of up to 8191, 16383 and
 *                     32767 bases). weights as for hx_poa_weighted (1..255, 0 refused), or NULL. Every type runs the general path. The consensus
 *                     and the counters are those of the consensus entries on the same sets (with weights: hx_poa_weighted's). Options
 *                     poa_modes_slot_kb and poa_workspace_gb act as on the other entries; poa_graph_aln_cap (test switch) caps a set's first
 *                     share of the alignment pool in pairs, forcing the rerun with the exact room; options poa_affine and poa_convex keep a
 *                     call of a simpler model on the richer kernel, as elsewhere. Not pinned against spoa, like the rest of the general path. */
int hx_poa_graph(hx_ctx*, uint32_t n_sets, const uint64_t* set_off, const uint64_t* seq_off, const char* bases, const uint8_t* weights, const hx_poa_convex_params*, hx_graph_out* out);
void hx_free_graph(hx_ctx*, hx_graph_out*);
/*   hx_poa_strand     the consensus of sets whose sequences may lie on either strand (spoa's command-line switch -s / --strand-ambiguous;
 *                     DESIGN.md "General POA path", "Strand-ambiguous sets"; the arrays: haslr_types.h, hx_strand_out). For every non-empty
 *                     sequence of a set, in the given order: the set's first one goes in forward; every later one is aligned to the graph as it
 *                     stands both as given and reverse-complemented (reversed, every code c replaced by 3 - c: a letter that is not ACGT reads
 *                     as A and its complement is T), under the call's type and gap model, and the orientation with the higher end-cell score
 *                     is added (a tie, and a local alignment without a cell above 0 either way, goes forward). With weights a reversed
 *                     sequence's weights are reversed with it. One entry over the convex parameters, by hx_poa_graph's rules for the gap
 *                     model (sequences of up to 8191, 16383 and 32767 bases); weights as for hx_poa_weighted (1..255, 0 refused), or NULL.
 *                     Every type runs the general path. The errors are hx_poa_graph's with this entry's name in front. Options
 *                     poa_modes_slot_kb and poa_workspace_gb act as on the other entries; poa_strand_one_h (default 1) keeps one score matrix
 *                     per workspace slot, so that a sequence whose reverse complement wins runs that orientation's DP once more before the
 *                     traceback: the only route there is, a value of 0 changes nothing. Not pinned against spoa, like the rest of the general
 *                     path: the rules are written after spoa's main.cpp as published and the tests hold them to a CPU restatement. */
int hx_poa_strand(hx_ctx*, uint32_t n_sets, const uint64_t* set_off, const uint64_t* seq_off, const char* bases, const uint8_t* weights, const hx_poa_convex_params*, const hx_poa_strand_want*, hx_strand_out* out);
void hx_free_strand(hx_ctx*, hx_strand_out*);
/*   hx_poa_banded     the consensus of sets aligned inside an adaptive band (DESIGN.md "General POA path", "Banded alignment"; the arrays:
 *                     haslr_types.h, hx_band_out). Row i of an alignment's score matrix owns the 2 w + 1 columns around a centre one past
 *                     the best cell of its best predecessor's row; every other cell is minus infinity. An alignment without a reachable
 *                     end cell (kNW, kOV) is a band miss: its set is run again from its first sequence with 2 w, and once 2 w + 1 would
 *                     pass 1023 columns on the full matrix; a set whose longest sequence + 1 fits the window runs on the full matrix at
 *                     once. band_used tells per set which it was. H takes (nodes + 1) x (2 w + 1) cells per workspace slot instead of
 *                     (nodes + 1) x (length + 1), and a window is one wavefront's. One entry over the convex parameters, by hx_poa_graph's
 *                     rules for the gap model (sequences of up to 8191, 16383 and 32767 bases: any set may end on the full matrix); weights
 *                     as for hx_poa_weighted (1..255, 0 refused), or NULL; MSA text, coverage and profile as hx_poa_strand hands them
 *                     over. Every type runs the general path. The errors are hx_poa_graph's with this entry's name in front, and: a band
 *                     outside 1..511; a set for which (its bases + its longest sequence) x the largest score magnitude reaches 2^28 (the
 *                     bound that keeps real scores and minus infinity apart). Options poa_modes_slot_kb and poa_workspace_gb act as on
 *                     the other entries. Under kOV and kSW, whose alignments start anywhere for free, the centre can leave the true diagonal in
 *                     a graph's first rows (DESIGN.md has the measurement): check the result against a wider band there. Graph output and
 *                     strand-ambiguous sets have no band. Not pinned against spoa, which has no band:
 *                     the tests hold the rules to a CPU restatement. */
int hx_poa_banded(hx_ctx*, uint32_t n_sets, const uint64_t* set_off, const uint64_t* seq_off, const char* bases, const uint8_t* weights, const hx_poa_convex_params*, const hx_poa_band_params*, hx_band_out* out);
void hx_free_band(hx_ctx*, hx_band_out*);
/*   hx_poa_labelled   one consensus per caller-given label over the one graph of every set (DESIGN.md "General POA path", "Per-label
 *                     consensus"; the arrays: haslr_types.h, hx_label_out). labels holds a byte per sequence of the call: 0 .. n_labels - 1,
 *                     or 255 for a sequence without a label; n_labels is 1..16. Alignment, graph, rank order, columns and weights are
 *                     hx_poa_weighted's for the same sets: labels enter none of them. The consensus of label g is spoa's heaviest bundle with
 *                     branch completion on the view of g: the edges its non-empty sequences walk, each weighing the sum of w[i-1] + w[i]
 *                     over those sequences alone; where spoa falls back to node 0 the view falls back to its own node of smallest id; a
 *                     label without a non-empty sequence in a set has an empty consensus. All labels of a set share its MSA columns;
 *                     coverage and profile count a label's own sequences of two or more bases; with include_consensus the MSA text has
 *                     one consensus row per label, in label order (a row of gaps for an empty consensus). One entry over the convex
 *                     parameters, by hx_poa_graph's rules for the gap model; weights as for hx_poa_weighted (1..255, 0 refused), or NULL.
 *                     The errors are hx_poa_graph's with this entry's name in front, and: n_labels outside 1..16; a label >= n_labels
 *                     other than 255 (names set and sequence). Options poa_modes_slot_kb and poa_workspace_gb act as on the other
 *                     entries. No band, no strands, no graph output. Not pinned against spoa, which has no such entry: the tests hold the
 *                     rules to a CPU restatement. */
int hx_poa_labelled(hx_ctx*, uint32_t n_sets, const uint64_t* set_off, const uint64_t* seq_off, const char* bases, const uint8_t* weights, const uint8_t* labels, const hx_poa_convex_params*, const hx_poa_label_params*, hx_label_out* out);
void hx_free_label(hx_ctx*, hx_label_out*);
/*   hx_poa_phased     two-haplotype consensus with automatic read phasing (DESIGN.md "General POA path", "Two-haplotype consensus"; the
 *                     arrays: haslr_types.h, hx_phase_out): for reads without haplotags from a diploid sample, a two-copy repeat or a mixed
 *                     amplicon. Alignment, graph, rank order, columns and weights are hx_poa_weighted's for the same sets. On the set's MSA
 *                     columns the call finds the sites (the second most frequent allele - a letter, or a gap inside a read's span - is seen
 *                     min_count times and in min_pct per cent of the column's depth), splits the reads at the site with the largest minor
 *                     count, lets every read vote over all of its sites for at most 8 rounds, and gives every haplotype hx_poa_labelled's
 *                     consensus, columns, coverage, profile and consensus row with its reads as a label. A set without a site, or with a
 *                     haplotype of fewer than min_count reads, is left unphased: n_haps 1, haplotype 0 holds every read and its consensus is
 *                     hx_poa_weighted's. All arithmetic is integer; base weights weigh the bundles, not the votes. One entry over the
 *                     convex parameters, by hx_poa_graph's rules for the gap model; weights as for hx_poa_weighted, or NULL. The errors are
 *                     hx_poa_graph's with this entry's name in front, and: min_count outside 1..255, min_pct outside 1..50 (each names the
 *                     value). Options poa_modes_slot_kb and poa_workspace_gb act as on the other entries. No band, no strands, no graph
 *                     output, two haplotypes at most. Not pinned against another program: the tests hold the rules to a CPU restatement. */
int hx_poa_phased(hx_ctx*, uint32_t n_sets, const uint64_t* set_off, const uint64_t* seq_off, const char* bases, const uint8_t* weights, const hx_poa_convex_params*, const hx_poa_phase_params*, hx_phase_out* out);
void hx_free_phase(hx_ctx*, hx_phase_out*);
void hx_free_chain(hx_ctx*, hx_chain_out*);
void hx_free_edges(hx_ctx*, hx_edges_out*);
void hx_free_coords(hx_ctx*, hx_coords_out*);
void hx_free_cns(hx_ctx*, hx_cns_out*);
void hx_free_msa(hx_ctx*, hx_msa_out*);
void hx_free_wcns(hx_ctx*, hx_wcns_out*);

/* multi-GPU exchange of the edge-support multiset (one all-gather between hx_chain_reads and the sort):
 *   hx_edge_emit            emit this shard's records (unsorted) on the device, returns their number
 *   hx_edge_records_bytes   bytes per record in the packed exchange layout (44: a forward record and its twin travel as one
 *                           88-byte unit - key, read id, compact indices and the two trimmed anchor alignments, once)
 *   hx_edge_records_export  pack the local records into a caller-owned DEVICE buffer (n * bytes; n is even): the set as hx_edge_emit or
 *                           hx_edge_records_import left it, in that order - the sort of hx_edge_support / _import works on a copy
 *   hx_edge_records_import  replace the record set by n records unpacked from a DEVICE buffer (all ranks,
 *                           rank order), then sort + segment; fills `out` like hx_edge_support */
int hx_edge_emit(hx_ctx*, const hx_params*, uint64_t* n_records);
uint32_t hx_edge_records_bytes(void);
int hx_edge_records_export(hx_ctx*, void* dst_device, uint64_t capacity_records);
int hx_edge_records_import(hx_ctx*, const void* src_device, uint64_t n_records, hx_edges_out* out);

/* Multi-GPU inside ONE process: the GPUs of a node behind the same binary, like the reference's worker threads behind asm_calc_edge_coordinates_MT
 * / asm_cal_cns_seq_MT (Assemble.cpp:453-477, :580-605, called from main.cpp:203-208). A group holds one context per rank (one host thread
 * each) and one RCCL communicator per rank (ncclCommInitAll; librccl is loaded at run time, only by this call).
 *   hx_group_create        n ranks on `devices` (NULL: ranks 0..n-1 on devices 0..n-1). `transport`: NULL = RCCL over xGMI when every rank has its
 *                          own device; "rccl" insists on it; "host" stages the exchange through host memory and lets ranks share devices (a
 *                          rehearsal of the multi-GPU logic on a box with fewer GPUs than ranks; haslr_assemble passes its HASLR_GROUP_TRANSPORT).
 *   hx_group_ctx           the rank's context: hx_upload (inputs are replicated), hx_set_read_shard, hx_set_prefiltered per rank as usual
 *   hx_edge_merge          COLLECTIVE - every rank's thread calls it once per pass, after hx_chain_reads on its read shard: emits the shard's
 *                          edge-support records, all-gathers the packed records (ONE ncclAllGather, padded to the largest shard; counts are
 *                          exchanged through the process's memory), imports the concatenation (rank order = read order), sorts and segments:
 *                          `out` like hx_edge_support, identical on every rank (bbg_build_graph's multiset, Backbone_graph.cpp:148-171).
 *                          The ranks agree on failure before the collective: if one fails there (emission, export, buffers), all return an error, none
 *                          hangs. A failure INSIDE the collective (ncclAllGather returning an error on one rank, a fault on its stream, or no
 *                          completion within hx_group_set_timeout - 300 s by default) raises the group's abort flag: every rank polls its stream
 *                          instead of blocking on it, aborts its communicator (ncclCommAbort) when it sees the flag, and all ranks return the
 *                          error; the group refuses further exchanges.
 *   hx_group_backend_fill  the rank's hx_backend table: its own chain / coordinate / consensus operators, hx_edge_merge as edge_support
 *   hx_group_exchange_stats  bytes of records exchanged by the last hx_edge_merge and its wall time in ms */
typedef struct hx_group hx_group;
int hx_group_create(int n_ranks, const int* devices, const char* transport, hx_group** out);
void hx_group_set_timeout(hx_group*, double seconds);
void hx_group_inject_fault(hx_group*, int rank); /* testing: this rank's next all-gather "returns an error" (-1: none) */
void hx_group_destroy(hx_group*);
int hx_group_size(const hx_group*);
hx_ctx* hx_group_ctx(hx_group*, int rank);
const char* hx_group_transport(const hx_group*); /* "rccl" or "host" */
int hx_edge_merge(hx_group*, int rank, const hx_params*, hx_edges_out* out);
int hx_group_backend_fill(hx_group*, int rank, void* backend_table);
void hx_group_exchange_stats(const hx_group*, uint64_t* bytes, double* ms);
int hx_group_rccl_ranks(const hx_group*, int* ranks_per_communicator /* hx_group_size entries */); /* ncclCommCount of every rank's communicator (0s: host transport); returns 1 over RCCL, 0 over host memory */

/* kernel timing measured with hipEvents on the context's stream, accumulated per kernel family since the
 * last reset: 0 chain, 1 edges (emit+sort+segment), 2 coords, 3 poa. ms[] and launches[] have 4 entries. */
void hx_timing_reset(hx_ctx*);
void hx_timing_get(hx_ctx*, double* ms, uint64_t* launches);
/* diagnostics of the last hx_poa_batch: shader-clock cycles spent by lane 0 per phase [decode, dp, traceback,
 * graph update + consensus, toposort, csr], summed over edges (sum6) and for the slowest edge (max6); returns #edges.
 * With option debug set it also prints the per-class row statistics of the call to stderr. */
uint32_t hx_poa_phase_cycles(hx_ctx*, uint64_t* sum6, uint64_t* max6);
/* bytes of POA workspace (all pools) the largest hx_poa_batch of this context has needed: (resident work-groups) x (largest edge of a launch
 * class) + the shared edges' own slots - not the sum over the edges of the call */
uint64_t hx_poa_workspace_bytes(const hx_ctx*);
/* memory of the consensus stage: device memory free when the context first ran a consensus (the budget is 90 % of it unless option
 * poa_workspace_gb says otherwise), the budget, and the workspace the LAST call settled on (slot counts are scaled down until it fits) */
/* frees the consensus workspace (the pools grow to the largest call and otherwise live as long as the context) and forgets the memory budget: the next
 * consensus call takes it again from what is free then, and allocates anew */
int hx_poa_release_workspace(hx_ctx*);
/* The consensus workspace is ONE device allocation (an arena every pool of a batch is carved from), made by the first hx_poa_batch that needs it - or
 * ahead of it by hx_poa_reserve(bytes): a one-shot program (the reference is one, main.cpp:28-228: every stage runs exactly once, the consensus at :207)
 * calls it on a thread of its own while it still parses its text inputs, so that the allocation of 10^2 GB is not part of its consensus stage. At most
 * 80 % of the device memory that is free at the time is taken (and no more than option poa_workspace_gb allows, when it is set); hx_upload gives the arena back if the inputs do not fit beside it; a call that needs more
 * than was reserved allocates again. Thread-safe against the operators of the same context. The first reservation (or, without one, the first consensus call) of a
 * process also takes the hardware queues of the launch streams to the scratch size the largest kernel instance asks for - one wave each, once per process and
 * device: queues that grow their scratch in the middle of a call hold some of its launches back.
 *   hx_poa_host_times   host wall time (ms) of the LAST consensus call, by part: [0] plan, [1] workspace (arena allocation + carving), [2] enqueue
 *                       (tables to the device, launches), [3] waiting for the device, [4] collection (status + consensus strings), [5] results
 *                       assembled, [6] unused, [7] the whole call
 *   hx_poa_arena_stats  bytes the arena holds, device allocations made for it so far, and their wall time */
int hx_poa_reserve(hx_ctx*, uint64_t bytes);
void hx_poa_host_times(const hx_ctx*, double* ms8);
void hx_poa_arena_stats(const hx_ctx*, uint64_t* capacity, uint64_t* allocations, double* alloc_ms);
void hx_poa_memory_stats(const hx_ctx*, uint64_t* free_at_first_call, uint64_t* budget, uint64_t* last_call_workspace);
/* pruning statistics of the last hx_poa_batch, summed over the pruned launches: [wave-rows, wave-rows skipped, attempts repeated, alignments with a threshold] */
void hx_poa_prune_stats(const hx_ctx*, uint64_t* out4);
/* edges (sets) the last consensus call of the tuned kNW path sent back from the kernel and ran again, counted once per round and reason: [far rows outgrew
 * H, a node with more in-edges than the direction bytes' limit (option poa_max_indeg), graph outgrew its workspace, rows with more than 4 predecessors
 * outgrew the wide-row pool, more sink rows than the launch keeps, members of a shared edge not resident together] */
void hx_poa_retry_stats(const hx_ctx*, uint64_t* out6);
/* POA work-group size: 0 = automatic (64..256 lanes per edge, ~8 DP columns per lane; gaps > 2047 columns are shared by several
 * work-groups), or force one work-group of 64/128/256/512/1024 lanes per edge (gaps up to 32767 bases) */
void hx_set_poa_block(hx_ctx*, int threads);
/* traceback source: 1 (default) = 1-byte direction codes written by the DP (an edge with a node of more than 16 in-edges is redone with 0), 0 = always re-derive the
 * moves from the int32 score matrix like the reference engine does (diagnostics / A-B comparison; results are identical) */
void hx_set_poa_traceback(hx_ctx*, int use_direction_bytes);

/* fill the host pipeline's backend table with the entry points above (struct hx_backend of haslr_host.h,
 * passed as void* to keep this header free of host-side types) */
void hx_backend_fill(hx_ctx*, void* backend_table);

#ifdef __cplusplus
}
#endif
#endif
