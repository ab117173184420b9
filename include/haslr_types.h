/* haslr_types.h — plain-C data layouts shared by the C-ABI (haslr_hip.h), the host
 * pipeline and the test oracle. Everything is structure-of-arrays: on the device each
 * array is one contiguous HBM allocation so that a wavefront's 64 lanes read 64
 * consecutive elements (coalesced), which the reference's 48-byte AoS `Align_Seq_t`
 * (Longread.hpp:32-48) does not allow.
 *
 * Reference types these replace (all under /root/reference/src/haslr_assemble/src):
 *   Align_Seq2_t / Align_Seq_t   Longread.hpp:16-48     -> hx_hits (raw) + hx_alns (surviving)
 *   Longread_t / Longread_List_t Longread.hpp:50-77     -> hx_reads
 *   Contig_t / Contig_List_t     Contig.hpp:14-32       -> hx_contigs
 *   Edge_Supp_t                  Backbone_graph.hpp:23-29 -> hx_edge_recs (key + lr + cmp ids [+ hit copies])
 *   Consensus_Supp_t             Backbone_graph.hpp:31-37 -> hx_coords (supp_lr/spos/epos)
 */
#ifndef HASLR_TYPES_H
#define HASLR_TYPES_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* CIGAR op word: (length << 2) | code. Codes keep the distinctions the reference makes when it
 * walks a per-base expanded CIGAR (Longread.cpp:384-396 forward, :401-413 undo; Assemble.cpp:141-153):
 * 'M' consumes read+contig, 'I' read only, anything else contig only; but only a literal 'D' is undone. */
enum { HX_CG_M = 0, HX_CG_I = 1, HX_CG_D = 2, HX_CG_OTHER = 3 };
#define HX_CG_LEN(w) ((uint32_t)(w) >> 2)
#define HX_CG_OP(w) ((uint32_t)(w) & 3u)

/* Options of the stage (Common.hpp:44-65, defaults Commandline.cpp:46-66). */
typedef struct {
    uint32_t min_aln_block; /* --aln-block, 500 */
    double min_aln_sim;     /* --aln-sim, 0.85 */
    uint32_t min_aln_mapq;  /* hard-wired 55 (Commandline.cpp:60) */
    double max_uniq_dev;    /* --uniq-dev, 0.15 */
    uint32_t min_edge_sup;  /* --edge-sup, 3 */
    double uniq_freq;       /* calc_uniq_freq, Contig.cpp:162-174 */
} hx_params;

/* Short-read contigs: what the filters look up (Contig_t.mean_kmer, .len). */
typedef struct {
    uint32_t n;
    const double* mean_kmer;
    const uint32_t* len;
} hx_contigs;

/* Long reads: 2-bit packed bases. Layout is the build's own (NOT the reference's reversed-byte
 * codec, Compressed_sequence.cpp:46-62): base i of a read lives in byte off+i/4, bits 2*(i%4),
 * A=0 C=1 G=2 T=3, and anything else packs as A exactly like the reference (`_dna_tableVal[..] & 3`).
 * Every read starts on a 4-byte boundary so a lane can fetch 16 bases with one aligned dword. */
typedef struct {
    uint32_t n;
    const uint32_t* len;   /* bases */
    const uint64_t* off;   /* byte offset of read i in `packed`; n+1 entries, multiples of 4 */
    const uint8_t* packed;
} hx_reads;

/* Raw PAF records, one per PAF line, in file order (Align_Seq2_t minus q_len, plus CIGAR ops). */
typedef struct {
    uint64_t n;
    const uint32_t *q_id, *q_start, *q_end, *t_id, *t_len, *t_start, *t_end, *n_match, *n_block;
    const uint8_t *is_rev, *mapq;
    const uint64_t* cg_off; /* n+1 */
    const uint32_t* cg_ops; /* cg_off[n] words */
} hx_hits;

/* Surviving alignments after filters 1-5 + palindrome rule, grouped by read in (q_end,q_start) order,
 * then overlap-trimmed (the reference's `alignments` arena after fix_alignments, Longread.cpp:626).
 * A trimmed CIGAR is always a contiguous piece of the raw one: ops [cg_begin,cg_end) with
 * cg_skip_front bases removed from the first op and cg_skip_back from the last. */
typedef struct {
    uint64_t n_aln;
    uint32_t n_reads;
    uint32_t* hit; /* index into hx_hits */
    uint32_t *q_start, *q_end, *t_start, *t_end, *n_match, *n_block;
    uint64_t *cg_begin, *cg_end;
    uint32_t *cg_skip_front, *cg_skip_back;
    uint64_t* read_off; /* n_reads+1: alignments of read r are [read_off[r], read_off[r+1]) */
    /* compact long reads (find_best_scheduling, Longread.cpp:524-610) */
    uint64_t n_cmp;
    uint64_t* cmp_off; /* n_reads+1 */
    uint32_t* cmp_aln; /* global alignment index of each compact element */
} hx_chain_out;

/* One side (head or tail) of an edge-support record: a copy of the compact element it points at, so
 * that a record is self-contained after the multi-GPU all-gather (raw CIGAR ops and packed reads are
 * replicated on every GPU; the alignment table is not). */
typedef struct {
    uint32_t *q_start, *q_end, *t_start, *t_end;
    uint8_t* is_rev;
    uint64_t *cg_begin, *cg_end;
    uint32_t *cg_skip_front, *cg_skip_back;
} hx_rec_side;

/* Edge-support multiset, sorted by (key, emission order) which reproduces the reference's per-edge
 * `edge_supp` vectors (Backbone_graph.cpp:10-25,148-171).  key = (n1<<1|rev1)<<32 | (n2<<1|rev2):
 * high word = source vertex (node, which end is left), low word = the reference's map key. */
typedef struct {
    uint64_t n_rec;
    uint64_t* key;
    uint32_t* lr; /* lr_id | lr_strand<<31 */
    uint32_t *cmp_head, *cmp_tail;
    hx_rec_side head, tail;
    uint64_t n_edge;
    uint64_t* edge_key;
    uint64_t* edge_off; /* n_edge+1; support count = edge_off[e+1]-edge_off[e] */
} hx_edges_out;

/* Per processed edge (asm_calc_single_edge_coordinates, Assemble.cpp:157-363). */
typedef struct {
    uint32_t n_edge;
    uint32_t *head_end, *tail_beg;
    uint64_t* supp_off; /* n_edge+1 */
    uint32_t *supp_lr;  /* lr_id | lr_strand<<31 */
    uint32_t *spos, *epos;
} hx_coords_out;

/* Per processed edge consensus (asm_calc_single_cns_seq, Assemble.cpp:479-560): ASCII ACGT. */
typedef struct {
    uint32_t n_edge;
    uint64_t* cns_off; /* n_edge+1 */
    char* cns;
    /* work counters, for the roofline report */
    uint64_t dp_cells;   /* sum over alignments of graph_nodes * seq_len (what the full-matrix reference computes) */
    uint64_t seq_bases;  /* bases fed to POA */
    uint64_t n_aligned;  /* sequences aligned */
} hx_cns_out;

/* POA scoring (Assemble.cpp:8-11): global NW, linear gap. */
typedef struct {
    int32_t match, mismatch, gap;
} hx_poa_params;

/* POA alignment type and scoring of hx_poa_sequences_mode: spoa's AlignmentType values (kSW local, kNW global, kOV overlap), linear gap. */
typedef enum { HX_POA_SW = 0, HX_POA_NW = 1, HX_POA_OV = 2 } hx_poa_type;
typedef struct {
    int32_t match, mismatch, gap;
    int32_t type; /* hx_poa_type */
} hx_poa_mode_params;

/* hx_poa_sequences_affine: the same with affine gaps. A gap of k bases costs gap_open + (k - 1) gap_extend;
 * gap_open < 0, gap_extend <= 0, gap_open <= gap_extend (gap_extend == gap_open is the linear model). */
typedef struct {
    int32_t match, mismatch, gap_open, gap_extend;
    int32_t type; /* hx_poa_type */
} hx_poa_affine_params;

/* hx_poa_sequences_convex, hx_poa_msa_convex, hx_poa_weighted_convex: two-piece affine ("convex") gaps. A gap of k bases scores
 * max(gap_open + (k - 1) gap_extend, gap_open2 + (k - 1) gap_extend2). Each piece is a valid affine one (open < 0, extend <= 0,
 * open <= extend), and gap_open2 <= gap_open: the first piece is the one that opens no dearer. gap_extend2 <= gap_extend: the second
 * piece never wins, the call is the affine one with the first piece. */
typedef struct {
    int32_t match, mismatch, gap_open, gap_extend, gap_open2, gap_extend2;
    int32_t type; /* hx_poa_type */
} hx_poa_convex_params;

/* hx_poa_msa: hx_poa_sequences_affine's scores and type (gap_extend == gap_open is the linear model), and whether the consensus is
 * the last row of every set. */
typedef struct {
    int32_t match, mismatch, gap_open, gap_extend;
    int32_t type; /* hx_poa_type */
    int32_t include_consensus; /* 0 / 1 */
} hx_poa_msa_params;

/* Multiple sequence alignment of every set (spoa's generate_multiple_sequence_alignment): set i is n_rows[i] rows of n_cols[i]
 * characters (ACGT and '-'), row-major without terminators, at msa + msa_off[i]. One row per GIVEN sequence, in the given order (an
 * empty sequence: a row of gaps), then the consensus row when it was asked for; a set without a non-empty sequence has no column.
 * The consensus strings and the work counters are hx_cns_out's. */
typedef struct {
    uint32_t n_set;
    uint32_t* n_rows;  /* n_set */
    uint32_t* n_cols;  /* n_set */
    uint64_t* msa_off; /* n_set+1; msa_off[i+1] - msa_off[i] = n_rows[i] * n_cols[i] */
    char* msa;
    uint64_t* cns_off; /* n_set+1 */
    char* cns;
    uint64_t dp_cells, seq_bases, n_aligned;
    /* the kernel that writes the rows, on its own: its time by device events and the bytes it has to move (text + 4 per base read) */
    double rows_kernel_ms;
    uint64_t rows_kernel_bytes;
} hx_msa_out;

/* hx_poa_weighted: hx_poa_sequences_affine's scores and type (gap_extend == gap_open is the linear model), and what is wanted beside
 * the consensus. */
typedef struct {
    int32_t match, mismatch, gap_open, gap_extend;
    int32_t type;          /* hx_poa_type */
    int32_t want_coverage; /* 0 / 1: the coverage of every consensus base */
    int32_t want_profile;  /* 0 / 1: and the four letter counts of its column (the coverage is filled in as well) */
} hx_poa_weighted_params;

/* Consensus of every set under per-base weights, with the coverage of every consensus base (spoa's generate_consensus(dst)): the
 * number of sequences of two or more bases that have a base in the consensus base's column of the alignment. coverage has one entry per
 * consensus base, at the base's offset in cns; profile has four (A, C, G, T: the sequences counted in the coverage by their letter in
 * that column; the rest of the set's sequences have a gap there). Both are NULL unless asked for. The consensus strings and the work
 * counters are hx_cns_out's. */
typedef struct {
    uint32_t n_set;
    uint64_t* cns_off;  /* n_set+1 */
    char* cns;
    uint32_t* coverage; /* cns_off[n_set], or NULL */
    uint32_t* profile;  /* 4 * cns_off[n_set], or NULL */
    uint64_t dp_cells, seq_bases, n_aligned;
    /* the kernels that count and gather the coverage, on their own: their time by device events and the bytes they have to move */
    double cov_kernel_ms;
    uint64_t cov_kernel_bytes;
} hx_wcns_out;

/* hx_poa_graph: the partial-order graph of every set as it stands after its last sequence, the path of every sequence through it and the
 * alignment of every sequence against the graph as it was before that sequence was added (DESIGN.md "General POA path", "Graph and
 * alignment output"). Node and edge ids are set-local. Nodes are in creation order (spoa's ids), edges in the order add_edge first made
 * them: the edges out of (into) a node, taken in edge-id order, are spoa's out-list (in-list) order.
 *   nodes   set i: node_off[i] .. node_off[i+1]. node_base the letter, node_rank the node's place in spoa's topological order (what the DP
 *           of one more sequence would use), node_col its MSA column (hx_poa_msa's): aligned nodes are the nodes that share a column.
 *   edges   set i: edge_off[i] .. edge_off[i+1]. edge_w is spoa's total weight (a sequence adds w[p-1] + w[p]: 2 on unit weights).
 *   paths   base_node[p] is the node of base p of `bases` (the caller's seq_off indexes it).
 *   consensus  cns / cns_off as in hx_cns_out, cns_node the node of every consensus base.
 *   alignments  sequence k of the call (all sets, in order; n_seq of them): pairs aln_off[k] .. aln_off[k+1] of (aln_node | -1, aln_pos |
 *           -1) in spoa's forward order, and aln_score[k], the score of the DP's end cell. A sequence that met no DP (an empty one, the
 *           first non-empty one of its set, a local alignment without a cell above 0) has no pair and score 0. */
typedef struct {
    uint32_t n_set;
    uint64_t n_seq;
    uint64_t* node_off; /* n_set+1 */
    char* node_base;
    uint32_t *node_rank, *node_col;
    uint64_t* edge_off; /* n_set+1 */
    uint32_t *edge_from, *edge_to;
    int32_t* edge_w;
    uint32_t* base_node; /* one per base of the call */
    uint64_t* cns_off;   /* n_set+1 */
    char* cns;
    uint32_t* cns_node; /* cns_off[n_set] */
    uint64_t* aln_off;  /* n_seq+1 */
    int32_t *aln_node, *aln_pos;
    int32_t* aln_score; /* n_seq */
    uint64_t dp_cells, seq_bases, n_aligned;
    /* the kernel that gathers the dense arrays, on its own: its time by device events and the bytes it has to move (every element of the
     * node, edge, consensus-node and alignment arrays read once and written once) */
    double gather_kernel_ms;
    uint64_t gather_kernel_bytes;
    /* sets that ran again: in a larger workspace slot, and because their alignments outgrew their share of the alignment pool */
    uint32_t slot_reruns, aln_reruns;
} hx_graph_out;

/* hx_poa_strand: what is wanted beside the consensus, the flags and the scores. */
typedef struct {
    int32_t want_msa;          /* 0 / 1: the alignment text of every set */
    int32_t include_consensus; /* 0 / 1: with want_msa, the consensus is the last row of every set */
    int32_t want_coverage;     /* 0 / 1: the coverage of every consensus base */
    int32_t want_profile;      /* 0 / 1: and the four letter counts of its column (the coverage is filled in as well) */
} hx_poa_strand_want;

/* hx_poa_strand: the consensus of sets whose sequences may lie on either strand (DESIGN.md "General POA path", "Strand-ambiguous
 * sets"). Per GIVEN sequence k of the call (all sets, in order; n_seq of them): reversed[k] is 1 when its reverse complement was the
 * orientation added to the graph, score_fwd[k] and score_rev[k] are the end-cell scores of the sequence and of its reverse complement
 * against the graph as it stood (both 0 for an empty sequence and for a set's first non-empty one, which meet no DP). Everything else
 * sees a sequence as it was added: the MSA row of a reversed sequence is its gapped reverse complement, coverage and profile count its
 * complemented letters. n_rows / n_cols / msa_off / msa are hx_msa_out's (NULL unless want_msa), coverage / profile hx_wcns_out's (NULL
 * unless asked for). dp_cells counts both orientations (2 x nodes x length per aligned sequence); third_passes the sequences whose
 * reverse complement won, each of which cost one more DP pass; slot_reruns the sets that ran again in a larger workspace slot. */
typedef struct {
    uint32_t n_set;
    uint64_t n_seq;
    uint64_t* cns_off; /* n_set+1 */
    char* cns;
    uint8_t* reversed;  /* n_seq */
    int32_t* score_fwd; /* n_seq */
    int32_t* score_rev; /* n_seq */
    uint32_t* n_rows;   /* n_set, or NULL */
    uint32_t* n_cols;   /* n_set, or NULL */
    uint64_t* msa_off;  /* n_set+1, or NULL */
    char* msa;          /* or NULL */
    uint32_t* coverage; /* cns_off[n_set], or NULL */
    uint32_t* profile;  /* 4 * cns_off[n_set], or NULL */
    uint64_t dp_cells, seq_bases, n_aligned, third_passes;
    uint32_t slot_reruns;
} hx_strand_out;

/* hx_poa_banded: the half-width of the adaptive band, and what is wanted beside the consensus (hx_poa_strand_want's four switches). */
typedef struct {
    uint32_t band;             /* the half-width w, 1..511: every row of the score matrix owns 2 w + 1 columns */
    int32_t want_msa;          /* 0 / 1: the alignment text of every set */
    int32_t include_consensus; /* 0 / 1: with want_msa, the consensus is the last row of every set */
    int32_t want_coverage;     /* 0 / 1: the coverage of every consensus base */
    int32_t want_profile;      /* 0 / 1: and the four letter counts of its column (the coverage is filled in as well) */
} hx_poa_band_params;

/* hx_poa_banded: the consensus of sets aligned inside an adaptive band (DESIGN.md "General POA path", "Banded alignment"). band_used[i]
 * is the half-width of the attempt that gave set i's result: the call's, a doubled one after band misses, or 0 for the full matrix (a
 * set whose longest sequence + 1 fits the window, or one that missed every band). n_rows / n_cols / msa_off / msa are hx_msa_out's (NULL
 * unless want_msa), coverage / profile hx_wcns_out's (NULL unless asked for). dp_cells counts, over the alignments of every set's final
 * attempt, nodes x min(2 w + 1, length + 1) inside a band and nodes x length on the full matrix. slot_reruns: the sets that ran again
 * in a larger workspace slot; band_reruns: the reruns after a band miss (a set counts once per rung it climbs); workspace_bytes: the
 * largest workspace a round of the call asked for. */
typedef struct {
    uint32_t n_set;
    uint64_t* cns_off;   /* n_set+1 */
    char* cns;
    uint32_t* band_used; /* n_set */
    uint32_t* n_rows;    /* n_set, or NULL */
    uint32_t* n_cols;    /* n_set, or NULL */
    uint64_t* msa_off;   /* n_set+1, or NULL */
    char* msa;           /* or NULL */
    uint32_t* coverage;  /* cns_off[n_set], or NULL */
    uint32_t* profile;   /* 4 * cns_off[n_set], or NULL */
    uint64_t dp_cells, seq_bases, n_aligned, workspace_bytes;
    uint32_t slot_reruns, band_reruns;
} hx_band_out;

/* hx_poa_labelled: the number of labels, and what is wanted beside the consensus strings and their columns (hx_poa_strand_want's four
 * switches). */
typedef struct {
    uint32_t n_labels;         /* 1..16: a sequence's label is 0 .. n_labels - 1, or 255 for none */
    int32_t want_msa;          /* 0 / 1: the alignment text of every set */
    int32_t include_consensus; /* 0 / 1: with want_msa, one consensus row per label behind the rows of every set */
    int32_t want_coverage;     /* 0 / 1: the coverage of every consensus base within its label */
    int32_t want_profile;      /* 0 / 1: and the four letter counts of its column within its label (the coverage is filled in as well) */
} hx_poa_label_params;

/* hx_poa_labelled: one consensus per label over the one graph of every set (DESIGN.md "General POA path", "Per-label consensus"). The
 * consensus of label g of set i is entry i * n_labels + g: cns[cns_off[i * n_labels + g] .. cns_off[i * n_labels + g + 1]). cns_col holds
 * the MSA column of every consensus base; the columns are the set's and shared by its labels. coverage / profile (NULL unless asked for)
 * count, per consensus base, the label's own sequences of two or more bases with a base in that column. n_rows / n_cols / msa_off / msa
 * are hx_msa_out's (NULL unless want_msa): with include_consensus a set has n_labels more rows, label after label. dp_cells, seq_bases
 * and n_aligned are hx_poa_weighted's on the same sets; slot_reruns the sets that ran again in a larger workspace slot. */
typedef struct {
    uint32_t n_set, n_labels;
    uint64_t* cns_off;  /* n_set * n_labels + 1 */
    char* cns;
    uint32_t* cns_col;  /* cns_off[n_set * n_labels] */
    uint32_t* coverage; /* cns_off[n_set * n_labels], or NULL */
    uint32_t* profile;  /* 4 * cns_off[n_set * n_labels], or NULL */
    uint32_t* n_rows;   /* n_set, or NULL */
    uint32_t* n_cols;   /* n_set, or NULL */
    uint64_t* msa_off;  /* n_set+1, or NULL */
    char* msa;          /* or NULL */
    uint64_t dp_cells, seq_bases, n_aligned;
    uint32_t slot_reruns;
} hx_label_out;

/* hx_poa_phased: the two thresholds of the site rule, and what is wanted beside the consensus strings and their columns (hx_poa_strand_want's
 * four switches). */
typedef struct {
    uint32_t min_count;        /* 1..255 (2 is a sound default): a column is a site if its second allele is seen at least this often ... */
    uint32_t min_pct;          /* 1..50 (25 is a sound default): ... and in at least this share, in per cent rounded up, of the column's depth */
    int32_t want_msa;          /* 0 / 1: the alignment text of every set */
    int32_t include_consensus; /* 0 / 1: with want_msa, one consensus row per haplotype (two) behind the rows of every set */
    int32_t want_coverage;     /* 0 / 1: the coverage of every consensus base within its haplotype */
    int32_t want_profile;      /* 0 / 1: and the four letter counts of its column within its haplotype (the coverage is filled in as well) */
} hx_poa_phase_params;

/* hx_poa_phased: two-haplotype consensus with automatic read phasing (DESIGN.md "General POA path", "Two-haplotype consensus"). The first
 * fields are hx_label_out's, at its offsets, for n_labels = 2 with the haplotypes as labels: the consensus of haplotype h of set i is entry
 * 2 i + h. hap holds a byte per sequence of the call: 0, 1, or 255 (an empty sequence, or one that no site assigned). n_haps is 2, or 1
 * where the set was left unphased: then every non-empty sequence is in haplotype 0 and haplotype 1's consensus is empty. rounds: the voting
 * rounds run (0 without a site, at most 8). The sites of set i are entries site_off[i] .. site_off[i + 1], in column order: the MSA column,
 * its two most frequent alleles (0..3 A C G T, 4 a gap inside a read's span) and the phase: +1 haplotype 0 carries a1, -1 it carries a2,
 * 0 undecided or unphased. */
typedef struct {
    uint32_t n_set, n_labels;
    uint64_t* cns_off;  /* n_set * 2 + 1 */
    char* cns;
    uint32_t* cns_col;  /* cns_off[n_set * 2] */
    uint32_t* coverage; /* cns_off[n_set * 2], or NULL */
    uint32_t* profile;  /* 4 * cns_off[n_set * 2], or NULL */
    uint32_t* n_rows;   /* n_set, or NULL */
    uint32_t* n_cols;   /* n_set, or NULL */
    uint64_t* msa_off;  /* n_set+1, or NULL */
    char* msa;          /* or NULL */
    uint64_t dp_cells, seq_bases, n_aligned;
    uint32_t slot_reruns;
    uint8_t* hap;        /* one per sequence of the call */
    uint32_t* n_haps;    /* n_set */
    uint32_t* rounds;    /* n_set */
    uint64_t* site_off;  /* n_set+1 */
    uint32_t* site_col;  /* site_off[n_set] */
    uint8_t* site_a1;    /* site_off[n_set] */
    uint8_t* site_a2;    /* site_off[n_set] */
    int8_t* site_phase;  /* site_off[n_set] */
} hx_phase_out;

#ifdef __cplusplus
}
#endif
#endif
