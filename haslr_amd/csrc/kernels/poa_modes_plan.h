// poa_modes_plan.h — the host arithmetic of the general POA path (kernels/poa_modes.hip) as pure steps: what a call holds (describe), the
// plan of a round (plan_round), what follows from the statuses a round left (after_round), and the work lists and offsets of the three
// output stages (plan_msa, plan_coverage, plan_graph_out). No HIP call, no clock, no context: poa_modes_run (Run) asks these between its
// HIP calls, and tests/poa_modes_plan_driver.cpp runs them alone, without a GPU (DESIGN.md "The general path's round plan and retry rule
// are pure host steps"). Of HIP only the vector type uint2 is used.
#ifndef HX_POA_MODES_PLAN_H
#define HX_POA_MODES_PLAN_H
#include "poa_modes.h"

namespace hxk {

enum { MT_SW = 0, MT_NW = 1, MT_OV = 2 };
enum { GM_LINEAR = 0, GM_AFFINE = 1, GM_CONVEX = 2 };   // PoaModesArgs::gap_model
enum { MS_OK = 0, MS_H_OVERFLOW = 1, MS_GRAPH_OVERFLOW = 2, MS_ALN_OVERFLOW = 3, MS_BAND_MISS = 4 };   // (3: done, but its alignments outgrew their share of the pool; 4: an alignment had no reachable end cell in its band)
constexpr uint32_t MAX_SET_BASES = (1u << 21) - 2;   // node ids are packed in 21 bits (+1) in the node records of poa_graph.inl

struct MSet { uint64_t seq_begin, sum_len, cns_off; uint32_t nseq, lmax; };

// the instances: workgroup lanes x columns per lane; a set goes to the first whose NT x CPL columns hold its longest sequence + 1.
// By gap model (GM_LINEAR, GM_AFFINE, GM_CONVEX). The affine instances keep two accumulators per column (diagonal and F): 16 columns per
// lane throughout, more lanes instead. The convex ones keep three (diagonal, F and O) and stop at 512 lanes, two waves per SIMD with up to
// 256 registers each: 1024 lanes would have 128 and spill the row (DESIGN.md "Convex gaps"). HX_POA_INSTANCES_LINEAR, _AFFINE and
// _CONVEX(X) list them as X(GM, NT, CPL); they stay defined for the includer: the kernel table of poa_modes.hip (kInst) is generated
// from the same lists.
constexpr int N_INST = 4;
#define HX_POA_INSTANCES_LINEAR(X) X(GM_LINEAR, 64, 16), X(GM_LINEAR, 256, 16), X(GM_LINEAR, 256, 32), X(GM_LINEAR, 1024, 32)
#define HX_POA_INSTANCES_AFFINE(X) X(GM_AFFINE, 64, 16), X(GM_AFFINE, 256, 16), X(GM_AFFINE, 512, 16), X(GM_AFFINE, 1024, 16)
#define HX_POA_INSTANCES_CONVEX(X) X(GM_CONVEX, 64, 16), X(GM_CONVEX, 128, 16), X(GM_CONVEX, 256, 16), X(GM_CONVEX, 512, 16)
struct InstShape { int nt, cpl; };
#define HX_SHAPE(GM, NT, CPL) {NT, CPL}
constexpr InstShape INST_SHAPE[3][N_INST] = {{HX_POA_INSTANCES_LINEAR(HX_SHAPE)}, {HX_POA_INSTANCES_AFFINE(HX_SHAPE)}, {HX_POA_INSTANCES_CONVEX(HX_SHAPE)}};
#undef HX_SHAPE
constexpr uint32_t MAX_LEN[3] = {1024 * 32 - 1, 1024 * 16 - 1, 512 * 16 - 1};
constexpr uint64_t CELL_BYTES[3] = {4, 8, 12};   // of a cell of H by gap model: what the kernels take as sizeof(Cell<GM>)
// The band instance (PoaModesArgs::band; DESIGN.md "Banded alignment"): one shape for the three gap models, one wavefront that holds a window of
// 2 w + 1 <= 1023 columns. It is slot BAND_INST of a round's plan, behind the N_INST full-matrix instances: a call without a band never names it.
constexpr int BAND_INST = N_INST, N_SLOTS = N_INST + 1;
constexpr InstShape BAND_SHAPE = {64, 16};
constexpr int64_t BAND_SCORE_BOUND = 1 << 28;   // (bases of a set + its longest sequence) x the largest score magnitude stays below it
// Every set of the path: (its bases + the NT x CPL columns of its full-matrix instance) x the largest score magnitude stays below it, which keeps every
// cell, every scan term and every sum with minus infinity of dp_rows inside int32 and on its side of -2^29 (DESIGN.md "Score range of the full matrix")
constexpr int64_t SCORE_BOUND = 1 << 29;
inline InstShape shape_of(int gm, int k) { return k == BAND_INST ? BAND_SHAPE : INST_SHAPE[gm][k]; }
static_assert(MAX_LEN[GM_LINEAR] + 1 == INST_SHAPE[GM_LINEAR][N_INST - 1].nt * INST_SHAPE[GM_LINEAR][N_INST - 1].cpl && MAX_LEN[GM_AFFINE] + 1 == INST_SHAPE[GM_AFFINE][N_INST - 1].nt * INST_SHAPE[GM_AFFINE][N_INST - 1].cpl &&
              MAX_LEN[GM_CONVEX] + 1 == INST_SHAPE[GM_CONVEX][N_INST - 1].nt * INST_SHAPE[GM_CONVEX][N_INST - 1].cpl, "MAX_LEN against the widest instance of every gap model");

// ---- a call: what never changes after describe()
struct ModesCall {
    const PoaModesArgs* a = nullptr;
    std::string who;
    uint32_t ns = 0;
    int gm = 0;                                              // GM_LINEAR, GM_AFFINE or GM_CONVEX (the entry points set nothing else)
    bool msa = false;
    bool wtd = false;                                        // hx_poa_weighted: the node of every base is kept, as for the MSA
    bool graph = false;                                      // hx_poa_graph: the node of every base stays a node, the graph and the alignments are written out
    bool strand = false;                                     // hx_poa_strand: every sequence in both orientations; MSA text, coverage and profile as asked
    bool cols = false, want_cov = false;
    bool band = false;                                       // hx_poa_banded: sets run inside an adaptive band as long as they do not miss it
    bool labels = false;                                     // hx_poa_labelled: one consensus per label and set over the set's one graph
    uint32_t nl = 1;                                         // consensus places per set: the call's n_labels, 1 without labels
    bool phase = false;                                      // hx_poa_phased: a labelled call (labels is set, nl is 2) whose labels the device derives
    const uint8_t* lab = nullptr;                            // labelled calls: the label of every sequence (the caller's; phased calls: what poa_modes_run downloaded, null until then)
    uint64_t nseq = 0, nb = 0;
    std::vector<MSet> sets;
    std::vector<uint64_t> cns_off;                           // ns x nl + 1: place g of set i is entry i x nl + g
    std::vector<uint8_t> codes;                              // the bases as 0..3
    std::vector<uint8_t> codes_rc, wts_rc;                   // strand calls: every sequence reverse-complemented at its own offset, its weights reversed with it
    uint64_t seq_bases = 0, n_aligned = 0;                   // (PoaModesOut's)
};

// ---- and what the rounds change
struct ModesState {
    std::vector<uint64_t> vest;      // per set: the estimate of its graph's final size that its H is sized from
    std::vector<uint32_t> todo;      // the sets of the next round
    // graph calls only. The alignment pool is one allocation per round (a rerun set's share lies in a later round's pool; pool_of / aln_at
    // tell where a set's pairs are after the last round it ran in)
    std::vector<uint32_t> pool_of, aln_room, aln_rerun;   // per set: the round of its share, the share in pairs, 1 once it was rerun for want of room
    std::vector<uint64_t> aln_at;
    uint32_t rounds = 0;             // planned so far
    uint32_t retried = 0, aln_retried = 0;   // sets rerun in a larger slot, sets rerun because their alignments outgrew their share
    // banded calls only: per set the half-width of its current attempt (0: the full matrix), and the reruns after a band miss
    std::vector<uint32_t> band;
    uint32_t band_retried = 0;
};

// the graph pools of a set in bytes: carve_pools (poa_modes_pools.inl) itself, asked without a slot
uint64_t pools_bytes(const MSet& S);
// the phase pool of a set in bytes (phased calls: behind the graph pools of the set's slot): carve_phase (poa_modes_pools.inl) itself
uint64_t phase_pool_bytes(uint64_t sum_len, uint32_t nseq);
// what a set's slot holds in front of H: the graph pools, and in a phased call the phase pool
uint64_t slot_pools_bytes(const ModesCall& c, uint32_t set);
// the first instance whose NT x CPL columns hold the set's longest sequence + 1
int inst_of(const ModesCall& c, uint32_t set);
// the slot of a round's plan a set runs in: BAND_INST while it has a half-width, else inst_of(c, set)
int slot_of(const ModesCall& c, const ModesState& st, uint32_t set);
// the half-width after a band miss at w of a set whose longest sequence is lmax: 2 w while that window holds at most 1023 columns and does
// not hold the whole sequence, else 0, the full matrix
uint32_t next_band(uint32_t w, uint32_t lmax);

// the sets checked and described, the codes, the first estimates and the first shares of the alignment pool. 0, or -1 with the reason in err
int describe(const PoaModesArgs& a, ModesCall& c, ModesState& st, std::string& err);

struct RoundPlan {
    struct PerInst { std::vector<uint32_t> sets; uint64_t base = 0, slot = 0; uint32_t nslots = 0; };   // sets: in launch order; base: their place in order
    PerInst inst[N_SLOTS];
    std::vector<uint32_t> order;
    uint64_t total = 0;        // bytes of the shared workspace
    uint64_t aln_pairs = 0;    // graph calls: the round's alignment pool
};
// one round over st.todo: per instance its sets costliest first, one slot size (the largest need), as many slots as are resident
// (resident[k]: workgroups of instance k the device holds; read for instances with sets only, so a call without a band may pass N_INST of
// them and a banded one passes N_SLOTS) and fit the budget. Graph calls: the
// shares of the round's pool side by side (st.pool_of, st.aln_at).
int plan_round(const ModesCall& c, ModesState& st, bool first, uint64_t budget, const uint64_t* resident, RoundPlan& p, std::string& err);
// the statuses of a round: st.todo becomes the sets that come back, with their new estimate or share
int after_round(const ModesCall& c, ModesState& st, bool first, const uint32_t* status, const uint32_t* vseen, const uint32_t* pairs, std::string& err);

// ---- the output stages
// the work list of a grid-wide row kernel (k_msa_rows, k_cov_hist, k_cov_gather, k_graph_gather): one descriptor per row and one chunk
// (row, first element) per 64 elements of it, one wavefront each. A row without elements still gets its one chunk (the MSA row of an empty sequence).
template <class Row> struct RowPlan {
    std::vector<Row> rows; std::vector<uint2> chunks;
    void add(const Row& r, uint32_t n) {
        for (uint32_t f = 0; f == 0 || f < n; f += 64) chunks.push_back(make_uint2((uint32_t)rows.size(), f));
        rows.push_back(r);
    }
    bool too_many() const { return rows.size() >= 0xffffffffULL || chunks.size() >= 0xffffffffULL / 64; }
    uint32_t n_chunks() const { return (uint32_t)chunks.size(); }
    uint32_t blocks() const { return (uint32_t)((chunks.size() + 3) / 4); }   // of 256 lanes
};
// the rows as the plan knows them; poa_modes.hip turns each into the kernel's descriptor (MRow, CRow, GRow) as it uploads
struct MsaRow { uint64_t src, dst; uint32_t len, ncols, is_cns; };
struct CovRow { uint64_t src, dst, hoff; uint32_t len, ncols; };
enum { ROW_NODES = 0, ROW_EDGES = 1, ROW_CNS = 2, ROW_ALN = 3 };
struct GraphRow { uint64_t src, dst; uint32_t len, kind; uint32_t round; };   // ROW_ALN: src is a place in the alignment pool of that round

// ncols: per set its columns; len: the length of every consensus (per set, labelled calls: per set and label, as cns_off);
// out_cns_off: PoaModesOut::cns_off. A labelled call counts per set and label (one counter block each, the blocks of a set side by
// side; a sequence without a label counts nowhere) and has one consensus row per label, in label order, behind a set's sequences
struct MsaPlan { RowPlan<MsaRow> rows; std::vector<uint32_t> msa_rows; std::vector<uint64_t> msa_off; uint64_t out_bytes = 0, moved_bytes = 0; };
int plan_msa(const ModesCall& c, const std::vector<uint32_t>& ncols, const std::vector<uint32_t>& len, const std::vector<uint64_t>& out_cns_off, MsaPlan& p, std::string& err);

struct CovPlan { RowPlan<CovRow> seqs, cnss; uint32_t stride = 1; uint64_t hist_words = 0, nc = 0, moved_bytes = 0; };
int plan_coverage(const ModesCall& c, const std::vector<uint32_t>& ncols, const std::vector<uint32_t>& len, const std::vector<uint64_t>& out_cns_off, CovPlan& p, std::string& err);

// nv, ne: per set its nodes and edges; cnt: per sequence the pairs of its alignment
struct GraphPlan { RowPlan<GraphRow> rows; std::vector<uint64_t> node_off, edge_off, aln_off; uint64_t NV = 0, NE = 0, NC = 0, NP = 0, moved_bytes = 0; };
int plan_graph_out(const ModesCall& c, const ModesState& st, const std::vector<uint32_t>& nv, const std::vector<uint32_t>& ne, const std::vector<uint32_t>& cnt, const std::vector<uint32_t>& len,
                   const std::vector<uint64_t>& out_cns_off, GraphPlan& p, std::string& err);

}  // namespace hxk
#endif
