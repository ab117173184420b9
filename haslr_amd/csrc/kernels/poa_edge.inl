// poa_edge.inl - part of kernels/poa.hip: the names of what crosses the phases of poa_edge - the edge's state, the words of the members' handshake, the words the
// traceback walk shares with its helper wave - with the steps of the handshake and the binding of the edge's views into the pools.

// ---- the edge's state (poa_edge's sOk): ES_OK while the edge is being worked on; anything else ends it, and the end of poa_edge turns it into the status word the host reads
enum EdgeState : uint32_t {
    ES_OVERFLOW = 0,    // the graph outgrows its workspace: the host retries with more
    ES_OK = 1,
    ES_INTERNAL = 2,    // the kernel variant cannot hold this many columns per lane, no LDS for a row, a walk that did not end, a carry lost inside a workgroup
                        // (3: unused)
    ES_NODIR = 4,       // a row with more predecessors than a direction byte holds: the host retries with the score-matrix traceback
    ES_FARROWS = 5,     // more rows read back from HBM than the estimate: the host retries with a row per node
    ES_SINKS = 6,       // more sink rows than the launch keeps: the host redoes the edge in a launch with the full list
    ES_WIDEROWS = 7,    // more rows with more than 4 predecessors than the estimate: the host retries with more
    ES_STALLED = 8      // a member gave up waiting for another one (the members were not resident together): the host redoes the edge unshared
};

// ---- the cluster handshake: the words the members of a shared edge talk through (PoaPools::csync, CW_STRIDE words per edge; relaxed device-scope atomics).
// Member 0 publishes every DP it wants - a new sequence, or the same one again under another threshold (PRUNE) - as {V, L, threshold} and a rising attempt
// number in CW_GO; the other members run one DP per attempt, whatever it is, add themselves to CW_DONE, and wait for the next number or for the release
// (CL_ABORT, written by member 0 when it leaves the loop for whatever reason). They do not count sequences.
enum ClusterWord : uint32_t {
    CW_GO = 0,          // the attempt member 0 wants (rising), or CL_ABORT
    CW_DONE = 1,        // + 1 per member and attempt
    CW_V = 2, CW_L = 3, // rows and columns of the attempt
    CW_ERR = 4,         // a waiter gave up (DpCl::err): 1 between workgroups, 2 inside one
    CW_THRESHOLD = 5,   // PRUNE: the attempt's threshold
    CW_STRIDE = 8
};
constexpr uint32_t CL_ABORT = 0xffffffffu;

// one lane: polls word w until it has reached `want` and returns it; gives up after poll_limit polls: flags the edge, returns CL_ABORT
__device__ __forceinline__ uint32_t cluster_wait(uint32_t* csy, const ClusterWord w, const uint32_t want, const uint32_t poll_limit) {
    uint32_t v = 0;
    for (uint32_t spin = 0;; spin++) {
        v = ld_dev(csy + w);
        if (v >= want) break;
        if (spin > poll_limit) { st_dev(csy + CW_ERR, 1u); v = CL_ABORT; break; }
        __builtin_amdgcn_s_sleep(32);
    }
    return v;
}
// member 0, all lanes: waits until every other member has done attempt `att`
__device__ __forceinline__ void cluster_wait_members(uint32_t* csy, const uint32_t GM, const uint32_t att, const uint32_t poll_limit) {
    __syncthreads();
    if (threadIdx.x == 0) cluster_wait(csy, CW_DONE, (GM - 1) * att, poll_limit);
    __syncthreads();
}
// member 0, all lanes: publishes attempt `att` to the other members: graph rows (CSR), decoded sequence, V, L, the threshold
__device__ __forceinline__ void cluster_publish(uint32_t* csy, const uint32_t V, const uint32_t L, const int thrT, const uint32_t att) {
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) { st_dev(csy + CW_V, V); st_dev(csy + CW_L, L); st_dev(csy + CW_THRESHOLD, (uint32_t)thrT); __threadfence(); st_dev(csy + CW_GO, att); }
}

// ---- the edge's graph: views into the pools at the offsets of its workspace slot
__device__ __forceinline__ void bind_graph(G& g, const PoaPools& P, const PoaSlot& SL, const PoaEdge& ED) {
    const uint64_t no = SL.node_off, eo = SL.edge_off;
    g.code = P.code + no; g.n_aligned = P.n_aligned + no; g.aligned = P.aligned + 3 * no;
    g.in_head = P.in_head + no; g.in_tail = P.in_tail + no; g.out_head = P.out_head + no; g.out_tail = P.out_tail + no;
    g.rank2node = P.rank2node + no; g.node2rank = P.node2rank + no; g.mark = P.mark + no; g.check = P.check + no;
    g.stack = P.stack + SL.stack_off; g.score = P.score + no; g.pred = P.pred + no;
    g.row_code = P.row_code + no; g.row_sink = P.row_sink + no; g.row_pred_off = P.row_pred_off + no; g.pred_rank = P.pred_rank + eo; g.pred_w = P.pred_w + eo;
    g.row_meta = P.row_meta + no; g.row_pred0 = P.row_pred0 + no; g.row_pred1 = P.row_pred1 + no; g.nrec = P.nrec + no; g.nrec2 = P.nrec2 + no; g.row_al = P.row_al + no; g.wslot = P.wslot + no;
    g.e_from = P.e_from + eo; g.e_to = P.e_to + eo; g.e_next_in = P.e_next_in + eo; g.e_next_out = P.e_next_out + eo; g.e_w = P.e_w + eo;
    g.aln_node = P.aln_node + SL.aln_off; g.aln_pos = P.aln_pos + SL.aln_off;
    g.vcap = ED.vcap; g.ecap = ED.ecap;
}

// ---- the words of poa_edge's lds_u[] that the traceback walk and its helper wave share (the scans of the graph phases use lds_u as scratch: between them only)
enum WalkWord : uint32_t {
    WALK_N = 0,         // result: entries of the walk proper, still in (rank, column) form ...
    WALK_I = 1,         // ... and where it stopped: rank,
    WALK_J = 2,         // column
    WALK_AT_I = 8,      // the helper's mailbox: the rank at which the walk's current tile begins,
    WALK_AT_J = 9,      // its last column,
    WALK_DONE = 10      // 1: the walk has ended
};
