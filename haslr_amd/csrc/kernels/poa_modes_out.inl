// poa_modes_out.inl - what the general POA path (kernels/poa_modes.hip) writes beside the consensus text: the columns of the multiple sequence
// alignment and its row text, the base weights on the graph's edges, the coverage of the consensus bases, the graph and the alignments
// themselves, the per-label views of a set's graph with their consensus, and the phasing of a set's reads into two haplotypes. Included inside that file's anonymous namespace, after MRow, GraphOutArgs and block_excl_sum.

// ---- MSA output (DESIGN.md "General POA path", "MSA output") ----
// The columns of spoa's generate_multiple_sequence_alignment on the final rank order (order_rows leaves aligned nodes contiguous): rank r
// opens a column iff none of its node's aligned nodes has a smaller rank, and the column of a rank is the number of openers up to it, less
// one. colr (by rank) receives them; returns the number of columns. All lanes.
template <int NT>
__device__ uint32_t msa_columns(const G& g, const uint32_t V, uint32_t* colr, uint32_t* s_scan) {
    const uint32_t t = threadIdx.x;
    uint32_t carry = 0;
    for (uint32_t b = 0; b < V; b += NT) {
        const uint32_t r = b + t;
        uint32_t opens = 0;
        if (r < V) {
            const uint32_t n = g.rank2node[r], na = g.n_aligned[n];
            opens = 1;
            for (uint32_t k = 0; k < na; k++) if (g.node2rank[g.aligned[3 * n + k]] < r) opens = 0;
        }
        uint32_t tot;
        const uint32_t pre = block_excl_sum<NT>(opens, s_scan, &tot);
        if (r < V) colr[r] = carry + pre + opens - 1u;   // (rank 0 always opens: never below 0)
        carry += tot;
    }
    __syncthreads();
    return carry;
}

// consensus_wave of poa_graph.inl that also hands back the rank the walk back starts from: the ranks of the consensus nodes are that rank and
// its chain of g.pred. A copy: with consensus_wave as a wrapper over this one, k_poa's objects no longer come out byte for byte as before.
__device__ uint32_t consensus_wave_end(G& g, const uint32_t V, char* out, uint32_t* end_rank) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t best, nbest;
    bundle_pass(g, V, 0, false, -1, best, nbest);
    if (best == NONE) best = g.node2rank[0];
    for (uint32_t round = 0; !(g.row_meta[best] & 4u) && round <= V; round++) {
        const uint32_t n0 = g.rank2node[best];
        if (lane == 0)
            for (uint32_t e = g.out_head[n0]; e != NONE; e = g.e_next_out[e])
                for (uint32_t oe = g.in_head[g.e_to[e]]; oe != NONE; oe = g.e_next_in[oe])
                    if (g.e_from[oe] != n0) g.score[g.node2rank[g.e_from[oe]]] = -1;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        uint32_t nb;
        bundle_pass(g, V, best + 1, true, 0, nb, nbest);
        best = nb == NONE ? g.node2rank[0] : nb;
    }
    *end_rank = best;
    return bundle_backtrack(g, best, out);
}

// the columns of the len consensus bases, by the first wavefront: bundle_backtrack's walk (64 ranks around the walk fetched at once, the
// walk inside them on v_readlane) with the rank's column in place of its base; back to front in rev, then turned round by all lanes
__device__ void consensus_columns(const G& g, const uint32_t end_rank, const uint32_t len, const uint32_t* colr, uint32_t* rev, uint32_t* out) {
    const uint32_t lane = threadIdx.x & 63u;
    const int32_t* pr_r = g.pred;
    int32_t r = __builtin_amdgcn_readfirstlane((int)end_rank);
    uint32_t k = 0;
    int acc = 0;
    while (r != -1 && k < len) {
        const uint32_t cb = (uint32_t)r & ~63u, idx = min(cb + lane, (uint32_t)r);
        const int p = pr_r[idx], c = (int)colr[idx];
        while (r >= (int32_t)cb && k < len) {
            const int l = r - (int32_t)cb;
            const int cl = __builtin_amdgcn_readlane(c, l);
            acc = lane == (k & 63u) ? cl : acc;
            k++;
            if ((k & 63u) == 0) rev[k - 64 + lane] = (uint32_t)acc;
            r = __builtin_amdgcn_readlane(p, l);
        }
    }
    if (lane < (k & 63u)) rev[(k & ~63u) + lane] = (uint32_t)acc;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    for (uint32_t q = lane; q < k; q += 64) out[q] = rev[k - 1 - q];
}

// The row text of one call, grid-wide: a wavefront takes 64 consecutive bases of one row. Columns rise strictly along a row, so lane i
// writes the gaps between the previous base's column and its own, then its base: one nearly contiguous span per wavefront, every byte of
// the output written exactly once (no fill pass). The gaps before a row's first base and after its last one can be long: the whole
// wavefront writes those. A row without bases (an empty sequence) is one chunk that writes ncols gaps.
__global__ __launch_bounds__(256) void k_msa_rows(const MRow* rows, const uint2* chunks, const uint32_t n_chunks, const uint32_t* base_col, const uint8_t* codes,
                                                  const uint32_t* cns_col, const char* cns, char* out) {
    const uint32_t w = (blockIdx.x * 256u + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (w >= n_chunks) return;
    const uint2 ch = chunks[w];
    const MRow R = rows[ch.x];
    const uint32_t* col = (R.is_cns ? cns_col : base_col) + R.src;
    char* row = out + R.dst;
    const uint32_t i = ch.y + lane;
    if (i < R.len) {
        const uint32_t c = col[i];
        const uint32_t from = i ? col[i - 1] + 1u : c;   // (the gaps before the first base: below, by all lanes)
        if (c < R.ncols && from <= c) {                   // (always true for the columns run_set leaves: the guard keeps a store inside the row)
            for (uint32_t q = from; q < c; q++) row[q] = '-';
            row[c] = R.is_cns ? cns[R.src + i] : "ACGT"[codes[R.src + i] & 3];
        }
    }
    if (ch.y == 0 && R.len) { const uint32_t c0 = min(col[0], R.ncols); for (uint32_t q = lane; q < c0; q += 64) row[q] = '-'; }
    if (ch.y + 64 >= R.len) {
        const uint32_t after = R.len ? col[R.len - 1] + 1u : 0u;
        for (uint32_t q = after + lane; q < R.ncols; q += 64) row[q] = '-';
    }
}

// ---- base weights and coverage (DESIGN.md "General POA path", "Base weights and coverage") ----
// spoa's weighted add_alignment, applied beside the unit-weight one: the sequence walks the edge path[i-1] -> path[i] for every pair of
// consecutive bases (prefix chain, aligned part, suffix chain alike) and add_alignment has given each of them 2; what is missing to spoa's
// w[i-1] + w[i] is added here, by all lanes. The nodes of one sequence are distinct (its columns rise strictly), so no two lanes meet on an
// edge. The edge is looked up in the out-list of path[i-1], as add_edge does.
template <int NT>
__device__ void weigh_path(G& g, const uint32_t* path, const uint8_t* w, const uint32_t L) {
    for (uint32_t i = threadIdx.x + 1; i < L; i += NT) {
        const int32_t extra = (int32_t)w[i - 1] + (int32_t)w[i] - 2;
        if (extra == 0) continue;
        const uint32_t to = path[i];
        for (uint32_t e = g.out_head[path[i - 1]]; e != NONE; e = g.e_next_out[e])
            if (g.e_to[e] == to) { g.e_w[e] += extra; break; }
    }
}

// ---- strand-ambiguous sets (DESIGN.md "General POA path", "Strand-ambiguous sets") ----
// all lanes, once the orientation of the sequence at base offset b (sequence `seq` of the call) is chosen: its codes and weights as they
// are added go to codes_used / wts_used, the choice and the two end-cell scores to the per-sequence arrays. The barrier at its end lets
// thread 0 (traceback, add_alignment) and weigh_path read what all lanes wrote.
template <int NT>
__device__ void keep_strand(const MArgs& a, const uint64_t b, const uint32_t L, const uint64_t seq, const bool rev, const int32_t score_f, const int32_t score_r) {
    const uint8_t *c = (rev ? a.sa.codes_rc : a.codes) + b, *w = (rev ? a.sa.wts_rc : a.wts) + b;
    for (uint32_t i = threadIdx.x; i < L; i += NT) { a.sa.codes_used[b + i] = c[i]; a.sa.wts_used[b + i] = w[i]; }
    if (threadIdx.x == 0) { a.sa.reversed[seq] = rev ? 1 : 0; a.sa.score_fwd[seq] = score_f; a.sa.score_rev[seq] = score_r; }
    __syncthreads();
}

// one sequence of >= 2 bases (k_cov_hist: src = its first base, hoff = the first column of its set among all columns of the call) or one
// consensus (k_cov_gather: src = its place beside the device's consensus text, dst = its place in the output)
struct CRow { uint64_t src, dst, hoff; uint32_t len, ncols; };

// The number of bases per column (stride 1) or per column and letter (stride 4) of one call, grid-wide: a wavefront takes 64 consecutive
// bases of one sequence. Columns rise strictly along a sequence, so the lanes of a wavefront never meet on a counter; different sequences
// of a set do, hence the atomic.
__global__ __launch_bounds__(256) void k_cov_hist(const CRow* rows, const uint2* chunks, const uint32_t n_chunks, const uint32_t* base_col, const uint8_t* codes,
                                                  const uint32_t stride, uint32_t* hist) {
    const uint32_t w = (blockIdx.x * 256u + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (w >= n_chunks) return;
    const uint2 ch = chunks[w];
    const CRow R = rows[ch.x];
    const uint32_t i = ch.y + lane;
    if (i >= R.len) return;
    const uint32_t c = base_col[R.src + i];
    if (c >= R.ncols) return;   // (never true for the columns run_set leaves: the guard keeps the add inside the set's counters)
    atomicAdd(&hist[(R.hoff + c) * stride + (stride == 4 ? (uint32_t)(codes[R.src + i] & 3) : 0u)], 1u);
}

// coverage (and the four letter counts) of every consensus base: the counters of its column. A wavefront takes 64 consecutive bases of
// one consensus; cov / prof are in the output's layout (consensus strings back to back).
__global__ __launch_bounds__(256) void k_cov_gather(const CRow* rows, const uint2* chunks, const uint32_t n_chunks, const uint32_t* cns_col, const uint32_t* hist,
                                                    const uint32_t stride, uint32_t* cov, uint32_t* prof) {
    const uint32_t w = (blockIdx.x * 256u + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (w >= n_chunks) return;
    const uint2 ch = chunks[w];
    const CRow R = rows[ch.x];
    const uint32_t i = ch.y + lane;
    if (i >= R.len) return;
    const uint32_t c = cns_col[R.src + i];
    uint32_t n[4] = {0, 0, 0, 0};
    if (c < R.ncols) {
        const uint32_t* h = hist + (R.hoff + c) * stride;
        n[0] = h[0];
        if (stride == 4) { n[1] = h[1]; n[2] = h[2]; n[3] = h[3]; }
    }
    cov[R.dst + i] = n[0] + n[1] + n[2] + n[3];
    if (prof) { uint32_t* p = prof + 4 * (R.dst + i); p[0] = n[0]; p[1] = n[1]; p[2] = n[2]; p[3] = n[3]; }
}

// ---- graph and alignment output (DESIGN.md "General POA path", "Graph and alignment output") ----
// The traceback reports 0 pairs for an alignment that holds no sequence position (add_alignment then adds the sequence as a chain), but the
// output keeps such an alignment as the walk produced it. Such a walk only ever steps up a row, so it leaves at most V pairs, each with
// position -1: with the first V + 1 positions set to -2 beforehand, the first -2 left tells where it ended. All lanes, before dp_rows.
constexpr int32_t ALN_UNSET = -2;
template <int NT>
__device__ void mark_pairs(G& g, const uint32_t V) {
    for (uint32_t i = threadIdx.x; i <= V; i += NT) g.aln_pos[i] = ALN_UNSET;
}

// thread 0, after the traceback returned na: stores the end cell's score and returns the pairs the walk left in aln_node / aln_pos
__device__ uint32_t keep_score(const G& g, const uint32_t V, uint32_t na, const int32_t score, int32_t* out) {
    *out = score;
    if (na == 0) while (na <= V && g.aln_pos[na] != ALN_UNSET) na++;
    return na;
}

// all lanes, after add_alignment's barrier: the na pairs of sequence `seq` (of the call) go to the set's share of the pool from `used` on,
// as far as they fit. Returns na.
template <int NT>
__device__ uint32_t keep_pairs(const G& g, const uint32_t na, const GraphOutArgs& o, const uint32_t set, const uint64_t seq, const uint64_t used) {
    const uint64_t at = o.aln_at[set], room = o.aln_room[set];
    for (uint32_t i = threadIdx.x; i < na; i += NT)
        if (used + i < room) { o.aln_node[at + used + i] = g.aln_node[i]; o.aln_pos[at + used + i] = g.aln_pos[i]; }
    if (threadIdx.x == 0) o.aln_cnt[seq] = na;
    return na;
}

// all lanes, after the last sort and msa_columns: the set's nodes (code, rank, column) from nb on, its edges in creation order from eb on
template <int NT>
__device__ void keep_graph(const G& g, const uint32_t V, const uint32_t E, const uint32_t* colr, const GraphOutArgs& o, const uint32_t set, const uint64_t nb, const uint64_t eb) {
    const uint32_t t = threadIdx.x;
    for (uint32_t n = t; n < V; n += NT) { const uint32_t r = g.node2rank[n]; o.node_code[nb + n] = g.code[n]; o.node_rank[nb + n] = r; o.node_col[nb + n] = colr[r]; }
    for (uint32_t e = t; e < E; e += NT) { o.edge_from[eb + e] = g.e_from[e]; o.edge_to[eb + e] = g.e_to[e]; o.edge_w[eb + e] = g.e_w[e]; }
    if (t == 0) { o.n_nodes[set] = V; o.n_edges[set] = E; }
}

// one run of elements that k_graph_gather moves from where run_set left them (src) to its place in the dense output (dst): the nodes of a
// set, its edges, the nodes of its consensus, or the pairs of one alignment (pa / pb: the pool's two arrays; read back to front)
enum { GR_NODES = 0, GR_EDGES = 1, GR_CNS = 2, GR_ALN = 3 };
struct GRow { const int32_t *pa, *pb; uint64_t src, dst; uint32_t len, kind; };
struct GatherArgs {
    const uint8_t* node_code; const uint32_t *node_rank, *node_col, *edge_from, *edge_to; const int32_t* edge_w; const uint32_t* cns_node;
    char* o_base; uint32_t *o_rank, *o_col, *o_from, *o_to; int32_t* o_w; uint32_t* o_cns_node; int32_t *o_aln_node, *o_aln_pos;
};

// The dense output of one call, grid-wide: a wavefront takes 64 consecutive elements of one run; reads and writes are contiguous (an
// alignment's are read in falling, written in rising order). Codes become letters here.
__global__ __launch_bounds__(256) void k_graph_gather(const GRow* rows, const uint2* chunks, const uint32_t n_chunks, const GatherArgs a) {
    const uint32_t w = (blockIdx.x * 256u + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (w >= n_chunks) return;
    const uint2 ch = chunks[w];
    const GRow R = rows[ch.x];
    const uint32_t i = ch.y + lane;
    if (i >= R.len) return;
    const uint64_t s = R.src + i, d = R.dst + i;
    if (R.kind == GR_NODES) { a.o_base[d] = "ACGT"[a.node_code[s] & 3]; a.o_rank[d] = a.node_rank[s]; a.o_col[d] = a.node_col[s]; }
    else if (R.kind == GR_EDGES) { a.o_from[d] = a.edge_from[s]; a.o_to[d] = a.edge_to[s]; a.o_w[d] = a.edge_w[s]; }
    else if (R.kind == GR_CNS) a.o_cns_node[d] = a.cns_node[s];
    else { const uint64_t b = R.src + (R.len - 1u - i); a.o_aln_node[d] = R.pa[b]; a.o_aln_pos[d] = R.pb[b]; }
}

// ---- per-label consensus (DESIGN.md "General POA path", "Per-label consensus") ----
// The rank-ordered rows of a label's view: the second half of order_rows with the edges no sequence of the label walks (weight 0 in vw)
// left out, the weights the view's, and the sink bit set where the node has no out-edge in the view. All lanes.
template <int NT>
__device__ void view_rows(G& g, const uint32_t V, const int32_t* vw, uint32_t* s_scan) {
    const uint32_t t = threadIdx.x;
    uint32_t carry = 0;
    for (uint32_t b = 0; b < V; b += NT) {
        const uint32_t r = b + t;
        uint32_t np = 0;
        if (r < V) {
            const uint32_t n = g.rank2node[r];
            for (uint32_t e = g.in_head[n]; e != NONE; e = g.e_next_in[e]) np += vw[e] != 0;
            bool sink = true;
            for (uint32_t e = g.out_head[n]; e != NONE && sink; e = g.e_next_out[e]) sink = vw[e] == 0;
            g.row_meta[r] = (uint32_t)g.code[n] | (sink ? 4u : 0u) | (np << META_NP);
        }
        uint32_t tot;
        const uint32_t pre = block_excl_sum<NT>(np, s_scan, &tot);
        if (r < V) {
            uint32_t o = carry + pre;
            g.row_pred_off[r] = o;
            for (uint32_t e = g.in_head[g.rank2node[r]]; e != NONE; e = g.e_next_in[e])
                if (vw[e] != 0) { g.pred_rank[o] = g.node2rank[g.e_from[e]]; g.pred_w[o] = vw[e]; o++; }
        }
        carry += tot;
    }
    if (t == 0) g.row_pred_off[V] = carry;
    __syncthreads();
}

// consensus_wave_end on a view: the rows are view_rows', the branch completion kills through the view's edges only, and where spoa falls
// back to node 0 the view falls back to its own node of smallest id (low_rank: its rank). The first wavefront.
__device__ uint32_t consensus_wave_view(G& g, const uint32_t V, const int32_t* vw, const uint32_t low_rank, char* out, uint32_t* end_rank) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t best, nbest;
    bundle_pass(g, V, 0, false, -1, best, nbest);
    if (best == NONE) best = low_rank;
    for (uint32_t round = 0; !(g.row_meta[best] & 4u) && round <= V; round++) {
        const uint32_t n0 = g.rank2node[best];
        if (lane == 0)
            for (uint32_t e = g.out_head[n0]; e != NONE; e = g.e_next_out[e]) {
                if (vw[e] == 0) continue;
                for (uint32_t oe = g.in_head[g.e_to[e]]; oe != NONE; oe = g.e_next_in[oe])
                    if (vw[oe] != 0 && g.e_from[oe] != n0) g.score[g.node2rank[g.e_from[oe]]] = -1;
            }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        uint32_t nb;
        bundle_pass(g, V, best + 1, true, 0, nb, nbest);
        best = nb == NONE ? low_rank : nb;
    }
    *end_rank = best;
    return bundle_backtrack(g, best, out);
}

// All lanes, after the last sort and msa_columns, while base_col still holds the node of every base: one consensus per label over the
// set's graph. Per label with members: the weight of every edge in its view (vw; cleared, then every base pair of the label's sequences
// adds w[i-1] + w[i] to the edge between its two nodes - looked up in the out-list of the first, as weigh_path does; two sequences of a
// label may share an edge, hence the atomic), the view's rows, the heaviest bundle on them and the columns of its bases. vw lies in the
// node records' pool, which nothing reads after the last add and which holds four words per node (a set has no more edges than bases);
// e_w itself stays as it is. A label without a non-empty sequence in the set keeps the length 0 its place was cleared to.
template <int NT>
__device__ void label_views(G& g, const MArgs& a, const MSet& S, const uint32_t set, const uint32_t V, const uint32_t E, const uint32_t* colr, Shared& sh, uint32_t* s_scan) {
    const uint32_t t = threadIdx.x;
    int32_t* vw = (int32_t*)g.nrec;
    for (uint32_t lb = 0; lb < a.n_labels; lb++) {
        for (uint32_t e = t; e < E; e += NT) vw[e] = 0;
        if (t == 0) sh.na = NONE;
        __syncthreads();
        uint32_t low = NONE;
        for (uint32_t k = 0; k < S.nseq; k++) {
            if (a.labels[S.seq_begin + k] != lb) continue;
            const uint64_t b = a.soff[S.seq_begin + k];
            const uint32_t L = (uint32_t)(a.soff[S.seq_begin + k + 1] - b);
            const uint32_t* path = a.base_col + b;
            const uint8_t* w = a.wts + b;
            for (uint32_t i = t; i < L; i += NT) {
                const uint32_t to = path[i];
                low = min(low, to);
                if (i == 0) continue;
                for (uint32_t e = g.out_head[path[i - 1]]; e != NONE; e = g.e_next_out[e])
                    if (g.e_to[e] == to) { if (e < E) atomicAdd(&vw[e], (int32_t)w[i - 1] + (int32_t)w[i]); break; }   // (e < E always: the guard keeps the add inside the array)
            }
        }
        if (low != NONE) atomicMin(&sh.na, low);
        __syncthreads();
        const uint32_t lowest = sh.na;   // (the same value in every lane)
        if (lowest < V) {
            view_rows<NT>(g, V, vw, s_scan);
            if (t < 64) {
                const uint64_t at = S.cns_off + (uint64_t)lb * S.sum_len;
                uint32_t end_rank = 0;
                const uint32_t len = consensus_wave_view(g, V, vw, g.node2rank[lowest], a.cns + at, &end_rank);
                consensus_columns(g, end_rank, len, colr, (uint32_t*)g.aln_pos, a.cns_col + at);
                if (t == 0) a.cns_len[(uint64_t)set * a.n_labels + lb] = len;
            }
        }
        __syncthreads();   // the next label rewrites vw, the rows and the smallest id
    }
}

// ---- two-haplotype consensus (DESIGN.md "General POA path", "Two-haplotype consensus") ----
constexpr uint32_t PHASE_ROUNDS = 8, HAP_NONE = 255;

__device__ __forceinline__ int wave_sum(int v) {
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// All lanes, after the last sort and msa_columns, while base_col still holds the node of every base, and in front of label_views: the
// haplotype of every sequence of the set (a.ph.hap: 0, 1, or 255 for none), the set's sites, rounds and verdict. The rules are DESIGN.md's,
// held to tests/poa_phase_ref.cpp; the work is laid out so that nothing is sequences x columns:
//   counts   one lane per base adds to its column's letter count; a sequence marks + 1 at its first column and - 1 behind its last, a block
//            scan of the marks is the depth, and the gaps of a column are its depth less its letters
//   sites    one lane per column tests the rule; a second block scan in the same pass numbers the sites; the seed is a 64-bit atomic
//            maximum over (minor count, sites counted from the back)
//   a base   then keeps one word: its site, its vote there (a1 + 1, a2 - 1, else 0) and the site's gap vote (a1 is the gap + 1, a2 - 1),
//            packed as site << 4 | (vote + 1) << 2 | (gap vote + 1); NONE: the base stands in no site
//   a round  with z = + 1 / - 1 / 0 for a sequence of haplotype 0 / 1 / none, a site's difference is the sum over the sequences that span
//            it of z x (their vote, or the gap vote where they have no base): every base at a site adds z x (vote - gap vote), the span of
//            every sequence marks + z / - z over the sites, and the scan of the marks times the gap vote is the rest. The sum of a sequence
//            is the same the other way round: its bases add sign x (vote - gap vote), and the prefix of sign x gap vote over its sites is
//            the rest. One wavefront per sequence, no barrier inside; the round's barriers stand in block-uniform code (the number of
//            sites and the changed flag are the same value in every lane)
// The pool: carve_phase (poa_modes_pools.inl); the few block-wide scalars (the seed's key, the changed flag, the members of the two
// haplotypes, the first assigned sequence) are words of it, reached by atomics.
template <int NT>
__device__ void phase_reads(const G& g, const MArgs& a, const MSet& S, const uint32_t set, const uint32_t C, const uint32_t* colr, const PhasePool& P, uint32_t* s_scan) {
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    constexpr uint32_t NW = NT / 64;
    const uint32_t n = S.nseq, T = (uint32_t)S.sum_len;
    const uint64_t* soff = a.soff + S.seq_begin;
    const uint64_t b0 = soff[0];
    const uint32_t* node = a.base_col + b0;
    const uint8_t* code = a.codes + b0;
    uint8_t* hap = a.ph.hap + S.seq_begin;
    // ---- the letter counts and the span marks (no run-time loop of this function is unrolled: twelve instances carry its code, and none of the loops is hot)
#pragma unroll 1
    for (uint32_t i = t; i < 4 * C; i += NT) P.cnt[i] = 0;
#pragma unroll 1
    for (uint32_t i = t; i <= C; i += NT) P.dep[i] = 0;
    unsigned long long* key = (unsigned long long*)P.scal;
    uint32_t *changed_at = P.scal + 2, *members = P.scal + 3, *first_at = P.scal + 5;
    if (t == 0) *key = 0;
    __syncthreads();
#pragma unroll 1
    for (uint32_t i = t; i < T; i += NT) {
        const uint32_t c = colr[g.node2rank[node[i]]];
        P.base[i] = c;
        if (c < C) atomicAdd(&P.cnt[4 * c + code[i]], 1u);   // (c < C always: the guard keeps the add inside the array)
    }
#pragma unroll 1
    for (uint32_t k = t; k < n; k += NT) {
        const uint32_t b = (uint32_t)(soff[k] - b0), L = (uint32_t)(soff[k + 1] - soff[k]);
        if (!L) continue;
        const uint32_t f = min(colr[g.node2rank[node[b]]], C - 1), l = min(colr[g.node2rank[node[b + L - 1]]], C - 1);   // (both below C always)
        P.lo[k] = f; P.hi[k] = l;
        atomicAdd(&P.dep[f], 1u);
        atomicAdd(&P.dep[l + 1], 0xffffffffu);
    }
    __syncthreads();
    // ---- depth, the site rule, the sites numbered in column order, the seed
    uint32_t carry_d = 0, Sn = 0;
#pragma unroll 1
    for (uint32_t cb = 0; cb < C; cb += NT) {
        const uint32_t c = cb + t, mark = c < C ? P.dep[c] : 0u;
        uint32_t tot;
        const uint32_t d = carry_d + block_excl_sum<NT>(mark, s_scan, &tot) + mark;
        carry_d += tot;
        uint32_t site = 0, al = 0, n2 = 0;
        if (c < C) {
            uint32_t cn[5];
            cn[4] = d;
#pragma unroll
            for (uint32_t q = 0; q < 4; q++) { cn[q] = P.cnt[4 * c + q]; cn[4] -= cn[q]; }
            uint32_t a1 = 0, n1 = cn[0], a2 = 5;   // by count, falling, then by code, rising
#pragma unroll
            for (uint32_t q = 1; q < 5; q++) if (cn[q] > n1) { n1 = cn[q]; a1 = q; }
#pragma unroll
            for (uint32_t q = 0; q < 5; q++) if (q != a1 && (a2 == 5 || cn[q] > n2)) { n2 = cn[q]; a2 = q; }
            site = n2 >= max(a.ph.min_count, (a.ph.min_pct * d + 99u) / 100u);
            al = a1 | a2 << 4;
        }
        const uint32_t j = Sn + block_excl_sum<NT>(site, s_scan, &tot);
        Sn += tot;
        if (c < C) {
            P.spre[c] = j;
            if (site) { P.s_col[j] = c; P.s_al[j] = al; atomicMax(key, (unsigned long long)n2 << 32 | (0xffffffffu - j)); }
        }
    }
    if (t == 0) P.spre[C] = Sn;
    __syncthreads();
    // ---- every base's word, every sequence's span in sites
#pragma unroll 1
    for (uint32_t i = t; i < T; i += NT) {
        const uint32_t c = min(P.base[i], C - 1), j = P.spre[c];
        uint32_t word = NONE;
        if (P.spre[c + 1] != j) {
            const uint32_t al = P.s_al[j], a1 = al & 15u, a2 = al >> 4, x = code[i];
            word = j << 4 | (x == a1 ? 2u : x == a2 ? 0u : 1u) << 2 | (a1 == 4 ? 2u : a2 == 4 ? 0u : 1u);
        }
        P.base[i] = word;
    }
#pragma unroll 1
    for (uint32_t k = t; k < n; k += NT) {
        if (soff[k + 1] == soff[k]) continue;
        const uint32_t f = P.lo[k], l = P.hi[k];
        P.lo[k] = P.spre[f]; P.hi[k] = P.spre[l + 1];
    }
    __syncthreads();
    // ---- the seed's haplotypes: one wavefront per sequence (every condition on k alone is the same in its 64 lanes)
    const uint32_t jstar = 0xffffffffu - (uint32_t)*key;
    const uint32_t al_star = Sn ? P.s_al[jstar] : 0u;
#pragma unroll 1
    for (uint32_t k = w; k < n; k += NW) {
        const uint32_t b = (uint32_t)(soff[k] - b0), L = (uint32_t)(soff[k + 1] - soff[k]);
        uint32_t h = HAP_NONE;
        if (Sn && L && P.lo[k] <= jstar && jstar < P.hi[k]) {
            uint32_t vote = 3;
#pragma unroll 1
            for (uint32_t i = lane; i < L; i += 64) { const uint32_t word = P.base[b + i]; if (word != NONE && word >> 4 == jstar) vote = word >> 2 & 3u; }
            const unsigned long long has = __ballot(vote != 3);   // (at most one base of a sequence stands in a column)
            vote = has ? (uint32_t)__shfl((int)vote, __builtin_ctzll(has)) : ((al_star & 15u) == 4 ? 2u : (al_star >> 4) == 4 ? 0u : 1u);
            h = vote == 2 ? 0u : vote == 0 ? 1u : HAP_NONE;
        }
        if (lane == 0) hap[k] = (uint8_t)h;
    }
    __syncthreads();
    // ---- the rounds
    uint32_t rounds = 0;
#pragma unroll 1
    while (Sn && rounds < PHASE_ROUNDS) {
#pragma unroll 1
        for (uint32_t j = t; j <= Sn; j += NT) { P.s_d[j] = 0; P.s_mark[j] = 0; }
        if (t == 0) *changed_at = 0;
        __syncthreads();
#pragma unroll 1
        for (uint32_t k = w; k < n; k += NW) {
            const uint32_t b = (uint32_t)(soff[k] - b0), L = (uint32_t)(soff[k + 1] - soff[k]), h = hap[k];
            if (!L || h == HAP_NONE) continue;
            const int z = h ? -1 : 1;
            if (lane == 0 && P.lo[k] < P.hi[k]) { atomicAdd(&P.s_mark[P.lo[k]], z); atomicAdd(&P.s_mark[P.hi[k]], -z); }
#pragma unroll 1
            for (uint32_t i = lane; i < L; i += 64) {
                const uint32_t word = P.base[b + i];
                if (word == NONE) continue;
                const int v = (int)(word >> 2 & 3u) - (int)(word & 3u);
                if (v && (word >> 4) < Sn) atomicAdd(&P.s_d[word >> 4], z * v);   // (below Sn always)
            }
        }
        __syncthreads();
        int carry_z = 0, carry_g = 0;
#pragma unroll 1
        for (uint32_t jb = 0; jb < Sn; jb += NT) {
            const uint32_t j = jb + t, mark = j < Sn ? (uint32_t)P.s_mark[j] : 0u;
            uint32_t tot;
            const int zs = carry_z + (int)(block_excl_sum<NT>(mark, s_scan, &tot) + mark);   // z over the sequences that span site j
            carry_z += (int)tot;
            int gv = 0, sg = 0;
            if (j < Sn) {
                const uint32_t al = P.s_al[j];
                gv = (al & 15u) == 4 ? 1 : (al >> 4) == 4 ? -1 : 0;
                const int D = P.s_d[j] + gv * zs;
                sg = D > 0 ? 1 : D < 0 ? -1 : 0;
                P.s_sign[j] = sg;
            }
            const int gp = carry_g + (int)block_excl_sum<NT>((uint32_t)(sg * gv), s_scan, &tot);
            carry_g += (int)tot;
            if (j < Sn) P.s_gp[j] = gp;
        }
        if (t == 0) P.s_gp[Sn] = carry_g;
        __syncthreads();
#pragma unroll 1
        for (uint32_t k = w; k < n; k += NW) {
            const uint32_t b = (uint32_t)(soff[k] - b0), L = (uint32_t)(soff[k + 1] - soff[k]);
            if (!L) continue;
            int sum = 0;
#pragma unroll 1
            for (uint32_t i = lane; i < L; i += 64) {
                const uint32_t word = P.base[b + i];
                if (word != NONE) sum += P.s_sign[word >> 4] * ((int)(word >> 2 & 3u) - (int)(word & 3u));
            }
            sum = wave_sum(sum) + P.s_gp[P.hi[k]] - P.s_gp[P.lo[k]];
            const uint32_t h = hap[k], nh = sum > 0 ? 0u : sum < 0 ? 1u : h;
            if (lane == 0 && nh != h) { hap[k] = (uint8_t)nh; *changed_at = 1; }
        }
        __syncthreads();
        rounds++;
        const uint32_t changed = *changed_at;
        __syncthreads();   // (the next round clears the flag)
        if (!changed) break;
    }
    // ---- the verdict, the renaming, the set's outputs
    if (t == 0) { members[0] = 0; members[1] = 0; *first_at = NONE; }
    __syncthreads();
#pragma unroll 1
    for (uint32_t k = t; k < n; k += NT) {
        if (soff[k + 1] == soff[k]) continue;
        const uint32_t h = hap[k];
        if (h == HAP_NONE) continue;
        atomicAdd(&members[h], 1u);
        atomicMin(first_at, k);
    }
    __syncthreads();
    const bool phased = Sn && members[0] >= a.ph.min_count && members[1] >= a.ph.min_count;
    const bool flip = phased && hap[min(*first_at, n - 1)] == 1;   // (phased: both haplotypes have members, *first_at is the first of them)
    __syncthreads();   // every lane has read that sequence's haplotype before any is renamed
#pragma unroll 1
    for (uint32_t k = t; k < n; k += NT) {
        const uint32_t h = hap[k];
        hap[k] = (uint8_t)(soff[k + 1] == soff[k] ? HAP_NONE : !phased ? 0u : h == HAP_NONE ? HAP_NONE : h ^ (uint32_t)flip);
    }
#pragma unroll 1
    for (uint32_t j = t; j < Sn; j += NT) {   // (a set has no more sites than bases: its sites start at its first base's offset)
        const int sg = !phased ? 0 : flip ? -P.s_sign[j] : P.s_sign[j];
        a.ph.site_col[b0 + j] = P.s_col[j];
        a.ph.site_inf[b0 + j] = P.s_al[j] | (uint32_t)(sg + 1) << 8;
    }
    if (t == 0) { a.ph.n_haps[set] = phased ? 2u : 1u; a.ph.rounds[set] = rounds; a.ph.n_sites[set] = Sn; }
    __syncthreads();   // label_views reads the haplotypes as labels
}
