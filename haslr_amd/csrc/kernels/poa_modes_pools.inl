// poa_modes_pools.inl - the graph pools of a set of the general POA path, for the kernel that carves them out of its slot (kernels/poa_modes.hip)
// and for the host plan that sizes the slots (kernels/poa_modes_plan.hip). Included inside a file's anonymous namespace, after poa_graph.inl (G).

__host__ __device__ inline uint64_t al256(uint64_t x) { return (x + 255) & ~255ull; }

// the graph pools of a set at the start of its slot: at most one node per base (vcap = total length), one edge per base and sequence.
// Returns their bytes; fills g / path / colref when base is not null. The host sizes slots with the same function.
__host__ __device__ inline uint64_t carve_pools(uint8_t* base, uint64_t T, uint32_t nseq, uint32_t lmax, G* g, uint32_t** path, uint32_t** colref) {
    const uint64_t vc = T + 1, ec = T + nseq + 1, ac = T + lmax + 2, sc = 4 * vc + ec + 64;
    uint64_t off = 0;
    auto take = [&](uint64_t bytes) -> uint8_t* { uint8_t* p = base ? base + off : nullptr; off += al256(bytes); return p; };
    G t{};
    t.code = take(vc); t.n_aligned = take(vc); t.mark = take(vc); t.check = take(vc);
    t.aligned = (uint32_t*)take(12 * vc);
    t.in_head = (uint32_t*)take(4 * vc); t.in_tail = (uint32_t*)take(4 * vc); t.out_head = (uint32_t*)take(4 * vc); t.out_tail = (uint32_t*)take(4 * vc);
    t.rank2node = (uint32_t*)take(4 * vc); t.node2rank = (uint32_t*)take(4 * vc); t.stack = (uint32_t*)take(4 * sc);
    t.score = (int32_t*)take(4 * vc); t.pred = (int32_t*)take(4 * vc);
    t.row_meta = (uint32_t*)take(4 * vc); t.row_pred_off = (uint32_t*)take(4 * vc + 4);
    t.pred_rank = (uint32_t*)take(4 * ec); t.pred_w = (int32_t*)take(4 * ec);
    t.nrec = (uint4*)take(16 * vc); t.nrec2 = (uint4*)take(16 * vc);
    t.e_from = (uint32_t*)take(4 * ec); t.e_to = (uint32_t*)take(4 * ec); t.e_next_in = (uint32_t*)take(4 * ec); t.e_next_out = (uint32_t*)take(4 * ec);
    t.e_w = (int32_t*)take(4 * ec);
    t.aln_node = (int32_t*)take(4 * ac); t.aln_pos = (int32_t*)take(4 * ac);
    uint32_t* p = (uint32_t*)take(4 * (uint64_t)(lmax + 1));
    uint32_t* c = (uint32_t*)take(4 * (uint64_t)(lmax + 1));
    t.vcap = (uint32_t)T; t.ecap = (uint32_t)(T + nseq);
    if (g) { *g = t; *path = p; *colref = c; }
    return off;
}

// The phase pool of a set (phase instances only; phase_reads, poa_modes_out.inl), behind the graph pools of its slot: words, sized from the
// set's bases T and sequences nseq alone. A set has at most T columns and at most as many sites as columns.
//   cnt    4 per column   the letter counts of the column
//   dep    1 per column   + 1: the span marks, then the depth
//   spre   1 per column   + 1: the sites in front of the column
//   base   1 per base     the column of the base, then its site, its vote and the site's gap vote, packed
//   s_col, s_al, s_sign, s_d, s_mark, s_gp   6 per site, + 1 each: the site's column, alleles, sign, the round's difference, its span marks
//          and the prefix of the gap votes
//   lo, hi 2 per sequence: first its span in columns, then in sites
//   scal   8 words: the block-wide scalars (the first two one 64-bit word)
struct PhasePool { uint32_t *cnt, *dep, *spre, *base, *s_col, *s_al; int32_t *s_sign, *s_d, *s_mark, *s_gp; uint32_t *lo, *hi, *scal; };
__host__ __device__ inline uint64_t carve_phase(uint8_t* base, uint64_t T, uint32_t nseq, PhasePool* pp) {
    const uint64_t cc = T + 1;
    uint64_t off = 0;
    auto take = [&](uint64_t words) -> uint32_t* { uint32_t* p = base ? (uint32_t*)(base + off) : nullptr; off += al256(4 * words); return p; };
    PhasePool t{};
    t.cnt = take(4 * cc); t.dep = take(cc); t.spre = take(cc); t.base = take(cc);
    t.s_col = take(cc); t.s_al = take(cc); t.s_sign = (int32_t*)take(cc); t.s_d = (int32_t*)take(cc); t.s_mark = (int32_t*)take(cc); t.s_gp = (int32_t*)take(cc);
    t.lo = take((uint64_t)nseq + 1); t.hi = take((uint64_t)nseq + 1); t.scal = take(8);
    if (pp) *pp = t;
    return off;
}
