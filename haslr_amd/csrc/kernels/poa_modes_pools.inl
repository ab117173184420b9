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
