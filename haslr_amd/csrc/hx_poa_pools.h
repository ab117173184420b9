// hx_poa_pools.h - THE list of the POA workspace pools (kernels/kernels.h PoaPools). One table gives every pool its name, its element type and
// the total it is counted in; the buffers of a context, their placement in the arena, the kernel argument and the bytes a node or a graph edge
// costs are all generated from it. Host code; no HIP runtime call.
#pragma once
#include <cstddef>
#include <cstdint>
#include <algorithm>
#include "kernels/kernels.h"

namespace hxi {

// What the pools are counted in: the sums over a batch's workspace slots (hx_poa_plan.h Need: nodes, graph edges, cells of H, direction bytes,
// wide-row bytes, decoded bases, stack entries, alignment entries), the mailbox words (slots' carries + the shared edges' cluster part), the
// consensus bytes, and the edges of the call.
struct PoaPoolTotals { uint64_t no = 0, eo = 0, ho = 0, dro = 0, wo = 0, so = 0, sto = 0, ao = 0, clo = 0, co = 0, ne = 0; };
enum class PoaPoolTotal { no, eo, ho, dro, wo, so, sto, ao, clo, co, ne };

// F(name, element type, total, factor): the pool holds factor x total elements. The order is the order in the arena. F names the members of the
// kernels' PoaPools, G the one pool that is not among them (the consensus strings: PoaLaunch::cns).
#define HX_POA_POOLS(F, G) \
    F(H, int32_t, ho, 1) F(dir, uint8_t, dro, 1) F(dirw, uint8_t, wo, 1) F(wslot, uint32_t, no, 1) F(code, uint8_t, no, 1) F(n_aligned, uint8_t, no, 1) \
    F(mark, uint8_t, no, 1) F(check, uint8_t, no, 1) F(row_code, uint8_t, no, 1) F(row_sink, uint8_t, no, 1) F(row_al, uint16_t, no, 1) F(aligned, uint32_t, no, 3) \
    F(in_head, uint32_t, no, 1) F(in_tail, uint32_t, no, 1) F(out_head, uint32_t, no, 1) F(out_tail, uint32_t, no, 1) F(rank2node, uint32_t, no, 1) \
    F(node2rank, uint32_t, no, 1) F(row_pred_off, uint32_t, no, 1) F(score, int32_t, no, 1) F(pred, int32_t, no, 1) F(pred_rank, uint32_t, eo, 1) \
    F(pred_w, int32_t, eo, 1) F(e_from, uint32_t, eo, 1) F(e_to, uint32_t, eo, 1) F(e_next_in, uint32_t, eo, 1) F(e_next_out, uint32_t, eo, 1) F(e_w, int32_t, eo, 1) \
    F(stack, uint32_t, sto, 1) F(aln_node, int32_t, ao, 1) F(aln_pos, int32_t, ao, 1) F(row_meta, uint32_t, no, 1) F(row_pred0, uint32_t, no, 1) \
    F(row_pred1, uint32_t, no, 1) F(nrec, uint4, no, 1) F(nrec2, uint4, no, 1) F(seq, uint8_t, so, 1) G(cns, char, co, 1) F(mbox, unsigned long long, clo, 1) \
    F(csync, uint32_t, ne, 8) F(sinkbuf, int32_t, ne, 1 + 2 * 1024)

// every member of the kernels' PoaPools is a pointer, and the F entries are all of them: a member added there without an entry here would stay null
constexpr size_t kPoaKernelPools = 0
#define HX_F(name, type, total, factor) + 1
#define HX_G(name, type, total, factor)
    HX_POA_POOLS(HX_F, HX_G)
#undef HX_F
#undef HX_G
    ;
static_assert(sizeof(hxk::PoaPools) == kPoaKernelPools * sizeof(void*), "HX_POA_POOLS and hxk::PoaPools (kernels/kernels.h) list different pools");

// bytes that one unit of a total costs over all the pools counted in it
constexpr uint64_t poa_pool_bytes_per(PoaPoolTotal t) {
    return 0
#define HX_F(name, type, total, factor) + (PoaPoolTotal::total == t ? (uint64_t)(factor) * sizeof(type) : 0)
        HX_POA_POOLS(HX_F, HX_F)
#undef HX_F
        ;
}

// where every pool of a batch begins in the arena (bytes, 256-byte aligned; an empty pool still gets one element)
struct PoaPoolOffsets {
#define HX_F(name, type, total, factor) size_t name = 0;
    HX_POA_POOLS(HX_F, HX_F)
#undef HX_F
    size_t place(const PoaPoolTotals& t) {   // returns the size of the arena
        size_t at = 0;
#define HX_F(name, type, total, factor) name = at; at += (std::max<uint64_t>(1, (uint64_t)(factor) * t.total) * sizeof(type) + 255) & ~(size_t)255;
        HX_POA_POOLS(HX_F, HX_F)
#undef HX_F
        return at;
    }
};

// The pools of a context: pointers into its arena (hx_internal.h PoaArena), bound anew for every batch
struct PoaPoolBufs {
#define HX_F(name, type, total, factor) type* name = nullptr;
    HX_POA_POOLS(HX_F, HX_F)
#undef HX_F
    void bind(uint8_t* arena, const PoaPoolOffsets& off) {
#define HX_F(name, type, total, factor) name = reinterpret_cast<type*>(arena + off.name);
        HX_POA_POOLS(HX_F, HX_F)
#undef HX_F
    }
    hxk::PoaPools view() const {   // the kernel argument, member by member
        hxk::PoaPools v{};
#define HX_F(name, type, total, factor) v.name = name;
#define HX_G(name, type, total, factor)
        HX_POA_POOLS(HX_F, HX_G)
#undef HX_F
#undef HX_G
        return v;
    }
};

}  // namespace hxi
