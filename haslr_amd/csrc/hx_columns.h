// hx_columns.h - THE lists of the structure-of-arrays columns of the chain, edge-support and coordinate operators (hx_api.hip, K1-K5). One table per family
// gives every column its element type, its name in the kernels' struct (kernels/common.h, kernels/kernels.h), its field in the public struct
// (include/haslr_types.h) and the count it is sized by; the buffers of a context, the kernel arguments, the downloads and hx_free_* are generated from them
// (hx_internal.h, hx_api.hip), member by member and by name: no list relies on the order of a struct. Host code.
#pragma once
#include <cstddef>
#include <cstdint>
#include "../../include/haslr_types.h"
#include "kernels/kernels.h"

// F(element type, member of the kernels' struct, field of the public struct, count). The counts are names of the code that uses a list.
// Resident raw hits: DevHits / hx_hits, n records and n_ops CIGAR words.
#define HX_HIT_COLUMNS(F) F(uint32_t, q_id, q_id, n) F(uint32_t, q_start, q_start, n) F(uint32_t, q_end, q_end, n) F(uint32_t, t_id, t_id, n) F(uint32_t, t_len, t_len, n) \
    F(uint32_t, t_start, t_start, n) F(uint32_t, t_end, t_end, n) F(uint32_t, n_match, n_match, n) F(uint32_t, n_block, n_block, n) F(uint8_t, is_rev, is_rev, n) \
    F(uint8_t, mapq, mapq, n) F(uint64_t, cg_off, cg_off, n + 1) F(uint32_t, cg_ops, cg_ops, n_ops)
// Per alignment: hxk::ChainScratch (at raw-hit size) and hxk::ChainFinal (n_aln) name them alike / hx_chain_out. What is not per alignment stays a
// plain member beside them: dp, from, cmp, n_aln, n_cmp of the scratch, cmp_aln of the result, the two offset arrays.
#define HX_CHAIN_COLUMNS(F) F(uint32_t, hit, hit, n_aln) F(uint32_t, qs, q_start, n_aln) F(uint32_t, qe, q_end, n_aln) F(uint32_t, ts, t_start, n_aln) F(uint32_t, te, t_end, n_aln) \
    F(uint32_t, nm, n_match, n_aln) F(uint32_t, nb, n_block, n_aln) F(uint32_t, skf, cg_skip_front, n_aln) F(uint32_t, skb, cg_skip_back, n_aln) \
    F(uint64_t, cb, cg_begin, n_aln) F(uint64_t, ce, cg_end, n_aln)
// One side of an edge-support record: DevSide / hx_rec_side. The record itself: hxk::EdgeRecs / hx_edges_out, these four and a head and a tail side.
#define HX_SIDE_COLUMNS(F) F(uint32_t, q_start, q_start, n) F(uint32_t, q_end, q_end, n) F(uint32_t, t_start, t_start, n) F(uint32_t, t_end, t_end, n) F(uint8_t, is_rev, is_rev, n) \
    F(uint64_t, cg_begin, cg_begin, n) F(uint64_t, cg_end, cg_end, n) F(uint32_t, cg_skip_front, cg_skip_front, n) F(uint32_t, cg_skip_back, cg_skip_back, n)
#define HX_REC_COLUMNS(F) F(uint64_t, key, key, n) F(uint32_t, lr, lr, n) F(uint32_t, cmp_head, cmp_head, n) F(uint32_t, cmp_tail, cmp_tail, n)
// Coordinate results (the kernels take them as plain pointers) / hx_coords_out: per selected edge, and per support; what is per support is also
// kept in a host mirror, for hx_poa_batch (with supp_off, the scan of the scratch).
#define HX_COORD_EDGE_COLUMNS(F) F(uint32_t, head_end, head_end, n_sel) F(uint32_t, tail_beg, tail_beg, n_sel)
#define HX_COORD_SUPP_COLUMNS(F) F(uint32_t, supp_lr, supp_lr, tot) F(uint32_t, spos, spos, tot) F(uint32_t, epos, epos, tot)

// what the generated code does with an entry (hx_internal.h; v = a kernels' struct, o = a public struct, h = the public hits, n = the count)
#define HX_COL_BUF(type, dev, pub, count) DV<type> dev;
#define HX_COL_MIRROR(type, dev, pub, count) std::vector<type> h_##dev;
#define HX_COL_MIRROR_KEEP(type, dev, pub, count) h_##dev.assign(o->pub, o->pub + n);
#define HX_COL_RESERVE(type, dev, pub, count) if ((e = dev.reserve(n)) != hipSuccess) return e;
#define HX_COL_UPLOAD(type, dev, pub, count) if (up(dev, h->pub, (size_t)(count))) return -1;
#define HX_COL_VIEW(type, dev, pub, count) v.dev = dev.p;
#define HX_COL_FETCH(type, dev, pub, count) ok = ok && fetch(o->pub, dev.p, n);
#define HX_COL_FREE(type, dev, pub, count) free(o->pub);
#define HX_COL_ONE(type, dev, pub, count) + 1

namespace hxi {
// every column is a pointer, and every other member of these structs is one 8-byte slot: a column added to a kernel's struct or a field added to a
// public struct without a line in its list does not compile
constexpr size_t kSlot = sizeof(void*), kHitColumns = 0 HX_HIT_COLUMNS(HX_COL_ONE), kChainColumns = 0 HX_CHAIN_COLUMNS(HX_COL_ONE), kSideColumns = 0 HX_SIDE_COLUMNS(HX_COL_ONE),
                 kRecColumns = 0 HX_REC_COLUMNS(HX_COL_ONE), kCoordColumns = 0 HX_COORD_EDGE_COLUMNS(HX_COL_ONE) HX_COORD_SUPP_COLUMNS(HX_COL_ONE);
static_assert(sizeof(DevHits) == (kHitColumns + 1) * kSlot && sizeof(hx_hits) == sizeof(DevHits), "HX_HIT_COLUMNS, DevHits and hx_hits list different columns (+ n)");
static_assert(sizeof(hxk::ChainFinal) == (kChainColumns + 1) * kSlot, "HX_CHAIN_COLUMNS and hxk::ChainFinal list different columns (+ cmp_aln)");
static_assert(sizeof(hxk::ChainScratch) == (kChainColumns + 5) * kSlot, "HX_CHAIN_COLUMNS and hxk::ChainScratch list different columns (+ dp, from, cmp, n_aln, n_cmp)");
static_assert(sizeof(hx_chain_out) == (kChainColumns + 6) * kSlot, "HX_CHAIN_COLUMNS and hx_chain_out list different columns (+ n_aln, n_reads, read_off, n_cmp, cmp_off, cmp_aln)");
static_assert(sizeof(DevSide) == kSideColumns * kSlot && sizeof(hx_rec_side) == sizeof(DevSide), "HX_SIDE_COLUMNS, DevSide and hx_rec_side list different columns");
static_assert(sizeof(hxk::EdgeRecs) == kRecColumns * kSlot + 2 * sizeof(DevSide), "HX_REC_COLUMNS and hxk::EdgeRecs list different columns (+ two sides)");
static_assert(sizeof(hx_edges_out) == (kRecColumns + 4) * kSlot + 2 * sizeof(hx_rec_side), "HX_REC_COLUMNS and hx_edges_out list different columns (+ n_rec, two sides, n_edge, edge_key, edge_off)");
static_assert(sizeof(hx_coords_out) == (kCoordColumns + 2) * kSlot, "HX_COORD_*_COLUMNS and hx_coords_out list different columns (+ n_edge, supp_off)");
}  // namespace hxi
