// hx_poa_report.cpp - sums and prints the diagnostic words of a consensus call. Every word is taken by its name and every packed word by the helpers of
// kernels/poa_phase_words.h: the kernel that writes them uses the same.
#include "hx_poa_report.h"

#include <algorithm>
#include <utility>
#include <vector>

namespace hxi {
using namespace hxk;
namespace {
typedef unsigned long long W;
constexpr int N_CLS = POA_NO_CLASS + 1;
W cycles(const PoaReportView& v, size_t e) { W t = 0; for (int k = 0; k < PW_N_PHASES; k++) t += v.edge(e)[k]; return t; }
std::vector<std::pair<W, uint32_t>> longest(const PoaReportView& v) {   // the five edges with the most phase cycles (the critical-path candidates), longest first
    std::vector<std::pair<W, uint32_t>> tt;
    for (size_t e = 0; e < v.n_edges; e++) tt.push_back({cycles(v, e), (uint32_t)e});
    std::sort(tt.rbegin(), tt.rend());
    tt.resize(std::min<size_t>(5, tt.size()));
    return tt;
}
W refs(W w) { return pw_lo(w, PW_SPLIT_REFS); }      // PW_RING_FIFTH, PW_FAR_WIDE: the references
W extra(W w) { return pw_hi(w, PW_SPLIT_REFS); }     // ... fifth-and-later entries, rows with more than 4 predecessors
W seqs(W w) { return pw_lo(w, PW_SPLIT_HALF); }      // PW_SEQS_NODES
void report_rowseg(const PoaReportView& v) {   // (a build with -DHX_DP_PROF: where the rows of the first wave of every workgroup spend their cycles, per launch class)
    static const char* seg[PW_N_BUILD] = {"decode", "predecessors + cells + chain", "wave scan", "carry", "carry applied + ring", "stores"};
    W cs[N_CLS][PW_N_BUILD + 1] = {};
    for (size_t e = 0; e < v.n_edges; e++) { const int k = v.cls_of(e); for (int j = 0; j < PW_N_BUILD; j++) cs[k][j] += v.edge(e)[PW_SEG0 + j]; cs[k][PW_N_BUILD] += v.edge(e)[PW_DP]; }
    for (int k = 0; k < N_CLS; k++) {
        W t = 0; for (int j = 0; j < PW_N_BUILD; j++) t += cs[k][j];
        if (!t) continue;
        fprintf(v.out, "[hx] prof1 class %d: row segments of wave 0, %.3g cycles (DP phase %.3g):", k, (double)t, (double)cs[k][PW_N_BUILD]);
        for (int j = 0; j < PW_N_BUILD; j++) fprintf(v.out, " %s %.1f %%%s", seg[j], 100.0 * (double)cs[k][j] / (double)t, j < PW_N_BUILD - 1 ? "," : "\n");
    }
}
void report_dpsub(const PoaReportView& v) {   // (a build with -DHX_DP_PROF -DHX_DP_PROF2: where member 0's DP phase goes, for the five longest edges)
    for (const auto& t : longest(v)) {
        const W* q = v.edge(t.second);
        fprintf(v.out, "[hx] prof2 edge %u lmax=%u nseq=%u dp phase %llu: publish %llu own columns %llu wait members %llu end node %llu (ties sorted %llu, toposort %llu)\n", t.second, v.lmax[t.second],
                v.nseq[t.second], q[PW_DP], q[PW_P2_PUBLISH], q[PW_P2_OWN], q[PW_P2_WAIT], q[PW_P2_END], q[PW_P2_TIES], q[PW_P2_TOPO]);
    }
}
void report_members(const PoaReportView& v) {   // (a build with -DHX_DP_PROF3: per member of the five longest edges, kilocycles inside the DP and of them waiting for carries)
    for (const auto& t : longest(v)) {
        const W* q = v.edge(t.second);
        fprintf(v.out, "[hx] prof3 edge %u lmax=%u nseq=%u dp %llu:", t.second, v.lmax[t.second], v.nseq[t.second], q[PW_DP]);
        for (int m = 0; m < PW_N_BUILD; m++) fprintf(v.out, " m%d dp %lluk wait %lluk", m, pw_lo(q[PW_P3_MEMBER0 + m], PW_SPLIT_HALF), pw_hi(q[PW_P3_MEMBER0 + m], PW_SPLIT_HALF));
        fprintf(v.out, "\n");
    }
}
void report_batchhead(const PoaReportView& v) {   // (a build with -DHX_DP_PROF4: what a carry batch costs the waves with a left neighbour in their workgroup besides its rows, for the five longest edges)
    for (const auto& t : longest(v)) {
        const W* q = v.edge(t.second);
        const W n = pw_hi(q[PW_BH_CLOCK], PW_SPLIT_HALF), ready = q[PW_BH_READY], polled = q[PW_BH_POLLED];
        fprintf(v.out, "[hx] prof4 edge %u lmax=%u nseq=%u dp %llu: waves x DPs %llu, batches %llu of %.2f rows (%.1f per wave and DP); carries there %llu batches, %.0f cycles each; polled %llu batches, %.0f cycles each; two clock reads %.0f cycles\n",
                t.second, v.lmax[t.second], v.nseq[t.second], q[PW_DP], n, ready + polled, ready + polled ? (double)q[PW_BH_ROWS] / (double)(ready + polled) : 0.0, n ? (double)(ready + polled) / (double)n : 0.0,
                ready, ready ? (double)q[PW_BH_READY_CYCLES] / (double)ready : 0.0, polled, polled ? (double)q[PW_BH_POLLED_CYCLES] / (double)polled : 0.0, n ? (double)pw_lo(q[PW_BH_CLOCK], PW_SPLIT_HALF) / (double)n : 0.0);
    }
}
void report_edges(const PoaReportView& v) {   // every edge: shape of its launch, begin and end on the 100 MHz wall clock (relative to the call's first edge), phase cycles, DP rows
    W t0 = ~0ull;
    for (size_t e = 0; e < v.n_edges; e++) if (v.edge(e)[PW_BEGIN]) t0 = std::min(t0, pw_lo(v.edge(e)[PW_BEGIN], PW_SPLIT_CLOCK));
    for (size_t e = 0; e < v.n_edges; e++) {
        const W* q = v.edge(e);
        if (!q[PW_BEGIN]) continue;
        const uint32_t sh = v.shape_of(e);
        fprintf(v.out, "[hx-edge] %zu lmax %u nseq %u cls %d lanes %u passes %u members %u hw %u begin_us %.1f end_us %.1f decode %llu dp %llu tb %llu graph %llu order %llu csr %llu rows %llu wrows %llu wskip %llu wbulk %llu cns %llu refcns %llu\n", e, v.lmax[e], v.nseq[e],
                v.cls_of(e), sh & 0xffffu, (sh >> 16) & 255u, sh >> 24, (unsigned)pw_hi(q[PW_BEGIN], PW_SPLIT_CLOCK), (double)(pw_lo(q[PW_BEGIN], PW_SPLIT_CLOCK) - t0) * 0.01, (double)(q[PW_END] - t0) * 0.01, q[PW_DECODE], q[PW_DP], q[PW_TRACEBACK], q[PW_GRAPH], q[PW_ORDER], q[PW_CSR], q[PW_ROWS], q[PW_PRUNE_ROWS], q[PW_PRUNE_SKIPPED], q[PW_PRUNE_BULK], q[PW_CNS], q[PW_REFCNS]);
    }
}
void report_rowstats(const PoaReportView& v, uint32_t slowest) {   // the default build's summary
    const size_t ne = v.n_edges;
    const W* q = v.edge(slowest);
    fprintf(v.out, "[hx] slowest edge %u: lmax=%u nseq=%u | DP rows %llu (multi-pred %llu, ring refs %llu, far refs %llu, kept %llu, more than 4 predecessors %llu, fifth-and-later entries %llu) over %llu sequences\n", slowest,
            v.lmax[slowest], v.nseq[slowest], q[PW_ROWS], q[PW_MULTI], refs(q[PW_RING_FIFTH]), refs(q[PW_FAR_WIDE]), q[PW_KEPT], extra(q[PW_FAR_WIDE]), extra(q[PW_RING_FIFTH]), seqs(q[PW_SEQS_NODES]));
    for (const auto& t : longest(v)) {
        const W* q2 = v.edge(t.second);
        fprintf(v.out, "[hx] top edge %u: lmax=%u nseq=%u cycles=%llu (dp %llu tb %llu graph %llu order %llu csr %llu) rows %llu multi %llu ring %llu far %llu kept %llu wide %llu fifth+ %llu\n", t.second, v.lmax[t.second], v.nseq[t.second],
                t.first, q2[PW_DP], q2[PW_TRACEBACK], q2[PW_GRAPH], q2[PW_ORDER], q2[PW_CSR], q2[PW_ROWS], q2[PW_MULTI], refs(q2[PW_RING_FIFTH]), refs(q2[PW_FAR_WIDE]), q2[PW_KEPT], extra(q2[PW_FAR_WIDE]), extra(q2[PW_RING_FIFTH]));
    }
    {   // finished graphs against the workspace estimate: nodes per base of the longest sequence, as a + b x sequences
        std::vector<double> grow, fill;
        for (size_t e = 0; e < ne; e++) {
            const double V = (double)pw_hi(v.edge(e)[PW_SEQS_NODES], PW_SPLIT_HALF), L = v.lmax[e], S = v.nseq[e];
            if (V <= 0 || L <= 0 || S <= 0) continue;
            grow.push_back((V - L) / (L * S));
            fill.push_back(V / (L * (3 + S / 10) + 1024));
        }
        std::sort(grow.begin(), grow.end()); std::sort(fill.begin(), fill.end());
        auto pc = [](const std::vector<double>& x, double p) { return x.empty() ? 0.0 : x[std::min(x.size() - 1, (size_t)(p * x.size()))]; };
        fprintf(v.out, "[hx] graph growth (nodes - L) / (L x sequences): median %.3f  p90 %.3f  p99 %.3f  max %.3f | nodes / estimate: median %.2f  p99 %.2f  max %.2f\n",
                pc(grow, 0.5), pc(grow, 0.9), pc(grow, 0.99), pc(grow, 1.0), pc(fill, 0.5), pc(fill, 0.99), pc(fill, 1.0));
    }
    {   // per launch class: how often a row is read back from the LDS ring / from HBM; then edges, all cycles, DP cycles, longest edge
        W cr[N_CLS][4] = {}, cy[N_CLS][4] = {};
        for (size_t e = 0; e < ne; e++) {
            const int k = v.cls_of(e); const W* q3 = v.edge(e); const W t = cycles(v, e);
            cr[k][0] += q3[PW_ROWS]; cr[k][1] += q3[PW_KEPT]; cr[k][2] += refs(q3[PW_RING_FIFTH]); cr[k][3] += refs(q3[PW_FAR_WIDE]);
            cy[k][0]++; cy[k][1] += t; cy[k][2] += q3[PW_DP]; cy[k][3] = std::max(cy[k][3], t);
        }
        for (int k = 0; k < N_CLS; k++) if (cr[k][0]) fprintf(v.out, "[hx] class %d (ring %u): DP rows %llu, kept %.1f %%, ring refs %.1f %%, far refs %.2f %%\n", k, k < N_CLS - 1 ? v.ring[k] : 0, cr[k][0], 100.0 * cr[k][1] / cr[k][0], 100.0 * cr[k][2] / cr[k][0], 100.0 * cr[k][3] / cr[k][0]);
        for (int k = 0; k < N_CLS; k++) if (cy[k][0]) fprintf(v.out, "[hx] class %d: %llu workgroups, %.3e cycles in all (DP %.0f %%), longest %.3e, DP cycles per row %.0f\n", k, cy[k][0], (double)cy[k][1], 100.0 * cy[k][2] / cy[k][1], (double)cy[k][3], cr[k][0] ? (double)cy[k][2] / cr[k][0] : 0.0);
    }
    {   // the pruning (kernels/poa.hip PRUNE): wave-rows of the pruned launches, those skipped, attempts repeated, per launch class
        W pr[N_CLS][PW_N_PRUNE] = {};
        for (size_t e = 0; e < ne; e++) for (int j = 0; j < PW_N_PRUNE; j++) pr[v.cls_of(e)][j] += v.edge(e)[PW_PRUNE0 + j];
        constexpr int ROWS = PW_PRUNE_ROWS - PW_PRUNE0, SKIPPED = PW_PRUNE_SKIPPED - PW_PRUNE0, REPEATED = PW_PRUNE_REPEATED - PW_PRUNE0, THRESHOLDS = PW_PRUNE_THRESHOLDS - PW_PRUNE0;
        for (int k = 0; k < N_CLS; k++) if (pr[k][ROWS]) fprintf(v.out, "[hx] class %d pruning: %.4g wave-rows, %.1f %% skipped, %llu alignments with a threshold, %llu repeated\n", k, (double)pr[k][ROWS], 100.0 * pr[k][SKIPPED] / pr[k][ROWS], pr[k][THRESHOLDS], pr[k][REPEATED]);
    }
    W tot[6] = {0, 0, 0, 0, 0, 0};
    for (size_t e = 0; e < ne; e++) { const W* q3 = v.edge(e); tot[0] += q3[PW_ROWS]; tot[1] += q3[PW_MULTI]; tot[2] += refs(q3[PW_RING_FIFTH]); tot[3] += refs(q3[PW_FAR_WIDE]); tot[4] += q3[PW_KEPT]; tot[5] += seqs(q3[PW_SEQS_NODES]); }
    fprintf(v.out, "[hx] all edges: DP rows %llu (multi-pred %llu, ring refs %llu, far refs %llu, kept %llu) over %llu sequences\n", tot[0], tot[1], tot[2], tot[3], tot[4], tot[5]);
}
}  // namespace

PoaReport poa_phase_report(const PoaReportView& v, uint64_t* sum6, uint64_t* max6) {
    // lane-0 cycle counters of the last consensus call: [decode, dp, traceback, graph update+consensus, toposort, csr];
    // sum over edges and the breakdown of the edge with the largest total (the critical path)
    PoaReport res{(uint32_t)v.n_edges, 0};
    W best = 0;
    for (int k = 0; k < PW_N_PHASES; k++) { sum6[k] = 0; max6[k] = 0; }
    for (size_t e = 0; e < v.n_edges; e++) for (int k = 0; k < PW_N_PHASES; k++) if ((long long)v.words[e * POA_PHASE_WORDS + k] < 0) v.words[e * POA_PHASE_WORDS + k] = 0;   // (a phase that began and ended on different waves' clocks)
    for (size_t e = 0; e < v.n_edges; e++) {
        for (int k = 0; k < PW_N_PHASES; k++) sum6[k] += v.edge(e)[k];
        if (cycles(v, e) > best) { best = cycles(v, e); for (int k = 0; k < PW_N_PHASES; k++) max6[k] = v.edge(e)[k]; res.slowest = (uint32_t)e; }
    }
    if (!v.debug || !v.n_edges) return res;
    if (v.prof == 1) report_rowseg(v);
    else if (v.prof == 2) report_dpsub(v);
    else if (v.prof == 3) report_members(v);
    else if (v.prof == 4) report_batchhead(v);
    else { if (v.debug >= 2) report_edges(v); report_rowstats(v, res.slowest); }
    return res;
}
void poa_prune_sums(const unsigned long long* words, size_t n_edges, uint64_t* out4) {
    for (int j = 0; j < PW_N_PRUNE; j++) out4[j] = 0;
    for (size_t e = 0; e < n_edges; e++) for (int j = 0; j < PW_N_PRUNE; j++) out4[j] += words[e * POA_PHASE_WORDS + PW_PRUNE0 + j];
}
}  // namespace hxi
