// poa_modes_plan_driver.cpp - runs a synthetic call of the general POA path through its plan alone (kernels/poa_modes_plan.hip compiled
// host-only: no HIP runtime in the link, no GPU) and prints what poa_modes_run would upload and launch (tests/test_poa_modes_plan.py). The
// stages follow poa_modes_run (kernels/poa_modes.hip); what a kernel would leave for a set comes from the case's rule (poa_modes_plan_text.h).
//   poa_modes_plan_driver CASE
// Lines that begin with "+ " show what no upload and no launch carries (needs, residents, the budget); the others are compared with the golden text.
#include "poa_modes_plan.h"
#include "poa_modes_plan_text.h"

using namespace hxk;
namespace pt = poa_modes_text;

template <class Row, class F> static void print_rows(const pt::Text& T, const char* kernel, const RowPlan<Row>& p, uint32_t stride, F row, std::initializer_list<std::pair<const char*, uint64_t>> allocs) {
    for (size_t k = 0; k < p.rows.size(); k++) row(k, p.rows[k]);
    for (const auto& al : allocs) T.alloc(al.first, al.second);
    for (const uint2& ch : p.chunks) T.chunk(kernel, ch.x, ch.y);
    T.rows_launch(kernel, p.blocks(), p.n_chunks(), stride);
}

int main(int argc, char** argv) {
    pt::Case cs;
    if (argc != 2 || !pt::make_case(argv[1], cs)) { fprintf(stderr, "usage: poa_modes_plan_driver CASE\n"); return 2; }
    const pt::Text T{stdout};
    const PoaModesArgs& a = cs.args;
    ModesCall c; ModesState st;
    std::string err;
    PoaModesOut o;
    if (describe(a, c, st, err)) { T.error(err); return 0; }
    if (!strncmp(argv[1], "bound_", 6)) {   // the score bound: describe's verdict is the case (no golden text: the check is younger than the harness that printed it)
        for (uint32_t i = 0; i < c.ns; i++) printf("accepted set %u sum_len %llu lmax %u columns %d\n", i, (unsigned long long)c.sets[i].sum_len, c.sets[i].lmax, INST_SHAPE[c.gm][inst_of(c, i)].nt * INST_SHAPE[c.gm][inst_of(c, i)].cpl);
        return 0;
    }
    o.seq_bases = c.seq_bases; o.n_aligned = c.n_aligned;
    const uint32_t ns = c.ns;
    const InstShape* shape = INST_SHAPE[c.gm];
    const bool wts = ((c.wtd || c.graph || c.strand) && a.weights) || c.graph || c.strand;   // a weight per base is on the device
    const int variant = c.strand ? 4 : c.graph ? 3 : wts ? 2 : c.cols ? 1 : 0;
    const int32_t sc[7] = {a.match, a.mismatch, a.gap, a.type, a.gap_extend, a.gap_open2, a.gap_extend2};
    const uint64_t budget = a.workspace_gb > 0 ? (uint64_t)(a.workspace_gb * 1e9) : (uint64_t)((double)pt::kFreeBytes * 0.4);
    uint64_t ws_cap = 0;
    std::vector<uint32_t> status(ns), vseen(ns), pairs(ns), ncols(ns, 0), len(ns, 0), nv(ns, 0), ne(ns, 0), cnt(c.nseq, 0);
    for (bool first = true; !st.todo.empty(); first = false) {
        uint64_t resident[N_INST] = {};
        for (int k = 0; k < N_INST; k++) {
            if (std::none_of(st.todo.begin(), st.todo.end(), [&](uint32_t i) { return inst_of(c, i) == k; })) continue;
            T.occ(shape[k].nt);
            resident[k] = (uint64_t)std::max(1, pt::occupancy(shape[k].nt)) * pt::kCUs;
        }
        const std::vector<uint32_t> todo = st.todo;
        RoundPlan p;
        if (plan_round(c, st, first, budget, resident, p, err)) { T.error(err); return 0; }
        if (p.total > ws_cap) { T.ws(p.total); ws_cap = p.total; }
        T.round(st.rounds - 1);
        if (first) {
            for (uint32_t i = 0; i < ns; i++) T.set(i, c.sets[i].seq_begin, c.sets[i].sum_len, c.sets[i].cns_off, c.sets[i].nseq, c.sets[i].lmax);
            T.bytes("codes", c.codes.data(), c.nb);
            if (c.strand) { T.bytes("codes_rc", c.codes_rc.data(), c.nb); if (!c.wts_rc.empty()) T.bytes("wts_rc", c.wts_rc.data(), c.nb); }
        }
        printf("+ round first %d budget %llu total %llu pool_pairs %llu todo", (int)first, (unsigned long long)budget, (unsigned long long)p.total, (unsigned long long)p.aln_pairs);
        for (uint32_t i : todo) printf(" %u", i);
        printf("\n");
        for (uint32_t i : todo)
            printf("+ need set %u inst %d pools %llu cells %llu cell_bytes %llu cost %llu\n", i, inst_of(c, i), (unsigned long long)pools_bytes(c.sets[i]), (unsigned long long)((st.vest[i] + 1) * (uint64_t)(c.sets[i].lmax + 1)),
                   (unsigned long long)CELL_BYTES[c.gm], (unsigned long long)(c.sets[i].sum_len * c.sets[i].lmax));
        for (int k = 0; k < N_INST; k++)
            if (!p.inst[k].sets.empty()) printf("+ inst %d columns %d slot %llu nslots %u resident %llu capped %d\n", k, shape[k].nt * shape[k].cpl, (unsigned long long)p.inst[k].slot, p.inst[k].nslots, (unsigned long long)resident[k], (int)(first && a.slot_kb_cap));
        if (c.graph) T.pool(std::max<uint64_t>(1, p.aln_pairs) * 4);
        std::fill(status.begin(), status.end(), 0xffffffffu);
        for (int k = 0; k < N_INST; k++) {
            const RoundPlan::PerInst& pk = p.inst[k];
            if (pk.sets.empty()) continue;
            T.launch(variant, pk.nslots, (uint32_t)shape[k].nt, (uint32_t)pk.sets.size(), pk.base, (uint64_t)k, pk.slot, sc);
            T.order(p.order.data() + pk.base, (uint32_t)pk.sets.size());
            for (uint32_t i : pk.sets) {
                const MSet& S = c.sets[i];
                if (c.graph) T.share(i, st.aln_at[i], st.aln_room[i]);
                const pt::SetResult r = pt::run_set(cs, i, pk.slot, pools_bytes(S), CELL_BYTES[c.gm], c.graph ? st.aln_room[i] : 0);
                T.result(i, r);
                status[i] = r.status; pairs[i] = r.pairs;
                if (r.status == 1) vseen[i] = r.vseen;
                if (!r.done) continue;
                len[i] = r.cns_len; nv[i] = r.nv; ne[i] = r.ne;
                if (c.cols) ncols[i] = r.ncols;
                for (uint32_t s = 0; s < S.nseq; s++) cnt[S.seq_begin + s] = r.cnt[s];
            }
        }
        if (after_round(c, st, first, status.data(), vseen.data(), pairs.data(), err)) { T.error(err); return 0; }
    }
    o.retried = st.retried; o.aln_retried = st.aln_retried;
    o.cns_off.assign((size_t)ns + 1, 0);
    for (uint32_t i = 0; i < ns; i++) o.cns_off[i + 1] = o.cns_off[i] + len[i];
    if (c.want_cov) {
        CovPlan p;
        if (plan_coverage(c, ncols, len, o.cns_off, p, err)) { T.error(err); return 0; }
        o.cov.assign(p.nc, 0);
        if (a.want_profile) o.prof.assign(4 * p.nc, 0);
        if (p.nc) {
            const uint64_t hist = std::max<uint64_t>(1, p.hist_words) * 4;
            if (p.seqs.n_chunks()) print_rows(T, "cov_hist", p.seqs, p.stride, [&](size_t k, const CovRow& r) { T.row("cov_hist", k, r.src, r.dst, r.hoff, r.len, r.ncols, 0, -1); }, {{"hist", hist}});
            print_rows(T, "cov_gather", p.cnss, p.stride, [&](size_t k, const CovRow& r) { T.row("cov_gather", k, r.src, r.dst, r.hoff, r.len, r.ncols, 0, -1); }, {{"hist", hist}});
            o.cov_moved_bytes = p.moved_bytes;
        }
    }
    if (c.graph) {
        GraphPlan p;
        if (plan_graph_out(c, st, nv, ne, cnt, len, o.cns_off, p, err)) { T.error(err); return 0; }
        o.node_off = p.node_off; o.edge_off = p.edge_off; o.aln_off = p.aln_off;
        if (p.rows.n_chunks()) {
            print_rows(T, "graph_gather", p.rows, 0, [&](size_t k, const GraphRow& r) { T.row("graph_gather", k, r.src, r.dst, 0, r.len, 0, r.kind, r.kind == ROW_ALN ? (long long)r.round : -1); },
                       {{"o_base", std::max<uint64_t>(1, p.NV)}, {"o_from", std::max<uint64_t>(1, p.NE) * 4}, {"o_cns", std::max<uint64_t>(1, p.NC) * 4}, {"o_aln", std::max<uint64_t>(1, p.NP) * 4}});
            o.gather_moved_bytes = p.moved_bytes;
        }
        for (uint32_t i = 0; i < ns; i++) printf("+ share set %u round %u at %llu room %u\n", i, st.pool_of[i], (unsigned long long)st.aln_at[i], st.aln_room[i]);
    } else if (c.msa) {
        MsaPlan p;
        if (plan_msa(c, ncols, len, o.cns_off, p, err)) { T.error(err); return 0; }
        o.msa_cols = ncols; o.msa_rows = p.msa_rows; o.msa_off = p.msa_off;
        o.msa.resize(p.out_bytes);
        if (p.out_bytes) {
            print_rows(T, "msa_rows", p.rows, 0, [&](size_t k, const MsaRow& r) { T.row("msa_rows", k, r.src, r.dst, 0, r.len, r.ncols, r.is_cns, -1); }, {{"msa_out", p.out_bytes}});
            o.msa_moved_bytes = p.moved_bytes;
        }
    }
    T.out(o);
    return 0;
}
