// poa_layout_driver.cpp - plans a synthetic consensus call with the POA planner alone (hx_poa_plan.hip compiled host-only: no HIP runtime in
// the link, no GPU) and prints the layout of every batch (tests/test_poa_layout.py). The rounds follow poa_consensus (hx_poa.hip); the
// statuses a kernel would report come from the case (poa_layout_text.h: Mark).
//   poa_layout_driver CASE
// Lines that begin with "+ " show what no upload and no launch carries (totals, classes, needs); the others are compared with the golden text.
#include "poa_layout_text.h"

namespace hxi {
thread_local std::string g_err;
int fail(const std::string& m) { g_err = m; return -1; }
}  // namespace hxi

using namespace hxi;

static void print_layout(FILE* f, PoaPlanner& K, const BatchLayout& Y, uint32_t shrink, const PoaCallShape& sh) {
    const poa_layout::Text T{f};
    T.batch(shrink, K.by_work, Y.bytes, Y.at, Y.tot.clo, Y.classes.size());
#define HX_F(name, type, total, factor) T.pool(#name, Y.off.name);
    HX_POA_POOLS(HX_F, HX_F)
#undef HX_F
    T.edges(K.P.edges.data(), Y.order_all.data(), Y.order_all.size(), sh.cls.data(), sh.shape.data());
    T.slots(Y.h_slots.data(), Y.h_slots.size());
    T.order(Y.order_all.data(), Y.order_all.size());
    T.btab(Y.h_btab.data(), Y.h_btab.size());
    for (size_t gi = 0; gi < Y.launches.size(); gi++) {
        const PoaLaunchRec& r = Y.launches[gi];
        T.launch(gi, r.stream, r.code, r.R, r.L, (long long)r.order_at, (long long)r.slot_at, r.persistent ? (long long)r.counter_at : -1, r.persistent ? (long long)r.btab_at : -1, r.started_at,
                 r.wait == PoaLaunchRec::kNoWait ? "none" : r.wait == PoaLaunchRec::kWaitStarted ? "started" : "delay");
        if (r.lds_bytes != r.L.ring_bytes) fprintf(f, "+ launch %zu lds_bytes %llu\n", gi, (unsigned long long)r.lds_bytes);
    }
    const PoaPoolTotals& t = Y.tot;
    fprintf(f, "+ totals no %llu eo %llu ho %llu dro %llu wo %llu so %llu sto %llu ao %llu clo %llu co %llu ne %llu\n", (unsigned long long)t.no, (unsigned long long)t.eo, (unsigned long long)t.ho, (unsigned long long)t.dro,
            (unsigned long long)t.wo, (unsigned long long)t.so, (unsigned long long)t.sto, (unsigned long long)t.ao, (unsigned long long)t.clo, (unsigned long long)t.co, (unsigned long long)t.ne);
#define HX_F(name, type, total, factor) fprintf(f, "+ pool_size %s %llu\n", #name, (unsigned long long)((uint64_t)(factor) * t.total * sizeof(type)));
    HX_POA_POOLS(HX_F, HX_F)
#undef HX_F
    std::vector<Cls> again = Y.classes;
    fprintf(f, "+ total_bytes %llu budget %llu\n", (unsigned long long)K.total_bytes(again, shrink), (unsigned long long)K.budget);
    for (size_t i = 0; i < Y.classes.size(); i++) {
        const Cls& q = Y.classes[i];
        fprintf(f, "+ class %zu shared %d persistent %d nt %u cm %u dir %d dpl %u pb %u pk %d n_slots %zu blocks %zu order_at %zu slot_at %zu edges", i, (int)q.shared, (int)q.persistent, q.nt, q.cm, (int)q.dir, q.dpl, q.pb, (int)q.pk,
                q.n_slots, q.blocks, q.order_at, q.slot_at);
        for (uint32_t e : q.edges) fprintf(f, " %u", e);
        fprintf(f, "\n");
        for (size_t k = 0; k < q.n_slots; k++) {
            const Need n = K.slot_need(q, k);
            fprintf(f, "+ need %zu nn %llu ec %llu hc %llu dc %llu wc %llu lm %llu st %llu al %llu mb %llu\n", q.slot_at + k, (unsigned long long)n.nn, (unsigned long long)n.ec, (unsigned long long)n.hc, (unsigned long long)n.dc,
                    (unsigned long long)n.wc, (unsigned long long)n.lm, (unsigned long long)n.st, (unsigned long long)n.al, (unsigned long long)n.mb);
        }
    }
    for (const auto& g : Y.groups) fprintf(f, "+ group classes %zu %zu btab_at %zu\n", g[0], g[1], g[2]);
}

int main(int argc, char** argv) {
    poa_layout::Case cs;
    if (argc != 2 || !poa_layout::make_case(argv[1], cs)) { fprintf(stderr, "usage: poa_layout_driver a|b|c_block|c_ring|d|e|f|g\n"); return 2; }
    const PoaInput in = cs.in.view();
    const hx_poa_params pp{3, -5, -4};
    PoaPlanner K(in, &pp, cs.opt, cs.poa_block, cs.poa_no_dir);
    std::vector<uint32_t> todo;
    if (K.plan_input(todo)) { fprintf(stderr, "%s\n", g_err.c_str()); return 1; }
    K.budget = cs.opt.poa_workspace_gb > 0 ? (uint64_t)(cs.opt.poa_workspace_gb * 1e9) : poa_layout::kBudget;
    PoaCallShape sh;
    sh.cls.assign(K.ne, POA_NO_CLASS); sh.shape.assign(K.ne, 0);
    std::vector<uint32_t> status(K.ne, 0);
    for (const poa_layout::Mark& m : cs.marks) status[m.edge] = m.status;
    for (int round = 0; !todo.empty(); round++) {
        if (K.knobs(todo.size()) || K.size_edges(todo)) { fprintf(stderr, "%s\n", g_err.c_str()); return 1; }
        std::vector<std::vector<uint32_t>> batches;
        std::vector<uint32_t> batch_shrink;
        if (K.plan_batches(todo, batches, batch_shrink)) { fprintf(stderr, "%s\n", g_err.c_str()); return 1; }
        std::vector<uint32_t> retry, retry_same;
        for (size_t bi = 0; bi < batches.size(); bi++) {
            if (batches[bi].empty()) continue;
            K.by_work = bi < K.batch_by_work.size() && K.batch_by_work[bi] != 0;
            BatchLayout Y;
            if (K.layout_slots(batches[bi], batch_shrink[bi], Y)) { fprintf(stderr, "%s\n", g_err.c_str()); return 1; }
            K.layout_order(Y); K.layout_launches(Y);   // (the three steps of the layout, in launch_batch's order)
            for (const auto& es : Y.shapes) { sh.cls[es[0]] = (uint8_t)es[1]; sh.shape[es[0]] = es[2]; }
            print_layout(stdout, K, Y, batch_shrink[bi], sh);
            for (uint32_t e : batches[bi]) {   // the verdicts of collect_batch (hx_poa.hip), in its order
                const uint32_t st = status[e];
                status[e] = 0;
                if (st & HXE_POA_FARROWS) { K.far_full[e]++; retry_same.push_back(e); }
                else if (st & HXE_POA_STALLED) { K.no_share[e] = 1; retry_same.push_back(e); }
                else if (st & HXE_POA_WIDEROWS) { K.wide_grow[e]++; retry_same.push_back(e); }
                else if (st & HXE_POA_SINKS) { K.many_sinks[e] = 1; retry_same.push_back(e); }
                else if (st & HXE_POA_NODIR) { K.force_nodir[e] = 1; retry_same.push_back(e); }
                else if (st & HXE_POA_OVERFLOW) { K.grow[e]++; retry.push_back(e); }
            }
        }
        todo.swap(retry);
        todo.insert(todo.end(), retry_same.begin(), retry_same.end());
    }
    return 0;
}
