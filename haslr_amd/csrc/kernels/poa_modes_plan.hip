// poa_modes_plan.hip — the host arithmetic of the general POA path (poa_modes_plan.h). Host code only: it makes no HIP call and holds no
// kernel; it is a .hip file because carve_pools takes the graph type of poa_graph.inl, which is HIP text.
#include <algorithm>

#include "kernels.h"
#include "poa_modes_plan.h"

namespace hxk {

namespace {
#include "poa_graph.inl"         // G
#include "poa_modes_pools.inl"   // al256, carve_pools
}  // namespace

uint64_t pools_bytes(const MSet& S) { return carve_pools(nullptr, S.sum_len, S.nseq, S.lmax, nullptr, nullptr, nullptr); }
uint64_t phase_pool_bytes(uint64_t sum_len, uint32_t nseq) { return carve_phase(nullptr, sum_len, nseq, nullptr); }
uint64_t slot_pools_bytes(const ModesCall& c, uint32_t set) { return pools_bytes(c.sets[set]) + (c.phase ? phase_pool_bytes(c.sets[set].sum_len, c.sets[set].nseq) : 0); }

int inst_of(const ModesCall& c, uint32_t set) {
    const InstShape* inst = INST_SHAPE[c.gm];
    int k = 0;
    while ((uint64_t)inst[k].nt * inst[k].cpl < (uint64_t)c.sets[set].lmax + 1) k++;
    return k;
}

int slot_of(const ModesCall& c, const ModesState& st, uint32_t set) { return c.band && st.band[set] ? BAND_INST : inst_of(c, set); }

uint32_t next_band(uint32_t w, uint32_t lmax) {
    const uint32_t w2 = 2 * w;
    return w2 <= MAX_BAND && (uint64_t)lmax + 1 > 2 * (uint64_t)w2 + 1 ? w2 : 0u;
}

int describe(const PoaModesArgs& a, ModesCall& c, ModesState& st, std::string& err) {
    c = ModesCall();
    st = ModesState();
    c.a = &a; c.who = a.who; c.ns = a.n_sets; c.gm = a.gap_model;
    c.msa = a.msa != 0; c.wtd = a.weighted != 0; c.graph = a.graph != 0; c.strand = a.strand != 0;
    c.phase = a.phase != 0;
    if (c.phase && a.labels) { err = c.who + ": a phased call derives its labels itself and takes none"; return -1; }
    c.labels = a.labels != nullptr || c.phase; c.nl = c.phase ? 2u : c.labels ? a.n_labels : 1u; c.lab = a.labels;
    c.cols = c.msa || c.wtd || c.graph || c.strand || c.labels;
    c.want_cov = (c.wtd || c.strand || c.labels) && (a.want_coverage || a.want_profile);
    c.band = a.band != 0;
    if (c.labels && (c.nl < 1 || c.nl > 16)) { err = c.who + ": n_labels must be 1..16, not " + std::to_string(c.nl); return -1; }
    if (c.phase && (a.phase_min_count < 1 || a.phase_min_count > 255)) { err = c.who + ": min_count must be 1..255, not " + std::to_string(a.phase_min_count); return -1; }
    if (c.phase && (a.phase_min_pct < 1 || a.phase_min_pct > 50)) { err = c.who + ": min_pct must be 1..50, not " + std::to_string(a.phase_min_pct); return -1; }
    if (c.phase && (c.graph || c.strand || c.band)) { err = c.who + ": graph output, strand-ambiguous sets and banded alignment have no phasing"; return -1; }
    if (c.labels && (c.graph || c.strand || c.band)) { err = c.who + ": graph output, strand-ambiguous sets and banded alignment have no labels"; return -1; }
    if (c.band && a.band > MAX_BAND) { err = c.who + ": the band half-width must be 1.." + std::to_string(MAX_BAND) + ", not " + std::to_string(a.band); return -1; }
    if (c.band && (c.graph || c.strand)) { err = c.who + ": graph output and strand-ambiguous sets have no band"; return -1; }
    const uint32_t ns = c.ns;
    const int gm = c.gm;
    c.nseq = a.set_off[ns]; c.nb = a.seq_off[c.nseq];
    c.sets.resize(ns);
    const uint32_t nl = c.nl;
    c.cns_off.assign((size_t)ns * nl + 1, 0);
    const uint32_t max_len = MAX_LEN[gm];
    for (uint32_t i = 0; i < ns; i++) {
        MSet& S = c.sets[i];
        S.seq_begin = a.set_off[i]; S.nseq = (uint32_t)(a.set_off[i + 1] - a.set_off[i]); S.sum_len = 0; S.lmax = 0;
        for (uint64_t k = a.set_off[i]; k < a.set_off[i + 1]; k++) {
            const uint64_t L = a.seq_off[k + 1] - a.seq_off[k];
            if (L > max_len) { err = c.who + ": set " + std::to_string(i) + " holds a sequence of " + std::to_string(L) + " bases, longer than " + std::to_string(max_len) + (gm == GM_CONVEX ? " (the longest the general POA path takes with convex gaps)" : gm == GM_AFFINE ? " (the longest the general POA path takes with affine gaps)" : " (the longest the general POA path takes)"); return -1; }
            S.sum_len += L; S.lmax = std::max(S.lmax, (uint32_t)L);
            c.seq_bases += L; c.n_aligned += L != 0;
        }
        if (S.sum_len > MAX_SET_BASES) { err = c.who + ": set " + std::to_string(i) + " holds " + std::to_string(S.sum_len) + " bases in all, more than the " + std::to_string(MAX_SET_BASES) + " nodes a graph can have"; return -1; }
        S.cns_off = c.cns_off[(size_t)i * nl];   // (a consensus has at most one base per node; a labelled set has nl places of that size)
        for (uint32_t g = 0; g < nl; g++) c.cns_off[(size_t)i * nl + g + 1] = c.cns_off[(size_t)i * nl + g] + S.sum_len;
    }
    int64_t mag = 0;   // the largest score magnitude
    for (const int32_t v : {a.match, a.mismatch, a.gap, a.gap_extend, a.gap_open2, a.gap_extend2}) mag = std::max<int64_t>(mag, v < 0 ? -(int64_t)v : v);
    if (c.band) {
        // every real value of a banded set's matrices stays above -2^28 and every value derived from minus infinity at or below it
        st.band.assign(ns, 0);
        for (uint32_t i = 0; i < ns; i++) {
            const MSet& S = c.sets[i];
            if ((int64_t)(S.sum_len + S.lmax) * mag >= BAND_SCORE_BOUND) { err = c.who + ": set " + std::to_string(i) + " holds " + std::to_string(S.sum_len) + " bases, its longest sequence " + std::to_string(S.lmax) + ": with scores of up to " + std::to_string(mag) + " their product " + std::to_string((int64_t)(S.sum_len + S.lmax) * mag) + " reaches 2^28 = " + std::to_string(BAND_SCORE_BOUND) + " (a banded set's scores must stay below it)"; return -1; }
            st.band[i] = (uint64_t)S.lmax + 1 <= 2 * (uint64_t)a.band + 1 ? 0u : a.band;   // (a window that holds the longest sequence is the full matrix)
        }
    }
    // The full matrix (a banded set may end there): a real value is a sum of at most nodes + columns scores, dp_rows computes every column of the set's
    // instance, those past the sequence on minus infinity, and its scans shift column j by j gap scores. Below the bound none of that leaves int32,
    // and a real value stays above -2^29, a value derived from it at or below (DESIGN.md "Score range of the full matrix")
    for (uint32_t i = 0; i < ns; i++) {
        const MSet& S = c.sets[i];
        if (!S.sum_len) continue;
        const InstShape sh = INST_SHAPE[gm][inst_of(c, i)];
        const int64_t cols = (int64_t)sh.nt * sh.cpl, prod = ((int64_t)S.sum_len + cols) * mag;
        if (prod >= SCORE_BOUND) { err = c.who + ": set " + std::to_string(i) + " holds " + std::to_string(S.sum_len) + " bases, its instance " + std::to_string(cols) + " columns: with scores of up to " + std::to_string(mag) + " their product " + std::to_string(prod) + " reaches 2^29 = " + std::to_string(SCORE_BOUND) + " (a set's scores must stay below it)"; return -1; }
    }
    c.codes.resize(std::max<uint64_t>(1, c.nb));
    for (uint64_t k = 0; k < c.nb; k++) c.codes[k] = base_code(a.bases[k]);
    if (c.strand) {
        c.codes_rc.resize(c.codes.size());
        if (a.weights) c.wts_rc.resize(c.codes.size());
        for (uint64_t k = 0; k < c.nseq; k++) {
            const uint64_t b = a.seq_off[k], L = a.seq_off[k + 1] - b;
            for (uint64_t i = 0; i < L; i++) { c.codes_rc[b + i] = (uint8_t)(3 - c.codes[b + L - 1 - i]); if (a.weights) c.wts_rc[b + i] = a.weights[b + L - 1 - i]; }
        }
    }
    if (c.graph) {
        // The share of the alignment pool a set gets in its first round. The alignment of a sequence of L bases holds one pair per base
        // and one per graph node the walk passes without a base; under kNW the walk spans the graph from a source to a sink, which for
        // copies of one template is about the longest sequence. So: max(L, longest) pairs, an eighth more for the nodes passed without
        // a base (the copy's deletions against that path: 3 % in the error models of the tests and the bench tool, a quarter of that
        // room), and 16 for short sequences, per sequence after the first non-empty one (DESIGN.md "Graph and alignment output" has
        // the reasoning and the measured reruns)
        st.pool_of.assign(ns, 0); st.aln_room.assign(ns, 0); st.aln_rerun.assign(ns, 0); st.aln_at.assign(ns, 0);
        for (uint32_t i = 0; i < ns; i++) {
            uint64_t est = 0;
            bool seen = false;
            for (uint64_t k = a.set_off[i]; k < a.set_off[i + 1]; k++) {
                const uint64_t L = a.seq_off[k + 1] - a.seq_off[k];
                if (L == 0) continue;
                if (seen) { const uint64_t span = std::max<uint64_t>(L, c.sets[i].lmax); est += span + span / 8 + 16; }
                seen = true;
            }
            st.aln_room[i] = (uint32_t)std::min<uint64_t>(est, 0xfffffffeu);
            if (a.aln_cap) st.aln_room[i] = std::min(st.aln_room[i], a.aln_cap);   // (test switch: forces the overflow and the rerun with the exact room)
        }
    }
    // H is sized from an estimate of the graph's final size (noisy copies add about a tenth of their length each); a set that outgrows its
    // slot comes back and is rerun with twice the room (or the room for what it had when it stopped, doubled), the worst case at most
    st.vest.resize(ns);
    for (uint32_t i = 0; i < ns; i++) { st.vest[i] = std::min<uint64_t>(c.sets[i].sum_len, c.sets[i].lmax + c.sets[i].sum_len / 8 + 64); if (c.sets[i].sum_len) st.todo.push_back(i); }
    return 0;
}

int plan_round(const ModesCall& c, ModesState& st, const bool first, const uint64_t budget, const uint64_t* resident, RoundPlan& p, std::string& err) {
    const PoaModesArgs& a = *c.a;
    const std::vector<MSet>& sets = c.sets;
    const uint64_t cell_bytes = CELL_BYTES[c.gm];
    // (a banded set: vest + 1 rows of B cells, and the rows' three word arrays)
    auto need = [&](uint32_t i) {
        if (c.band && st.band[i]) return slot_pools_bytes(c, i) + al256((st.vest[i] + 1) * (2 * (uint64_t)st.band[i] + 1) * cell_bytes + 12 * (st.vest[i] + 1));
        return slot_pools_bytes(c, i) + al256((st.vest[i] + 1) * (uint64_t)(sets[i].lmax + 1) * cell_bytes);
    };
    p = RoundPlan();
    for (uint32_t i : st.todo) p.inst[slot_of(c, st, i)].sets.push_back(i);
    for (int k = 0; k < N_SLOTS; k++) {
        auto& v = p.inst[k].sets;
        if (v.empty()) continue;
        std::stable_sort(v.begin(), v.end(), [&](uint32_t x, uint32_t y) { return sets[x].sum_len * sets[x].lmax > sets[y].sum_len * sets[y].lmax; });
        uint64_t sb = 0, pmax = 0;
        uint32_t big = v[0];
        for (uint32_t i : v) {
            const uint64_t nd = need(i);
            if (nd > sb) { sb = nd; big = i; }
            pmax = std::max(pmax, slot_pools_bytes(c, i));
        }
        if (first && a.slot_kb_cap) sb = std::max(pmax, std::min<uint64_t>(sb, (uint64_t)a.slot_kb_cap << 10));   // (test switch: forces the overflow and rerun)
        sb = al256(sb);
        const uint64_t fit = budget / sb;
        if (fit == 0) { err = c.who + ": set " + std::to_string(big) + " needs " + std::to_string(sb) + " bytes of workspace, more than the budget of " + std::to_string(budget) + " (option poa_workspace_gb)"; return -1; }
        p.inst[k].slot = sb; p.inst[k].nslots = (uint32_t)std::min<uint64_t>({(uint64_t)v.size(), resident[k], fit});
        p.inst[k].base = p.order.size();
        p.order.insert(p.order.end(), v.begin(), v.end());
        p.total = std::max(p.total, p.inst[k].nslots * sb);   // (the instances run one after the other on the stream: they share the workspace)
    }
    if (c.graph) {   // this round's pool: the shares of its sets side by side
        for (uint32_t i : st.todo) { st.pool_of[i] = st.rounds; st.aln_at[i] = p.aln_pairs; p.aln_pairs += st.aln_room[i]; }
    }
    st.rounds++;
    return 0;
}

int after_round(const ModesCall& c, ModesState& st, const bool first, const uint32_t* status, const uint32_t* vseen, const uint32_t* pairs, std::string& err) {
    const PoaModesArgs& a = *c.a;
    std::vector<uint32_t> next;
    for (uint32_t i : st.todo) {
        if (status[i] == MS_OK) continue;
        if (c.graph && status[i] == MS_ALN_OVERFLOW) {   // done, but for its alignments: once more, with exactly the room they need (pairs: what they hold in all)
            if (st.aln_rerun[i] || pairs[i] == 0xffffffffu) { err = c.who + ": set " + std::to_string(i) + " failed on the device (its alignments hold " + std::to_string(pairs[i]) + " pairs, its share of the pool " + std::to_string(st.aln_room[i]) + ")"; return -1; }
            st.aln_rerun[i] = 1; st.aln_room[i] = pairs[i];
            next.push_back(i);
            st.aln_retried++;
            continue;
        }
        if (c.band && st.band[i] && status[i] == MS_BAND_MISS) {   // from its first sequence again, in twice the band or on the full matrix
            st.band[i] = next_band(st.band[i], c.sets[i].lmax);
            next.push_back(i);
            st.band_retried++;
            continue;
        }
        const bool capped = first && a.slot_kb_cap;   // (a capped slot can be short of even the worst case)
        if (status[i] != MS_H_OVERFLOW || (st.vest[i] >= c.sets[i].sum_len && !capped)) { err = c.who + ": set " + std::to_string(i) + " failed on the device (status " + std::to_string((int)status[i]) + ")"; return -1; }
        st.vest[i] = std::min<uint64_t>(c.sets[i].sum_len, std::max<uint64_t>(2 * st.vest[i], 2 * (uint64_t)vseen[i] + 64));
        next.push_back(i);
        st.retried++;
    }
    st.todo.swap(next);
    return 0;
}

// the MSA text: the rows' places (set i = rows x n_cols bytes, row-major) and the work list of k_msa_rows
int plan_msa(const ModesCall& c, const std::vector<uint32_t>& ncols, const std::vector<uint32_t>& len, const std::vector<uint64_t>& out_cns_off, MsaPlan& p, std::string& err) {
    const PoaModesArgs& a = *c.a;
    const uint32_t ns = c.ns, nl = c.nl;
    p = MsaPlan();
    p.msa_rows.assign(ns, 0);
    p.msa_off.assign((size_t)ns + 1, 0);
    for (uint32_t i = 0; i < ns; i++) {
        const uint32_t nc = ncols[i];
        uint64_t dst = p.msa_off[i];
        if (nc) {   // (no column: no non-empty sequence, nothing to write)
            for (uint64_t k = a.set_off[i]; k < a.set_off[i + 1]; k++, dst += nc) { const uint32_t L = (uint32_t)(a.seq_off[k + 1] - a.seq_off[k]); p.rows.add(MsaRow{a.seq_off[k], dst, L, nc, 0}, L); }
            if (a.include_consensus)
                for (size_t j = (size_t)i * nl; j < (size_t)(i + 1) * nl; j++, dst += nc) p.rows.add(MsaRow{c.cns_off[j], dst, len[j], nc, 1}, len[j]);   // (a label without a consensus: a row of gaps)
        }
        p.msa_rows[i] = c.sets[i].nseq + (a.include_consensus ? nl : 0u);
        p.msa_off[i + 1] = p.msa_off[i] + (uint64_t)p.msa_rows[i] * nc;
    }
    if (p.rows.too_many()) { err = c.who + ": too many rows"; return -1; }
    p.out_bytes = p.msa_off[ns];
    p.moved_bytes = p.out_bytes + 4 * (c.nb + (a.include_consensus ? out_cns_off.back() : 0));
    return 0;
}

// coverage and profile: one counter per column (four with the profile: one per letter) for the whole call, filled from the bases of the
// sequences of >= 2 bases (k_cov_hist), then read at the columns of the consensus bases (k_cov_gather)
int plan_coverage(const ModesCall& c, const std::vector<uint32_t>& ncols, const std::vector<uint32_t>& len, const std::vector<uint64_t>& out_cns_off, CovPlan& p, std::string& err) {
    const PoaModesArgs& a = *c.a;
    p = CovPlan();
    p.stride = a.want_profile ? 4u : 1u;
    uint64_t hoff = 0, hist_bases = 0;
    const uint32_t nl = c.nl;
    for (uint32_t i = 0; i < c.ns; i++) {
        for (uint64_t k = a.set_off[i]; k < a.set_off[i + 1]; k++) {
            const uint32_t L = (uint32_t)(a.seq_off[k + 1] - a.seq_off[k]);
            if (L < 2) continue;   // (spoa counts the sequence labels of a node's edges: a sequence of one base has none)
            const uint32_t g = c.labels ? c.lab[k] : 0u;
            if (g >= nl) continue;   // (a labelled call: the sequence has no label)
            p.seqs.add(CovRow{a.seq_off[k], 0, hoff + (uint64_t)g * ncols[i], L, ncols[i]}, L);
            hist_bases += L;
        }
        for (uint32_t g = 0; g < nl; g++) {
            const size_t j = (size_t)i * nl + g;
            if (len[j]) p.cnss.add(CovRow{c.cns_off[j], out_cns_off[j], hoff + (uint64_t)g * ncols[i], len[j], ncols[i]}, len[j]);
        }
        hoff += (uint64_t)nl * ncols[i];
    }
    if (p.seqs.too_many() || p.cnss.too_many()) { err = c.who + ": too many sequences"; return -1; }
    const uint64_t nc = out_cns_off.back(), stride = p.stride;
    p.nc = nc; p.hist_words = hoff * stride;
    // what the two kernels and the clearing of the counters must move: a column (and a letter) read per counted base, the
    // counters written twice and read once where a consensus base stands, a column read and the counts written per consensus base
    p.moved_bytes = hist_bases * (4 + (stride == 4 ? 1 : 0)) + 2 * hoff * stride * 4 + nc * (4 + 4 * stride + 4 + (a.want_profile ? 16 : 0));
    return 0;
}

// the graph and the alignments: the dense places of every set's nodes, edges, consensus nodes and pairs, and the work list of k_graph_gather
int plan_graph_out(const ModesCall& c, const ModesState& st, const std::vector<uint32_t>& nv, const std::vector<uint32_t>& ne, const std::vector<uint32_t>& cnt, const std::vector<uint32_t>& len,
                   const std::vector<uint64_t>& out_cns_off, GraphPlan& p, std::string& err) {
    const PoaModesArgs& a = *c.a;
    const uint32_t ns = c.ns;
    p = GraphPlan();
    p.node_off.assign((size_t)ns + 1, 0); p.edge_off.assign((size_t)ns + 1, 0); p.aln_off.assign((size_t)c.nseq + 1, 0);
    for (uint32_t i = 0; i < ns; i++) {
        const uint64_t b0 = a.seq_off[a.set_off[i]];
        p.node_off[i + 1] = p.node_off[i] + nv[i]; p.edge_off[i + 1] = p.edge_off[i] + ne[i];
        if (nv[i]) p.rows.add(GraphRow{b0, p.node_off[i], nv[i], ROW_NODES, 0}, nv[i]);
        if (ne[i]) p.rows.add(GraphRow{b0 + a.set_off[i], p.edge_off[i], ne[i], ROW_EDGES, 0}, ne[i]);
        if (len[i]) p.rows.add(GraphRow{c.cns_off[i], out_cns_off[i], len[i], ROW_CNS, 0}, len[i]);
        uint64_t at = c.sets[i].sum_len ? st.aln_at[i] : 0;
        for (uint64_t k = a.set_off[i]; k < a.set_off[i + 1]; k++) {
            p.aln_off[k + 1] = p.aln_off[k] + cnt[k];
            if (cnt[k]) p.rows.add(GraphRow{at, p.aln_off[k], cnt[k], ROW_ALN, st.pool_of[i]}, cnt[k]);
            at += cnt[k];
        }
        if (c.sets[i].sum_len && at - st.aln_at[i] > st.aln_room[i]) { err = c.who + ": internal error (the alignments of set " + std::to_string(i) + " outgrew their share of the pool)"; return -1; }
    }
    if (p.rows.too_many()) { err = c.who + ": too many sequences"; return -1; }
    p.NV = p.node_off[ns]; p.NE = p.edge_off[ns]; p.NC = out_cns_off[ns]; p.NP = p.aln_off[c.nseq];
    p.moved_bytes = 2 * (9 * p.NV + 12 * p.NE + 4 * p.NC + 8 * p.NP);   // every element read once and written once
    return 0;
}

}  // namespace hxk
