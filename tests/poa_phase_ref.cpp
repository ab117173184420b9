// poa_phase_ref.cpp — CPU restatement of two-haplotype consensus with read phasing on the general POA path, as DESIGN.md "General POA
// path" states it under "Two-haplotype consensus". The graph, the paths and the MSA columns of a set are built exactly as the label
// restatement (tests/poa_label_ref.cpp, included here as that file includes the convex one) builds them; the phasing rules are restated
// literally on a dense sequences x columns table of alleles (0..3 a letter, 4 a gap inside the span, -1 outside the span), and the output
// per haplotype is plr_labelled's own for n_labels = 2 with labels = hap. The tests compile this file with g++ and load it through ctypes
// (tests/phaselib.py).
//
//   phr_phased(seqs, weights, n, sc, model, type, include_consensus, min_count, min_pct)
//                  Text, one item per line: "n_haps rounds n_sites"; the haplotype of every sequence (0, 1, 255); per site four numbers
//                  (column, a1, a2, phase); then plr_labelled's text for the two labels
//   phr_free(p)    frees it
#include "poa_label_ref.cpp"

namespace {

constexpr int PHASE_ROUNDS = 8;
constexpr uint8_t HAP_NONE = 255;

struct Site { uint32_t col; int a1, a2; uint32_t n2; int s; };

int sign_of(int64_t v) { return v > 0 ? 1 : v < 0 ? -1 : 0; }

}  // namespace

extern "C" char* phr_phased(const char* const* seqs, const uint8_t* const* weights, uint32_t n, const int32_t* sc6, int32_t model, int32_t type, int32_t include_consensus,
                            uint32_t min_count, uint32_t min_pct) {
    const Scores sc{sc6[0], sc6[1], sc6[2], sc6[3], sc6[4], sc6[5]};
    // the graph, the path of every sequence and the columns: as plr_labelled has them (weights change no path and no column)
    Graph G;
    uint64_t cells = 0;
    std::vector<std::vector<uint32_t>> paths(n);
    std::vector<std::vector<uint8_t>> codes(n);
    for (uint32_t k = 0; k < n; k++) {
        const size_t L = strlen(seqs[k]);
        if (L == 0) continue;
        std::vector<uint8_t>& s = codes[k];
        s.resize(L);
        for (size_t i = 0; i < L; i++) s[i] = read_code(seqs[k][i]);
        const std::vector<std::pair<int32_t, int32_t>> aln = align_model(G, s.data(), (uint32_t)L, sc, model, type, &cells);
        uint32_t n_after = 0;
        paths[k] = derive_path(G, aln, s.data(), (uint32_t)L, &n_after);
        G.add_alignment(aln, s.data(), (uint32_t)L);
        if (weights && weights[k])
            for (size_t i = 1; i < L; i++)
                for (uint32_t ed : G.outs[paths[k][i - 1]])
                    if (G.edges[ed].to == paths[k][i]) { G.edges[ed].w += (int64_t)weights[k][i - 1] + (int64_t)weights[k][i] - 2; break; }
    }
    const size_t V = G.code.size();
    std::vector<uint32_t> col(V, 0);
    uint32_t C = 0;
    for (size_t i = 0; i < V; C++) {
        const uint32_t nd = G.rank2node[i++];
        col[nd] = C;
        for (uint32_t a : G.aligned[nd]) { col[a] = C; if (i < V && G.rank2node[i] == a) i++; }
    }
    // the allele of every sequence at every column: -1 outside its span, 4 inside it without a base
    std::vector<std::vector<int>> al(n, std::vector<int>(C, -1));
    for (uint32_t k = 0; k < n; k++) {
        if (paths[k].empty()) continue;
        for (uint32_t c = col[paths[k].front()]; c <= col[paths[k].back()]; c++) al[k][c] = 4;
        for (size_t i = 0; i < paths[k].size(); i++) al[k][col[paths[k][i]]] = codes[k][i];
    }
    // 1. counts, 2. sites
    std::vector<Site> sites;
    for (uint32_t c = 0; c < C; c++) {
        uint32_t cnt[5] = {0, 0, 0, 0, 0}, d = 0;
        for (uint32_t k = 0; k < n; k++) if (al[k][c] >= 0) { cnt[al[k][c]]++; d++; }
        int order[5] = {0, 1, 2, 3, 4};
        std::stable_sort(order, order + 5, [&](int x, int y) { return cnt[x] > cnt[y]; });   // (count descending, then code ascending)
        const uint32_t n2 = cnt[order[1]];
        if (n2 >= std::max<uint32_t>(min_count, (min_pct * d + 99) / 100)) sites.push_back(Site{c, order[0], order[1], n2, 0});
    }
    std::vector<uint8_t> hap(n, HAP_NONE);
    uint32_t rounds = 0, n_haps = 1;
    if (!sites.empty()) {
        // 3. the seed: the largest minor count, the smallest column among equals
        size_t seed = 0;
        for (size_t j = 1; j < sites.size(); j++) if (sites[j].n2 > sites[seed].n2) seed = j;
        for (uint32_t k = 0; k < n; k++) {
            const int a = paths[k].empty() ? -1 : al[k][sites[seed].col];
            hap[k] = a >= 0 && a == sites[seed].a1 ? 0 : a >= 0 && a == sites[seed].a2 ? 1 : HAP_NONE;
        }
        // 4. the rounds
        for (bool changed = true; changed && rounds < PHASE_ROUNDS; rounds++) {
            changed = false;
            for (Site& s : sites) {
                int64_t m[2][5] = {{0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}};
                for (uint32_t k = 0; k < n; k++) if (hap[k] != HAP_NONE && al[k][s.col] >= 0) m[hap[k]][al[k][s.col]]++;
                s.s = sign_of((m[0][s.a1] - m[0][s.a2]) - (m[1][s.a1] - m[1][s.a2]));
            }
            std::vector<uint8_t> next(hap);
            for (uint32_t k = 0; k < n; k++) {
                if (paths[k].empty()) continue;
                int64_t S = 0;
                for (const Site& s : sites) { const int a = al[k][s.col]; if (a >= 0) S += s.s * (a == s.a1 ? 1 : a == s.a2 ? -1 : 0); }
                if (S > 0) next[k] = 0;
                if (S < 0) next[k] = 1;
                changed = changed || next[k] != hap[k];
            }
            hap.swap(next);
        }
    }
    // 5. the verdict
    uint32_t members[2] = {0, 0};
    for (uint32_t k = 0; k < n; k++) if (hap[k] != HAP_NONE) members[hap[k]]++;
    if (sites.empty() || members[0] < min_count || members[1] < min_count) {
        for (uint32_t k = 0; k < n; k++) hap[k] = paths[k].empty() ? HAP_NONE : 0;
        for (Site& s : sites) s.s = 0;
    } else {
        n_haps = 2;
        uint32_t first = 0;
        while (hap[first] == HAP_NONE) first++;
        if (hap[first] == 1) {
            for (uint32_t k = 0; k < n; k++) if (hap[k] != HAP_NONE) hap[k] ^= 1;
            for (Site& s : sites) s.s = -s.s;
        }
    }
    std::string out = std::to_string(n_haps) + " " + std::to_string(rounds) + " " + std::to_string(sites.size()) + "\n";
    for (uint32_t k = 0; k < n; k++) out += (k ? " " : "") + std::to_string(hap[k]);
    out += "\n";
    for (size_t j = 0; j < sites.size(); j++) out += (j ? " " : "") + std::to_string(sites[j].col) + " " + std::to_string(sites[j].a1) + " " + std::to_string(sites[j].a2) + " " + std::to_string(sites[j].s);
    out += "\n";
    // 6. the output: hx_poa_labelled's for two labels
    if (n == 0) hap.push_back(HAP_NONE);   // (a pointer with something behind it)
    char* lab = plr_labelled(seqs, weights, hap.data(), n, 2, sc6, model, type, include_consensus);
    out += lab;
    free(lab);
    return text(out);
}

extern "C" void phr_free(char* p) { free(p); }
