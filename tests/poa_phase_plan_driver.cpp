// poa_phase_plan_driver.cpp - runs a synthetic call of the general POA path through its plan alone (kernels/poa_modes_plan.hip compiled
// host-only: no HIP runtime in the link, no GPU) as a phased call, as a labelled call with two labels, or as a weighted call, and prints
// what the plan makes of it (tests/test_poa_phase_plan.py).
//   poa_phase_plan_driver pool T NSEQ            the bytes of the phase pool of a set of T bases in NSEQ sequences
//   poa_phase_plan_driver MODE MIN_COUNT MIN_PCT LEN:LABEL,LEN:LABEL,... [LEN:LABEL,...] ...
// MODE: phase, label or weighted; one further argument per set, the length and the label (0, 1, 255) of each of its sequences. A labelled
// call is given the labels; a phased call gets them as what the device would have left (ModesCall::lab, set after the round); a weighted
// call ignores them. Every set has as many columns as its longest sequence has bases, and a label with a non-empty member a consensus of
// that length. Lines: "call labels L nl N cols C cov V"; "cns_off ..."; per slot "slot K bytes S nslots N"; per set "set I pools P";
// "cov stride S hist H nc N"; per counted sequence "cov_seq SRC HOFF LEN NCOLS"; per consensus "cov_cns SRC DST HOFF LEN NCOLS";
// per row "msa_row SRC DST LEN NCOLS IS_CNS"; "msa_rows ..."; "msa_off ..."; or "error TEXT".
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "poa_modes_plan.h"

using namespace hxk;

int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "pool")) { printf("%llu\n", (unsigned long long)phase_pool_bytes(strtoull(argv[2], nullptr, 10), (uint32_t)atoi(argv[3]))); return 0; }
    if (argc < 5) { fprintf(stderr, "usage: poa_phase_plan_driver pool T NSEQ | MODE MIN_COUNT MIN_PCT LEN:LABEL,... ...\n"); return 2; }
    const bool phase = !strcmp(argv[1], "phase"), label = !strcmp(argv[1], "label");
    PoaModesArgs a;
    a.who = phase ? "hx_poa_phased" : label ? "hx_poa_labelled" : "hx_poa_weighted";
    a.match = 5; a.mismatch = -4; a.gap = -8; a.gap_extend = -8; a.type = MT_NW;
    a.weighted = !phase && !label; a.msa = 1; a.include_consensus = 1; a.want_coverage = 1; a.want_profile = 1;
    a.phase = phase; a.phase_min_count = (uint32_t)atoi(argv[2]); a.phase_min_pct = (uint32_t)atoi(argv[3]);
    std::vector<uint64_t> set_off{0}, seq_off{0};
    std::vector<uint8_t> labels;
    for (int k = 4; k < argc; k++) {
        for (char* tok = strtok(argv[k], ","); tok; tok = strtok(nullptr, ",")) {
            char* colon = strchr(tok, ':');
            seq_off.push_back(seq_off.back() + strtoull(tok, nullptr, 10));
            labels.push_back(colon ? (uint8_t)atoi(colon + 1) : 0);
        }
        set_off.push_back(seq_off.size() - 1);
    }
    labels.push_back(255);
    const std::string bases(seq_off.back() + 1, 'A');
    a.n_sets = (uint32_t)set_off.size() - 1; a.set_off = set_off.data(); a.seq_off = seq_off.data(); a.bases = bases.c_str();
    if (label) { a.labels = labels.data(); a.n_labels = 2; }
    ModesCall c; ModesState st;
    std::string err;
    if (describe(a, c, st, err)) { printf("error %s\n", err.c_str()); return 0; }
    printf("call labels %d nl %u cols %d cov %d\n", (int)c.labels, c.nl, (int)c.cols, (int)c.want_cov);
    printf("cns_off");
    for (uint64_t v : c.cns_off) printf(" %llu", (unsigned long long)v);
    printf("\n");
    uint64_t resident[N_SLOTS];
    for (int k = 0; k < N_SLOTS; k++) resident[k] = 256;
    RoundPlan p;
    if (plan_round(c, st, true, 8ull << 30, resident, p, err)) { printf("error %s\n", err.c_str()); return 0; }
    for (int k = 0; k < N_SLOTS; k++) {
        if (p.inst[k].sets.empty()) continue;
        printf("slot %d bytes %llu nslots %u\n", k, (unsigned long long)p.inst[k].slot, p.inst[k].nslots);
        for (uint32_t i : p.inst[k].sets) printf("set %u pools %llu\n", i, (unsigned long long)slot_pools_bytes(c, i));
    }
    if (phase) c.lab = labels.data();   // (poa_modes_run: the downloaded haplotypes)
    const uint32_t ns = c.ns, nl = c.nl;
    std::vector<uint32_t> ncols(ns), len((size_t)ns * nl, 0);
    std::vector<uint64_t> out_off((size_t)ns * nl + 1, 0);
    for (uint32_t i = 0; i < ns; i++) {
        ncols[i] = c.sets[i].lmax;
        for (uint64_t k = set_off[i]; k < set_off[i + 1]; k++) {
            const uint32_t g = c.labels ? c.lab[k] : 0u;
            if (g < nl && seq_off[k + 1] > seq_off[k]) len[(size_t)i * nl + g] = c.sets[i].lmax;
        }
    }
    for (size_t j = 0; j < len.size(); j++) out_off[j + 1] = out_off[j] + len[j];
    CovPlan cp;
    if (plan_coverage(c, ncols, len, out_off, cp, err)) { printf("error %s\n", err.c_str()); return 0; }
    printf("cov stride %u hist %llu nc %llu\n", cp.stride, (unsigned long long)cp.hist_words, (unsigned long long)cp.nc);
    for (const CovRow& r : cp.seqs.rows) printf("cov_seq %llu %llu %u %u\n", (unsigned long long)r.src, (unsigned long long)r.hoff, r.len, r.ncols);
    for (const CovRow& r : cp.cnss.rows) printf("cov_cns %llu %llu %llu %u %u\n", (unsigned long long)r.src, (unsigned long long)r.dst, (unsigned long long)r.hoff, r.len, r.ncols);
    MsaPlan mp;
    if (plan_msa(c, ncols, len, out_off, mp, err)) { printf("error %s\n", err.c_str()); return 0; }
    for (const MsaRow& r : mp.rows.rows) printf("msa_row %llu %llu %u %u %u\n", (unsigned long long)r.src, (unsigned long long)r.dst, r.len, r.ncols, r.is_cns);
    printf("msa_rows");
    for (uint32_t v : mp.msa_rows) printf(" %u", v);
    printf("\nmsa_off");
    for (uint64_t v : mp.msa_off) printf(" %llu", (unsigned long long)v);
    printf("\n");
    return 0;
}
