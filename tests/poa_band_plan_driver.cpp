// poa_band_plan_driver.cpp - runs a synthetic banded call of the general POA path through its plan alone (kernels/poa_modes_plan.hip compiled
// host-only: no HIP runtime in the link, no GPU) and prints what every round plans (tests/test_poa_band_plan.py).
//   poa_band_plan_driver GM BAND SLOT_KB MISSES SCORE LEN,LEN,... [LEN,LEN,...] ...
// GM: 0 linear, 1 affine, 2 convex; BAND: the half-width (0: no band); SLOT_KB: option poa_modes_slot_kb; MISSES: how many banded attempts
// of every set end in a band miss before one succeeds; SCORE: the magnitude of the gap open score; one further argument per set, the
// lengths of its sequences. A set's graph grows to its longest sequence and a sixteenth of its bases; in a slot with fewer rows it leaves MS_H_OVERFLOW.
// One line per set and round: "set I round R slot K band W pools P vest V need N"; one per slot with sets: "slot K bytes S nslots N";
// at the end per set "done I band_used W" and "reruns slot A band B", or "error TEXT".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "poa_modes_plan.h"

using namespace hxk;

int main(int argc, char** argv) {
    if (argc < 7) { fprintf(stderr, "usage: poa_band_plan_driver GM BAND SLOT_KB MISSES SCORE LEN,LEN,... ...\n"); return 2; }
    PoaModesArgs a;
    a.who = "hx_poa_banded";
    a.gap_model = atoi(argv[1]); a.band = (uint32_t)atoi(argv[2]); a.slot_kb_cap = (uint32_t)atoi(argv[3]);
    const int misses = atoi(argv[4]);
    a.match = 5; a.mismatch = -4; a.gap = -atoi(argv[5]); a.gap_extend = a.gap_model ? -6 : a.gap; a.gap_open2 = a.gap_model == 2 ? a.gap - 2 : 0; a.gap_extend2 = a.gap_model == 2 ? -4 : 0; a.type = MT_NW;
    std::vector<uint64_t> set_off{0}, seq_off{0};
    for (int k = 6; k < argc; k++) {
        for (char* tok = strtok(argv[k], ","); tok; tok = strtok(nullptr, ",")) seq_off.push_back(seq_off.back() + strtoull(tok, nullptr, 10));
        set_off.push_back(seq_off.size() - 1);
    }
    const std::string bases(seq_off.back() + 1, 'A');
    a.n_sets = (uint32_t)set_off.size() - 1; a.set_off = set_off.data(); a.seq_off = seq_off.data(); a.bases = bases.c_str();
    ModesCall c; ModesState st;
    std::string err;
    if (describe(a, c, st, err)) { printf("error %s\n", err.c_str()); return 0; }
    const uint32_t ns = c.ns;
    std::vector<int> left(ns, misses);
    std::vector<uint32_t> status(ns), vseen(ns), pairs(ns), used(ns, 0);
    for (bool first = true; !st.todo.empty(); first = false) {
        uint64_t resident[N_SLOTS];
        for (int k = 0; k < N_SLOTS; k++) resident[k] = 256;
        RoundPlan p;
        if (plan_round(c, st, first, 8ull << 30, resident, p, err)) { printf("error %s\n", err.c_str()); return 0; }
        for (int k = 0; k < N_SLOTS; k++) {
            const RoundPlan::PerInst& pk = p.inst[k];
            if (pk.sets.empty()) continue;
            printf("slot %d bytes %llu nslots %u\n", k, (unsigned long long)pk.slot, pk.nslots);
            for (uint32_t i : pk.sets) {
                const uint32_t w = c.band ? st.band[i] : 0;
                const uint64_t pools = pools_bytes(c.sets[i]), cell = CELL_BYTES[c.gm];
                const uint64_t row = w ? (2 * (uint64_t)w + 1) * cell + 12 : (uint64_t)(c.sets[i].lmax + 1) * cell;   // bytes a row of the graph takes
                const uint64_t need = pools + ((st.vest[i] + 1) * row + 255) / 256 * 256;
                printf("set %u round %u slot %d band %u pools %llu vest %llu need %llu\n", i, st.rounds - 1, k, w, (unsigned long long)pools, (unsigned long long)st.vest[i], (unsigned long long)need);
                const uint64_t rows = pk.slot > pools ? (pk.slot - pools) / row : 0;
                const uint64_t nodes = std::min<uint64_t>(c.sets[i].sum_len, c.sets[i].lmax + c.sets[i].sum_len / 16);   // what the set's graph grows to
                if (rows < nodes + 1) { status[i] = MS_H_OVERFLOW; vseen[i] = (uint32_t)(rows ? rows - 1 : 0); }
                else if (w && left[i] > 0) { status[i] = MS_BAND_MISS; left[i]--; }
                else { status[i] = MS_OK; used[i] = w; }
            }
        }
        if (after_round(c, st, first, status.data(), vseen.data(), pairs.data(), err)) { printf("error %s\n", err.c_str()); return 0; }
    }
    for (uint32_t i = 0; i < ns; i++) printf("done %u band_used %u\n", i, used[i]);
    printf("reruns slot %u band %u\n", st.retried, st.band_retried);
    return 0;
}
