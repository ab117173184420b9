#!/usr/bin/env python3
"""Throughput of the general POA path (hx_poa_sequences_mode and hx_poa_sequences_affine, kernels/poa_modes.hip) on two seeded workloads,
in one process:
  (a) noisy copies: 8-40 copies of 200-4 000-base templates (8 % insertions, 3 % deletions, 2 % substitutions), run as kSW with random
      0-300-base flanks on both sides of every copy, and as kNW / kOV without them
  (b) tiled fragments: 20 fragments of 1-3 kb drawn at random from 5 kb templates (same error model), kOV
For every mode: sets, cells (sum of V x L, the full matrices spoa computes), kernel time (hipEvents; warmed up, median and spread of
--repeats runs), GCUPS; for context the tuned kNW path on the same sets, and the CPU restatement (tests/poa_modes_ref.cpp) on 16 threads over
a sample of the sets (GCUPS of the sample). Every row also runs the affine kernel on the same sets (hx_poa_sequences_affine with
--affine-scores, default 5 -4 -8 -6): same figures, the affine / linear ratio of the median kernel times, and the sample compared with the
affine restatement (tests/poa_affine_ref.cpp). And every row asks for the multiple sequence alignment of the same sets (hx_poa_msa, linear
scores, with the consensus row): kernel time against the consensus-only general path ("over_general": ratio of the medians, and the
smallest and largest ratio the repeats allow), the kernel that writes the row text on its own (time by device events, the bytes it has to
move = text + 4 per base read, GB/s), and the sample compared with the MSA restatement (tests/poa_msa_ref.cpp). And every row runs the
weighted entry on the same sets (hx_poa_weighted, linear scores, seeded quality-like weights in 1..60, with coverage and profile): kernel
time against the consensus-only general path ("over_general", as for the MSA), the coverage kernels on their own (time by device events,
the bytes they have to move, GB/s), and the sample compared with the weighted restatement (tests/poa_weighted_ref.cpp). Prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def text(a):
    return ACGT[a].tobytes().decode()


def noisy(rng, t):
    """PacBio-like copy: 3 % deletions, 2 % substitutions, 8 % insertions (a random base after the position)"""
    n = len(t)
    u = rng.random(n)
    base = np.where((u >= 0.03) & (u < 0.05), rng.integers(0, 4, n), t)
    ins = rng.random(n) < 0.08
    cnt = (u >= 0.03).astype(np.int64) + ins
    out = np.repeat(base, cnt)
    pos = np.cumsum(cnt)[ins & (cnt == 2)] - 1
    out[pos] = rng.integers(0, 4, len(pos))
    return out


def workload_a(rng, n_sets, flanks):
    sets = []
    for _ in range(n_sets):
        t = rng.integers(0, 4, int(rng.integers(200, 4001)))
        st = []
        for _ in range(int(rng.integers(8, 41))):
            c = noisy(rng, t)
            if flanks:
                c = np.concatenate([rng.integers(0, 4, int(rng.integers(0, 301))), c, rng.integers(0, 4, int(rng.integers(0, 301)))])
            st.append(text(c))
        sets.append(st)
    return sets


def workload_b(rng, n_sets):
    sets = []
    for _ in range(n_sets):
        t = rng.integers(0, 4, 5000)
        st = []
        for _ in range(20):
            L = int(rng.integers(1000, 3001))
            b = int(rng.integers(0, 5000 - L + 1))
            st.append(text(noisy(rng, t[b:b + L])))
        sets.append(st)
    return sets


def gpu_time(ctx, fn, repeats):
    fn()   # warm-up (workspace allocation, code objects)
    ms = []
    for _ in range(repeats):
        ctx.timing_reset()
        fn()
        ms.append(ctx.timing()["poa"]["ms"])
    return ms


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sets-a", type=int, default=256)
    ap.add_argument("--sets-b", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cpu-sample", type=int, default=32, help="sets of each workload the CPU restatement runs (16 threads)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--affine-scores", type=int, nargs=4, default=[5, -4, -8, -6], metavar=("M", "N", "G", "E"), help="match, mismatch, gap open, gap extend of the affine rows")
    a = ap.parse_args()
    from haslr_amd import hip
    import msalib
    import parlib
    import pmrlib
    import wgtlib
    rng = np.random.default_rng(a.seed)
    loads = {"a_sw": ("sw", workload_a(rng, a.sets_a, True)), "a_nw": ("nw", workload_a(rng, a.sets_a, False))}
    loads["a_ov"] = ("ov", loads["a_nw"][1])
    loads["b_ov"] = ("ov", workload_b(rng, a.sets_b))
    ctx = hip.HipContext(0)
    res = {"tool": "poa_modes_bench", "seed": a.seed, "repeats": a.repeats, "affine_scores": list(a.affine_scores)}
    with tempfile.TemporaryDirectory() as d:
        ref = pmrlib.ModesRef(d)
        aref = parlib.AffineRef(d)
        mref = msalib.MsaRef(d)
        wref = wgtlib.WeightedRef(d)
        wrng = np.random.default_rng(a.seed + 1000)   # (a generator of its own: the workloads are those of the earlier lines)
        for name, (mode, sets) in loads.items():
            r = {"mode": mode, "sets": len(sets)}
            for path, opts in (("general", {"poa_general": 1}), ("tuned_nw", {})):
                if path == "tuned_nw" and mode != "nw":
                    continue
                with ctx.options(**opts):
                    cells = ctx.poa_sequences_mode(sets, mode, stats=True)[1]["dp_cells"]
                    ms = gpu_time(ctx, lambda: ctx.poa_sequences_mode(sets, mode), a.repeats)
                med = float(np.median(ms))
                r[path] = {"cells": int(cells), "kernel_ms_median": round(med, 2), "kernel_ms_min": round(min(ms), 2), "kernel_ms_max": round(max(ms), 2),
                           "gcups": round(cells / med / 1e6, 2)}
            sample = sets[:a.cpu_sample]
            t0 = time.perf_counter()
            with ThreadPoolExecutor(16) as ex:
                out = list(ex.map(lambda st: ref.consensus_cells(st, mode), sample))
            dt = time.perf_counter() - t0
            sc = sum(c for _, c in out)
            r["cpu_restatement_16t"] = {"sets": len(sample), "cells": int(sc), "s": round(dt, 2), "gcups": round(sc / dt / 1e9, 3)}
            got = ctx.poa_sequences_mode(sample, mode)
            r["sample_equal"] = got == [c for c, _ in out]
            cells = ctx.poa_sequences_affine(sets, mode, *a.affine_scores, stats=True)[1]["dp_cells"]
            ms = gpu_time(ctx, lambda: ctx.poa_sequences_affine(sets, mode, *a.affine_scores), a.repeats)
            med = float(np.median(ms))
            r["affine"] = {"cells": int(cells), "kernel_ms_median": round(med, 2), "kernel_ms_min": round(min(ms), 2), "kernel_ms_max": round(max(ms), 2),
                           "gcups": round(cells / med / 1e6, 2), "over_linear": round(med / r["general"]["kernel_ms_median"], 3)}
            with ThreadPoolExecutor(16) as ex:
                out = list(ex.map(lambda st: aref.consensus(st, mode, *a.affine_scores), sample))
            r["affine_sample_equal"] = ctx.poa_sequences_affine(sample, mode, *a.affine_scores) == out
            rows_ms, moved = [], 0

            def msa_call():
                nonlocal moved
                st = ctx.poa_msa(sets, mode, include_consensus=True, stats=True)[2]
                rows_ms.append(st["rows_kernel_ms"])
                moved = st["rows_kernel_bytes"]
            ms = gpu_time(ctx, msa_call, a.repeats)
            med, gen = float(np.median(ms)), r["general"]
            rmed = float(np.median(rows_ms[1:]))
            r["msa"] = {"kernel_ms_median": round(med, 2), "kernel_ms_min": round(min(ms), 2), "kernel_ms_max": round(max(ms), 2),
                        "over_general": round(med / gen["kernel_ms_median"], 4), "over_general_min": round(min(ms) / gen["kernel_ms_max"], 4),
                        "over_general_max": round(max(ms) / gen["kernel_ms_min"], 4),
                        "rows_kernel": {"ms_median": round(rmed, 4), "ms_min": round(min(rows_ms[1:]), 4), "ms_max": round(max(rows_ms[1:]), 4),
                                        "bytes": int(moved), "gb_per_s": round(moved / rmed / 1e6, 1)}}
            with ThreadPoolExecutor(16) as ex:
                out = list(ex.map(lambda st: mref.rows(st, mode, include_consensus=True), sample))
            r["msa_sample_equal"] = ctx.poa_msa(sample, mode, include_consensus=True) == out
            wts = [[wrng.integers(1, 61, len(q), dtype=np.uint8) for q in st] for st in sets]
            cov_ms, moved = [], 0

            def weighted_call():
                nonlocal moved
                st = ctx.poa_weighted(sets, wts, type=mode, coverage=True, profile=True, stats=True)[3]
                cov_ms.append(st["cov_kernel_ms"])
                moved = st["cov_kernel_bytes"]
            ms = gpu_time(ctx, weighted_call, a.repeats)
            med = float(np.median(ms))
            cmed = float(np.median(cov_ms[1:]))
            r["weighted"] = {"kernel_ms_median": round(med, 2), "kernel_ms_min": round(min(ms), 2), "kernel_ms_max": round(max(ms), 2),
                             "over_general": round(med / gen["kernel_ms_median"], 4), "over_general_min": round(min(ms) / gen["kernel_ms_max"], 4),
                             "over_general_max": round(max(ms) / gen["kernel_ms_min"], 4),
                             "coverage_kernels": {"ms_median": round(cmed, 4), "ms_min": round(min(cov_ms[1:]), 4), "ms_max": round(max(cov_ms[1:]), 4),
                                                  "bytes": int(moved), "gb_per_s": round(moved / cmed / 1e6, 1)}}
            swts = [[w.tolist() for w in ws] for ws in wts[:a.cpu_sample]]
            with ThreadPoolExecutor(16) as ex:
                out = list(ex.map(lambda k: wref.weighted(sample[k], swts[k], mode), range(len(sample))))
            got = ctx.poa_weighted(sample, swts, type=mode, coverage=True, profile=True)
            r["weighted_sample_equal"] = list(zip(*got)) == [(w.consensus, w.coverage, w.profile) for w in out]
            r["weighted_sample_changed"] = sum(c != u for c, u in zip(got[0], ctx.poa_weighted(sample, type=mode)))
            res[name] = r
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
