#!/usr/bin/env python3
"""Throughput of the general POA path (hx_poa_sequences_mode and hx_poa_sequences_affine, kernels/poa_modes.hip) on two seeded workloads,
in one process:
  (a) noisy copies: 8-40 copies of 200-4 000-base templates (8 % insertions, 3 % deletions, 2 % substitutions), run as kSW with random
      0-300-base flanks on both sides of every copy, and as kNW / kOV without them
  (b) tiled fragments: 20 fragments of 1-3 kb drawn at random from 5 kb templates (same error model), kOV
For every mode: sets, cells (sum of V x L, the full matrices spoa computes), kernel time (hipEvents; warmed up, median and spread of
--repeats runs), GCUPS; for the general path, the MSA, the weighted, the graph and the strand calls also the wall time of the whole call
on the host (wall_ms_*: what the host side of the path adds shows there and nowhere in the kernel time); for context the tuned kNW path on the same sets, and the CPU restatement (tests/poa_modes_ref.cpp) on 16 threads over
a sample of the sets (GCUPS of the sample). Every row also runs the affine kernel on the same sets (hx_poa_sequences_affine with
--affine-scores, default 5 -4 -8 -6): same figures, the affine / linear ratio of the median kernel times, and the sample compared with the
affine restatement (tests/poa_affine_ref.cpp). And every row asks for the multiple sequence alignment of the same sets (hx_poa_msa, linear
scores, with the consensus row): kernel time against the consensus-only general path ("over_general": ratio of the medians, and the
smallest and largest ratio the repeats allow), the kernel that writes the row text on its own (time by device events, the bytes it has to
move = text + 4 per base read, GB/s), and the sample compared with the MSA restatement (tests/poa_msa_ref.cpp). And every row runs the
weighted entry on the same sets (hx_poa_weighted, linear scores, seeded quality-like weights in 1..60, with coverage and profile): kernel
time against the consensus-only general path ("over_general", as for the MSA), the coverage kernels on their own (time by device events,
the bytes they have to move, GB/s), and the sample compared with the weighted restatement (tests/poa_weighted_ref.cpp). And every row runs
the convex kernel on the same sets (hx_poa_sequences_convex with --convex-scores, default 5 -4 -8 -6 -10 -4): same figures, the convex /
affine and convex / linear ratios of the median kernel times with the smallest and largest ratio the repeats allow, and every sampled set
compared with the convex restatement (tests/poa_convex_ref.cpp). And rows (a) and (b) ask for the graph and the alignments of the same sets
(hx_poa_graph, linear scores, unit weights; part "graph", which needs general and outputs): kernel time against the MSA's in the same
process ("over_msa") and against the consensus-only general path, the gather kernel on its own (time by device events, the bytes it has to
move, GB/s), the sets that were rerun because their alignments outgrew their share of the alignment pool under the default estimate, and
the sample compared with the graph restatement (tests/poa_graph_ref.cpp). And the rows of workload (a) run the strand-ambiguous entry (hx_poa_strand,
linear scores, unit weights, with the rows and the consensus row; part "strand", which needs general and outputs) on the same sets with
every member after the first reverse-complemented with probability 1/2: kernel time against the MSA's on the sets as they are, which is
the same call on the sets oriented beforehand ("over_msa", with the smallest and largest ratio the repeats allow), the sequences whose
reverse complement won and with them the ratio the DP passes alone predict (2 + third_passes / aligned sequences), and a sample compared
with the strand restatement (tests/poa_strand_ref.cpp). --band W [W ...] is a mode of its own: workload (a) under kNW and kOV, linear
scores, consensus only, through the banded entry (hx_poa_banded) at every half-width W against the full-matrix general path on the same
sets in the same process: kernel time by the same protocol, the workspace the call left allocated on the device (free memory before and
after, the workspace released in between; the banded call also reports the plan's own figure), the share of sets that did not finish at
W (band_used != W: they climbed to a wider band or to the full matrix), the reruns that cost, and the share of sets whose banded consensus
is the full-matrix one. A package without the banded entry (--package-root of a parent checkout) gives the full-matrix figures alone.
--phase is a mode of its own over the workload of --labels: hx_poa_phased beside hx_poa_labelled at n_labels = 2 with the true haplotypes
as labels, on the same sets in the same session; the ratio of the kernel times is what the phasing costs, and the share of the reads that
land on their true haplotype is reported as a measurement.

--labels is another mode of its own: a two-haplotype workload (per set a template and a copy of it with SNPs and one indel, noisy reads of
each) under kNW, affine scores, through hx_poa_labelled at n_labels = 1, 2 and 16 beside hx_poa_weighted on the same sets in the same
build: kernel time of each and the ratio over the weighted call, which is what the label passes cost on top of the DP.
--rows picks the rows, --only picks the parts to run; --package-root runs the parts another
build of the package has (a checkout of the parent commit, say) in the same way, for a comparison on one machine. Prints one JSON line,
and writes it to --out when given."""
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
PARTS = ["general", "tuned_nw", "cpu", "affine", "outputs", "convex", "graph", "strand"]   # outputs: the MSA and the weighted entry


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


def note(*what):
    """progress on stderr: a row takes minutes, and stdout carries the one JSON line"""
    print("[poa_modes_bench]", *what, file=sys.stderr, flush=True)


def gpu_time(ctx, fn, repeats):
    """kernel time (device events) and wall time of the whole call on the host, per repeat"""
    fn()   # warm-up (workspace allocation, code objects)
    ms, wall = [], []
    for _ in range(repeats):
        ctx.timing_reset()
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(ctx.timing()["poa"]["ms"])
    return ms, wall


def wall_stats(wall):
    return {"wall_ms_median": round(float(np.median(wall)), 2), "wall_ms_min": round(min(wall), 2), "wall_ms_max": round(max(wall), 2)}


def device_free_bytes():
    import ctypes
    free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
    if ctypes.CDLL("libamdhip64.so").hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) != 0:
        raise RuntimeError("hipMemGetInfo failed")
    return free.value


def band_mode(a, hip):
    rng = np.random.default_rng(a.seed)
    workload_a(rng, a.sets_a, True)   # (the kSW sets come first in the generator's sequence: the kNW / kOV sets are those of the other rows)
    sets = workload_a(rng, a.sets_a, False)
    ctx = hip.HipContext(0)
    has_band = hasattr(hip.HipContext, "poa_banded")
    res = {"tool": "poa_modes_bench", "mode": "band", "seed": a.seed, "repeats": a.repeats, "sets": len(sets), "bands": list(a.band) if has_band else [],
           "longest_sequence": max(len(q) for st in sets for q in st), "bases": sum(len(q) for st in sets for q in st)}

    def timed(fn):
        ctx.poa_release_workspace()
        before = device_free_bytes()
        ms, wall = gpu_time(ctx, fn, a.repeats)
        held = before - device_free_bytes()
        med = float(np.median(ms))
        out = {"kernel_ms_median": round(med, 2), "kernel_ms_min": round(min(ms), 2), "kernel_ms_max": round(max(ms), 2), "workspace_bytes_held": int(held)}
        out.update(wall_stats(wall))
        return out
    for mode in ("nw", "ov"):
        r = {}
        with ctx.options(poa_general=1):
            full_cns, st = ctx.poa_sequences_mode(sets, mode, stats=True)
            r["full"] = timed(lambda: ctx.poa_sequences_mode(sets, mode))
        r["full"].update({"cells": int(st["dp_cells"]), "gcups": round(st["dp_cells"] / r["full"]["kernel_ms_median"] / 1e6, 2)})
        note("band", mode, "full", r["full"]["kernel_ms_median"], "ms")
        for w in (a.band if has_band else []):
            recs, st = ctx.poa_banded(sets, w, type=mode, stats=True)
            b = timed(lambda: ctx.poa_banded(sets, w, type=mode))
            other = sum(rec.band_used != w for rec in recs)
            b.update({"cells": int(st["dp_cells"]), "workspace_bytes_planned": int(st["workspace_bytes"]), "band_reruns": int(st["band_reruns"]), "slot_reruns": int(st["slot_reruns"]),
                      "sets_not_at_w": int(other), "share_not_at_w": round(other / len(sets), 4), "sets_on_full_matrix": int(sum(rec.band_used == 0 for rec in recs)),
                      "share_consensus_equal_full": round(sum(rec.consensus == c for rec, c in zip(recs, full_cns)) / len(sets), 4),
                      "over_full": round(b["kernel_ms_median"] / r["full"]["kernel_ms_median"], 4), "over_full_min": round(b["kernel_ms_min"] / r["full"]["kernel_ms_max"], 4),
                      "over_full_max": round(b["kernel_ms_max"] / r["full"]["kernel_ms_min"], 4),
                      "workspace_over_full": round(b["workspace_bytes_held"] / max(1, r["full"]["workspace_bytes_held"]), 4)})
            r["band_%d" % w] = b
            note("band", mode, w, b["kernel_ms_median"], "ms")
        res["a_" + mode] = r
    ctx.close()
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res) + "\n")


def workload_haplotypes(rng, n_sets):
    """per set: a template of 200..4000 bases, a second haplotype of it (one SNP per 200 bases, at least three, and one indel of 1..8
    bases), and 4..20 noisy reads of each, the haplotypes interleaved. Returns (sets, per set the haplotype of every read)"""
    sets, haps = [], []
    for _ in range(n_sets):
        t = rng.integers(0, 4, int(rng.integers(200, 4001)))
        h = t.copy()
        for p in rng.choice(len(t), max(3, len(t) // 200), replace=False):
            h[p] = (h[p] + int(rng.integers(1, 4))) % 4
        p, k = int(rng.integers(10, len(t) - 10)), int(rng.integers(1, 9))
        h = np.concatenate([h[:p], h[p + k:]]) if rng.random() < 0.5 else np.concatenate([h[:p], rng.integers(0, 4, k), h[p:]])
        n = int(rng.integers(4, 21))
        sets.append([text(noisy(rng, (t, h)[i % 2])) for i in range(2 * n)])
        haps.append([i % 2 for i in range(2 * n)])
    return sets, haps


def labels_mode(a, hip):
    rng = np.random.default_rng(a.seed)
    sets, haps = workload_haplotypes(rng, a.sets_a)
    m, n, g, e = a.affine_scores
    kw = dict(type="nw", match=m, mismatch=n, gap_open=g, gap_extend=e)
    ctx = hip.HipContext(0)
    res = {"tool": "poa_modes_bench", "mode": "labels", "seed": a.seed, "repeats": a.repeats, "sets": len(sets), "scores": [m, n, g, e],
           "longest_sequence": max(len(q) for st in sets for q in st), "bases": sum(len(q) for st in sets for q in st)}

    def timed(fn):
        ms, wall = gpu_time(ctx, fn, a.repeats)
        out = {"kernel_ms_median": round(float(np.median(ms)), 2), "kernel_ms_min": round(min(ms), 2), "kernel_ms_max": round(max(ms), 2)}
        out.update(wall_stats(wall))
        return out
    with ctx.options(poa_weighted=1):   # (the weighted kernels, as the label instances are: weights of 1)
        wcns, st = ctx.poa_weighted(sets, stats=True, **kw)
        res["weighted"] = timed(lambda: ctx.poa_weighted(sets, **kw))
    res["weighted"]["cells"] = int(st["dp_cells"])
    note("labels", "weighted", res["weighted"]["kernel_ms_median"], "ms")
    if hasattr(hip.HipContext, "poa_labelled"):
        for nl in (1, 2, 16):
            labels = [[0 if nl == 1 else hp if nl == 2 else hp * 8 + (i // 2) % 8 for i, hp in enumerate(hs)] for hs in haps]
            recs, st = ctx.poa_labelled(sets, labels, nl, stats=True, **kw)
            r = timed(lambda: ctx.poa_labelled(sets, labels, nl, **kw))
            w = res["weighted"]
            r.update({"cells": int(st["dp_cells"]), "slot_reruns": int(st["slot_reruns"]), "over_weighted": round(r["kernel_ms_median"] / w["kernel_ms_median"], 4),
                      "over_weighted_min": round(r["kernel_ms_min"] / w["kernel_ms_max"], 4), "over_weighted_max": round(r["kernel_ms_max"] / w["kernel_ms_min"], 4),
                      "consensus_bases": int(sum(len(c) for rec in recs for c in rec.consensus))})
            if nl == 1:
                r["share_consensus_equal_weighted"] = round(sum(rec.consensus[0] == c for rec, c in zip(recs, wcns)) / len(sets), 4)
            if nl == 2:
                r["share_sets_with_two_consensuses"] = round(sum(rec.consensus[0] != rec.consensus[1] for rec in recs) / len(sets), 4)
            res["labels_%d" % nl] = r
            note("labels", nl, r["kernel_ms_median"], "ms")
    ctx.close()
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res) + "\n")


def phase_mode(a, hip):
    """the two-haplotype workload of --labels through hx_poa_phased and, on the same sets in the same session, through hx_poa_labelled
    with n_labels = 2 and the true haplotypes as labels: the ratio of the kernel times is what the phasing costs"""
    rng = np.random.default_rng(a.seed)
    sets, haps = workload_haplotypes(rng, a.sets_a)
    m, n, g, e = a.affine_scores
    kw = dict(type="nw", match=m, mismatch=n, gap_open=g, gap_extend=e)
    ctx = hip.HipContext(0)
    res = {"tool": "poa_modes_bench", "mode": "phase", "seed": a.seed, "repeats": a.repeats, "sets": len(sets), "scores": [m, n, g, e],
           "longest_sequence": max(len(q) for st in sets for q in st), "bases": sum(len(q) for st in sets for q in st)}

    def one(fn):
        ctx.timing_reset()
        t0 = time.perf_counter()
        fn()
        return ctx.timing()["poa"]["ms"], (time.perf_counter() - t0) * 1e3

    def stats_of(runs):
        ms = [m for m, _ in runs]
        out = {"kernel_ms_median": round(float(np.median(ms)), 2), "kernel_ms_min": round(min(ms), 2), "kernel_ms_max": round(max(ms), 2)}
        out.update(wall_stats([w for _, w in runs]))
        return out
    # the first call of each is its warm-up (workspace, code objects); then the two calls take turns, so that neither has the later, warmer half of the session to itself
    lrecs, lst = ctx.poa_labelled(sets, haps, 2, stats=True, **kw)
    recs, st = ctx.poa_phased(sets, stats=True, **kw)
    lruns, pruns = [], []
    for _ in range(a.repeats):
        lruns.append(one(lambda: ctx.poa_labelled(sets, haps, 2, **kw)))
        pruns.append(one(lambda: ctx.poa_phased(sets, **kw)))
    lab = stats_of(lruns)
    lab["cells"] = int(lst["dp_cells"])
    res["labelled_2"] = lab
    note("phase", "labelled", lab["kernel_ms_median"], "ms")
    r = stats_of(pruns)
    r["over_labelled_by_turn"] = [round(p[0] / q[0], 4) for p, q in zip(pruns, lruns)]
    same = sum(rec.hap in (hs, [1 - h for h in hs]) for rec, hs in zip(recs, haps))
    reads = sum(len(hs) for hs in haps)
    agree = sum(max(sum(x == y for x, y in zip(rec.hap, hs)), sum(x == 1 - y for x, y in zip(rec.hap, hs))) for rec, hs in zip(recs, haps))
    r.update({"cells": int(st["dp_cells"]), "slot_reruns": int(st["slot_reruns"]), "over_labelled": round(r["kernel_ms_median"] / lab["kernel_ms_median"], 4),
              "over_labelled_min": round(r["kernel_ms_min"] / lab["kernel_ms_max"], 4), "over_labelled_max": round(r["kernel_ms_max"] / lab["kernel_ms_min"], 4),
              "ranges_overlap": bool(r["kernel_ms_min"] <= lab["kernel_ms_max"] and lab["kernel_ms_min"] <= r["kernel_ms_max"]),
              "sets_phased": int(sum(rec.n_haps == 2 for rec in recs)), "sites": int(sum(len(rec.sites) for rec in recs)), "rounds_max": int(max(rec.rounds for rec in recs)),
              "share_sets_with_the_true_haplotypes": round(same / len(sets), 4), "share_reads_on_their_true_haplotype": round(agree / reads, 4),
              "share_sets_with_the_labelled_consensus": round(sum(rec.consensus in (lr.consensus, lr.consensus[::-1]) for rec, lr in zip(recs, lrecs)) / len(sets), 4)})
    res["phased"] = r
    note("phase", "phased", r["kernel_ms_median"], "ms")
    ctx.close()
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sets-a", type=int, default=256)
    ap.add_argument("--sets-b", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cpu-sample", type=int, default=32, help="sets of each workload the CPU restatement runs (16 threads)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--affine-scores", type=int, nargs=4, default=[5, -4, -8, -6], metavar=("M", "N", "G", "E"), help="match, mismatch, gap open, gap extend of the affine rows")
    ap.add_argument("--convex-scores", type=int, nargs=6, default=[5, -4, -8, -6, -10, -4], metavar=("M", "N", "G", "E", "Q", "C"), help="match, mismatch and the two gap pieces of the convex rows")
    ap.add_argument("--only", nargs="+", default=PARTS, choices=PARTS, help="the parts of every row to run (outputs: the MSA and the weighted entry, which need general; ratios are given against the parts that ran)")
    ap.add_argument("--rows", nargs="+", default=["a_sw", "a_nw", "a_ov", "b_ov"], choices=["a_sw", "a_nw", "a_ov", "b_ov"], help="the rows to run")
    ap.add_argument("--package-root", default=ROOT, help="the tree whose built haslr_amd package runs (default: this one); parts it does not have are left out")
    ap.add_argument("--band", type=int, nargs="+", metavar="W", help="the band mode: workload (a) under kNW and kOV through hx_poa_banded at these half-widths, against the full-matrix general path")
    ap.add_argument("--labels", action="store_true", help="the label mode: the two-haplotype workload through hx_poa_labelled at n_labels = 1, 2 and 16, against hx_poa_weighted on the same sets")
    ap.add_argument("--phase", action="store_true", help="the phase mode: the two-haplotype workload through hx_poa_phased, against hx_poa_labelled with n_labels = 2 and the true haplotypes on the same sets")
    ap.add_argument("--out", help="also write the JSON line to this file")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))
    from haslr_amd import hip
    if a.band:
        return band_mode(a, hip)
    if a.labels:
        return labels_mode(a, hip)
    if a.phase:
        return phase_mode(a, hip)
    import cvxlib
    import msalib
    import parlib
    import pmrlib
    import wgtlib
    only = set(a.only)
    if not hasattr(hip.HipContext, "poa_sequences_convex"):
        only.discard("convex")
    if not hasattr(hip.HipContext, "poa_graph"):
        only.discard("graph")
    if not hasattr(hip.HipContext, "poa_strand"):
        only.discard("strand")
    rng = np.random.default_rng(a.seed)
    loads = {"a_sw": ("sw", workload_a(rng, a.sets_a, True)), "a_nw": ("nw", workload_a(rng, a.sets_a, False))}
    loads["a_ov"] = ("ov", loads["a_nw"][1])
    loads["b_ov"] = ("ov", workload_b(rng, a.sets_b))
    ctx = hip.HipContext(0)
    res = {"tool": "poa_modes_bench", "seed": a.seed, "repeats": a.repeats, "affine_scores": list(a.affine_scores), "convex_scores": list(a.convex_scores), "parts": [p for p in PARTS if p in only]}
    with tempfile.TemporaryDirectory() as d:
        ref = pmrlib.ModesRef(d)
        aref = parlib.AffineRef(d)
        mref = msalib.MsaRef(d)
        wref = wgtlib.WeightedRef(d)
        cref = cvxlib.ConvexRef(d)
        wrng = np.random.default_rng(a.seed + 1000)   # (a generator of its own: the workloads are those of the earlier lines)
        for name, (mode, sets) in loads.items():
            if name not in a.rows:
                continue
            r = {"mode": mode, "sets": len(sets)}
            note(name, "sets", len(sets))
            for path, opts in (("general", {"poa_general": 1}), ("tuned_nw", {})):
                if (path == "tuned_nw" and mode != "nw") or path not in only:
                    continue
                with ctx.options(**opts):
                    cells = ctx.poa_sequences_mode(sets, mode, stats=True)[1]["dp_cells"]
                    ms, wall = gpu_time(ctx, lambda: ctx.poa_sequences_mode(sets, mode), a.repeats)
                med = float(np.median(ms))
                r[path] = {"cells": int(cells), "kernel_ms_median": round(med, 2), "kernel_ms_min": round(min(ms), 2), "kernel_ms_max": round(max(ms), 2),
                           "gcups": round(cells / med / 1e6, 2)}
                if path == "general":
                    r[path].update(wall_stats(wall))
                note(name, path, r[path]["kernel_ms_median"], "ms")
            sample = sets[:a.cpu_sample]
            if "cpu" in only:
                t0 = time.perf_counter()
                with ThreadPoolExecutor(16) as ex:
                    out = list(ex.map(lambda st: ref.consensus_cells(st, mode), sample))
                dt = time.perf_counter() - t0
                sc = sum(c for _, c in out)
                r["cpu_restatement_16t"] = {"sets": len(sample), "cells": int(sc), "s": round(dt, 2), "gcups": round(sc / dt / 1e9, 3)}
                got = ctx.poa_sequences_mode(sample, mode)
                r["sample_equal"] = got == [c for c, _ in out]
            if "affine" in only:
                cells = ctx.poa_sequences_affine(sets, mode, *a.affine_scores, stats=True)[1]["dp_cells"]
                ms, _ = gpu_time(ctx, lambda: ctx.poa_sequences_affine(sets, mode, *a.affine_scores), a.repeats)
                med = float(np.median(ms))
                r["affine"] = {"cells": int(cells), "kernel_ms_median": round(med, 2), "kernel_ms_min": round(min(ms), 2), "kernel_ms_max": round(max(ms), 2),
                               "gcups": round(cells / med / 1e6, 2)}
                if "general" in r:
                    r["affine"]["over_linear"] = round(med / r["general"]["kernel_ms_median"], 3)
                with ThreadPoolExecutor(16) as ex:
                    out = list(ex.map(lambda st: aref.consensus(st, mode, *a.affine_scores), sample))
                r["affine_sample_equal"] = ctx.poa_sequences_affine(sample, mode, *a.affine_scores) == out
                note(name, "affine", r["affine"]["kernel_ms_median"], "ms")
            if "convex" in only:
                cells = ctx.poa_sequences_convex(sets, mode, *a.convex_scores, stats=True)[1]["dp_cells"]
                ms, _ = gpu_time(ctx, lambda: ctx.poa_sequences_convex(sets, mode, *a.convex_scores), a.repeats)
                med = float(np.median(ms))
                r["convex"] = {"cells": int(cells), "kernel_ms_median": round(med, 2), "kernel_ms_min": round(min(ms), 2), "kernel_ms_max": round(max(ms), 2),
                               "gcups": round(cells / med / 1e6, 2)}
                for key, base in (("over_affine", r.get("affine")), ("over_linear", r.get("general"))):
                    if base:
                        r["convex"].update({key: round(med / base["kernel_ms_median"], 3), key + "_min": round(min(ms) / base["kernel_ms_max"], 3),
                                            key + "_max": round(max(ms) / base["kernel_ms_min"], 3)})
                with ThreadPoolExecutor(16) as ex:
                    out = list(ex.map(lambda st: cref.consensus(st, mode, tuple(a.convex_scores)), sample))
                got = ctx.poa_sequences_convex(sample, mode, *a.convex_scores)
                r["convex_sample_equal"] = got == out
                r["convex_sample_differing_sets"] = [k for k in range(len(sample)) if got[k] != out[k]]
                note(name, "convex", r["convex"]["kernel_ms_median"], "ms")
            if "outputs" not in only or "general" not in r:
                res[name] = r
                continue
            rows_ms, moved = [], 0

            def msa_call():
                nonlocal moved
                st = ctx.poa_msa(sets, mode, include_consensus=True, stats=True)[2]
                rows_ms.append(st["rows_kernel_ms"])
                moved = st["rows_kernel_bytes"]
            ms, wall = gpu_time(ctx, msa_call, a.repeats)
            med, gen = float(np.median(ms)), r["general"]
            rmed = float(np.median(rows_ms[1:]))
            r["msa"] = {"kernel_ms_median": round(med, 2), "kernel_ms_min": round(min(ms), 2), "kernel_ms_max": round(max(ms), 2),
                        "over_general": round(med / gen["kernel_ms_median"], 4), "over_general_min": round(min(ms) / gen["kernel_ms_max"], 4),
                        "over_general_max": round(max(ms) / gen["kernel_ms_min"], 4),
                        "rows_kernel": {"ms_median": round(rmed, 4), "ms_min": round(min(rows_ms[1:]), 4), "ms_max": round(max(rows_ms[1:]), 4),
                                        "bytes": int(moved), "gb_per_s": round(moved / rmed / 1e6, 1)}}
            r["msa"].update(wall_stats(wall))
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
            ms, wall = gpu_time(ctx, weighted_call, a.repeats)
            med = float(np.median(ms))
            cmed = float(np.median(cov_ms[1:]))
            r["weighted"] = {"kernel_ms_median": round(med, 2), "kernel_ms_min": round(min(ms), 2), "kernel_ms_max": round(max(ms), 2),
                             "over_general": round(med / gen["kernel_ms_median"], 4), "over_general_min": round(min(ms) / gen["kernel_ms_max"], 4),
                             "over_general_max": round(max(ms) / gen["kernel_ms_min"], 4),
                             "coverage_kernels": {"ms_median": round(cmed, 4), "ms_min": round(min(cov_ms[1:]), 4), "ms_max": round(max(cov_ms[1:]), 4),
                                                  "bytes": int(moved), "gb_per_s": round(moved / cmed / 1e6, 1)}}
            r["weighted"].update(wall_stats(wall))
            swts = [[w.tolist() for w in ws] for ws in wts[:a.cpu_sample]]
            with ThreadPoolExecutor(16) as ex:
                out = list(ex.map(lambda k: wref.weighted(sample[k], swts[k], mode), range(len(sample))))
            got = ctx.poa_weighted(sample, swts, type=mode, coverage=True, profile=True)
            r["weighted_sample_equal"] = list(zip(*got)) == [(w.consensus, w.coverage, w.profile) for w in out]
            r["weighted_sample_changed"] = sum(c != u for c, u in zip(got[0], ctx.poa_weighted(sample, type=mode)))
            if "graph" in only:
                import grflib
                gath_ms, gst = [], {}

                def graph_call():
                    nonlocal gst
                    gst = ctx.poa_graph(sets, mode, stats=True)[1]
                    gath_ms.append(gst["gather_kernel_ms"])
                ms, wall = gpu_time(ctx, graph_call, a.repeats)
                med, gmed, msa = float(np.median(ms)), float(np.median(gath_ms[1:])), r["msa"]
                r["graph"] = {"kernel_ms_median": round(med, 2), "kernel_ms_min": round(min(ms), 2), "kernel_ms_max": round(max(ms), 2),
                              "over_msa": round(med / msa["kernel_ms_median"], 4), "over_msa_min": round(min(ms) / msa["kernel_ms_max"], 4), "over_msa_max": round(max(ms) / msa["kernel_ms_min"], 4),
                              "over_general": round(med / gen["kernel_ms_median"], 4),
                              "gather_kernel": {"ms_median": round(gmed, 4), "ms_min": round(min(gath_ms[1:]), 4), "ms_max": round(max(gath_ms[1:]), 4),
                                                "bytes": int(gst["gather_kernel_bytes"]), "gb_per_s": round(gst["gather_kernel_bytes"] / gmed / 1e6, 1)},
                              "aln_reruns": int(gst["aln_reruns"]), "slot_reruns": int(gst["slot_reruns"])}
                r["graph"].update(wall_stats(wall))
                gref = grflib.GraphRef(d)
                with ThreadPoolExecutor(16) as ex:
                    out = list(ex.map(lambda st: gref.graph(st, mode), sample))
                r["graph_sample_equal"] = all(grflib.same(x, y) for x, y in zip(ctx.poa_graph(sample, mode), out))
                note(name, "graph", r["graph"]["kernel_ms_median"], "ms")
            if "strand" in only and name.startswith("a_"):
                import strlib
                srng = np.random.default_rng(a.seed + 2000)   # (a generator of its own, as for the weights)
                mixed = [[q if k == 0 or srng.random() < 0.5 else strlib.rc(q) for k, q in enumerate(st)] for st in sets]
                sst = {}

                def strand_call():
                    nonlocal sst
                    sst = ctx.poa_strand(mixed, mode, msa=True, include_consensus=True, stats=True)[1]
                ms, wall = gpu_time(ctx, strand_call, a.repeats)
                med, msa = float(np.median(ms)), r["msa"]
                r["strand"] = {"kernel_ms_median": round(med, 2), "kernel_ms_min": round(min(ms), 2), "kernel_ms_max": round(max(ms), 2),
                               "over_msa": round(med / msa["kernel_ms_median"], 4), "over_msa_min": round(min(ms) / msa["kernel_ms_max"], 4), "over_msa_max": round(max(ms) / msa["kernel_ms_min"], 4),
                               "third_passes": int(sst["third_passes"]), "n_aligned": int(sst["n_aligned"]), "dp_cells": int(sst["dp_cells"]),
                               "dp_passes_per_sequence": round(2 + sst["third_passes"] / max(1, sst["n_aligned"] - len(sets)), 4), "slot_reruns": int(sst["slot_reruns"])}
                r["strand"].update(wall_stats(wall))
                sref = strlib.StrandRef(d)
                few = mixed[:max(1, a.cpu_sample // 4)]   # (the restatement aligns every sequence twice, on full matrices)
                with ThreadPoolExecutor(16) as ex:
                    out = list(ex.map(lambda st: sref.strand(st, mode, include_consensus=True), few))
                got = ctx.poa_strand(few, mode, msa=True, include_consensus=True, coverage=True, profile=True)
                r["strand_sample_equal"] = got == out
                note(name, "strand", r["strand"]["kernel_ms_median"], "ms")
            res[name] = r
    ctx.close()
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
