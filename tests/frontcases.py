"""Seeded builder of hand-shaped inputs for the front half: the chain stage (filters, sort, palindrome rule, filter 5, overlap trim,
chaining), the edge-support stage and the coordinate stage. The simulator (tools/hxsim) never reaches many of their branches: reads
with more than 64 raw hits (the chain kernel's one-lane path), CIGAR letters other than M/I/D, trim walks that stop in particular
places, filters hit at exact equality, ties, and edges with more than 384 supports.

Every family is a function `add_<name>(case)` that plants its reads into a `Case` and records in `case.man` what it planted: which
hits must be kept or dropped, chained or not, which reads must keep how many alignments, which edges must exist. `build(dir, names,
seed)` writes contigs.fa / reads.fa / map.paf in hxsim's formats and returns (prefix, case); the tests check the manifest against the
oracle's chain / edge / coordinate output, so that a change to the builder cannot quietly turn a case into one that tests nothing.

The inputs keep to the reference's preconditions:
  - the PAF is grouped by ascending read id;
  - every CIGAR starts and ends with an M run, so a trim walk always finds an M to back off to (the back walk of Longread.cpp:399
    would otherwise read before index 0);
  - at most 10 000 hits per read (dp[10000], Longread.cpp:529);
  - a reverse-strand hit has t_start at least its total OTHER length, so no contig walk wraps below 0 (wrapping is out of scope);
  - hits with equal (q_end, q_start) only in reads with at most 16 surviving hits, where the reference is compared: libstdc++'s
    std::sort insertion-sorts such groups and keeps ties in order, above 16 it is unstable ("std::sort is unstable").
    Family `ties_large` has ties in larger groups and is for the GPU-against-oracle comparison only: the oracle fixes ties to PAF order.

OTHER letters (`=`, `X`, `S`, `N`, `H`) are contig-only steps for the trim walks, which never undo them when they back off
(Longread.cpp:375-420). `trim_model` restates those walks per base, from the reference's documented behaviour, for the families
whose reads lose no hit before the trim.
"""
import math
import os
import random

import numpy as np

import util

OTHER = "=XSNH"
UNIQ_KM = 30.0                  # km of the 20 longest contigs and of every ordinary contig: uniq_freq is exactly 30.0
MAX_UNIQ_DEV = 0.15             # defaults of Commandline.cpp (ctypes_defs.default_params)
THR_UNIQ = UNIQ_KM * (1 + MAX_UNIQ_DEV)    # the products the C code forms, in the same double arithmetic
THR_LOAD = UNIQ_KM * (3 + MAX_UNIQ_DEV)
MIN_BLOCK, MIN_SIM, MIN_MAPQ = 500, 0.85, 55

FAMILIES = ("hit_counts", "trims", "thresholds", "palindrome", "ties", "coords")   # all comparable with the reference
GPU_ONLY = ("ties_large",)


class Hit:
    __slots__ = ("read", "contig", "qs", "qe", "rev", "ts", "te", "nm", "nb", "mapq", "runs", "tag", "index")

    @property
    def cigar(self):
        return "".join(f"{n}{c}" for n, c in self.runs)

    @property
    def has_other(self):
        return any(c in OTHER for _, c in self.runs)


def spans(runs):
    q = sum(n for n, c in runs if c in "MI")
    t = sum(n for n, c in runs if c not in "I")
    return q, t


class Case:
    """contigs, reads and hits under construction; `man` is the manifest the families fill in"""

    def __init__(self, seed):
        self.rng = random.Random(seed)
        self.contigs = []      # [length, km, sequence or None]
        self.reads = []        # [length, sequence or None]
        self.hits = []
        self.man = {"kept": [], "dropped": [], "chained": [], "unchained": [], "n_aln": {}, "serial_reads": [], "model_reads": [],
                    "pairs": [], "no_pair": [], "edge_records": [], "ref_ties": True}
        for _ in range(20):    # the 20 longest contigs: uniq_freq = their mean km, exactly UNIQ_KM (Contig.cpp:162-174)
            self.contig(70000)

    def contig(self, length, km=UNIQ_KM, seq=None):
        self.contigs.append([length, km, seq])
        return len(self.contigs) - 1

    def read(self, length=0, seq=None):
        self.reads.append([length, seq])
        return len(self.reads) - 1

    def hit(self, read, contig, qs, runs, rev=False, ts=None, nm=None, nb=None, mapq=60, tag=None, tlen=None):
        """one PAF record; the contig is created to fit when `contig` is None (full coverage unless tlen says otherwise)"""
        assert runs[0][1] == "M" and runs[-1][1] == "M", "a CIGAR starts and ends with an M run"
        q, t = spans(runs)
        n_other = sum(n for n, c in runs if c in OTHER)
        if ts is None:
            ts = n_other if rev else 0
        assert not rev or ts >= n_other
        if contig is None:
            contig = self.contig(tlen or ts + t)
        assert ts + t <= self.contigs[contig][0]
        h = Hit()
        h.read, h.contig, h.qs, h.qe, h.rev, h.ts, h.te = read, contig, qs, qs + q, rev, ts, ts + t
        h.nb = nb if nb is not None else sum(n for n, _ in runs)
        h.nm = nm if nm is not None else sum(n for n, c in runs if c == "M")
        h.mapq, h.runs, h.tag, h.index = mapq, runs, tag, None
        self.reads[read][0] = max(self.reads[read][0], h.qe)
        self.hits.append(h)
        return h

    # ---- CIGAR shapes
    def dense(self, n_ops):
        """n_ops runs (n_ops >= 1), short and mixed, first and last M, no two neighbours with the same letter"""
        rng = self.rng
        if n_ops == 1:
            return [(rng.randint(1, 6), "M")]
        out = [(rng.randint(1, 6), "M")]
        while len(out) < n_ops - 1:
            c = rng.choice("MMMMIID" + OTHER)
            if c == out[-1][1]:
                continue
            out.append((rng.randint(1, 6) if c == "M" else rng.randint(1, 3), c))
        if out[-1][1] == "M":        # the last run must be M and differ from its neighbour: swap in a non-M
            out[-1] = (rng.randint(1, 3), rng.choice("ID" + OTHER))
        out.append((rng.randint(1, 6), "M"))
        return out

    def shaped(self, q_len, ends=12, n_ops=None):
        """about q_len read bases. By default a dense, mixed head and tail of `ends` runs around one long M run (the trim walks stop
        near the ends). n_ops: exactly that many runs (1 or at least 3), M runs alternating with one-base non-M runs throughout"""
        rng = self.rng
        if n_ops is None:
            head, tail = self.dense(ends)[:-1], self.dense(ends)[1:]
            mid = max(1, q_len - spans(head)[0] - spans(tail)[0])
            return head + [(mid, "M")] + tail
        assert n_ops == 1 or n_ops >= 3
        if n_ops == 1:
            return [(q_len, "M")]
        n_m = (n_ops + 1) // 2
        ln = max(8, q_len // n_m)
        out = []
        for k in range(n_m):
            out.append((rng.randint(ln - 3, ln + 3), "M"))
            if k + 1 < n_m:
                out.append((1, rng.choice("ID" + OTHER)))
        if n_ops % 2 == 0:     # one place with two different non-M letters in a row
            i = 2 * rng.randrange(n_m - 1) + 1
            out.insert(i + 1, (1, rng.choice([c for c in "ID" + OTHER if c != out[i][1]])))
        assert len(out) == n_ops
        return out

    # ---- writers
    def seq(self, n):
        return "".join(self.rng.choices("ACGT", k=n))

    def write(self, prefix):
        hits = sorted(self.hits, key=lambda h: h.read)   # stable: a read's hits stay in the order they were planted
        for i, h in enumerate(hits):
            h.index = i
        self.hits = hits
        with open(prefix + ".contigs.fa", "w") as f:
            for i, (ln, km, s) in enumerate(self.contigs):
                s = s if s is not None else self.seq(ln)
                assert len(s) == ln
                f.write(f">{i} LN:i:{ln} KC:i:{int(km * ln)} km:f:{km!r}\n{s}\n")
        with open(prefix + ".reads.fa", "w") as f:
            for i, (ln, s) in enumerate(self.reads):
                s = s if s is not None else self.seq(max(ln, 1))
                f.write(f">{i}\n{s}\n")
        with open(prefix + ".paf", "w") as f:
            for h in hits:
                f.write("%d\t%d\t%d\t%d\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\ttp:A:P\tcg:Z:%s\n" % (
                    h.read, max(self.reads[h.read][0], 1), h.qs, h.qe, "-" if h.rev else "+", h.contig, self.contigs[h.contig][0],
                    h.ts, h.te, h.nm, h.nb, h.mapq, h.cigar))
        return prefix

    def tagged(self, tag):
        return [h.index for h in self.hits if h.tag == tag]

    def spread(self, n_reads, at):
        """move read r to index at[r] among n_reads reads; every other read has 4 bases and no hit. The manifest follows."""
        assert len(at) == len(self.reads) and len(set(at)) == len(at) and max(at) < n_reads
        fill = [4, "ACGT"]
        reads = [fill] * n_reads
        for old, new in enumerate(at):
            reads[new] = self.reads[old]
        self.reads = reads
        for h in self.hits:
            h.read = at[h.read]
        self.man["n_aln"] = {at[r]: n for r, n in self.man["n_aln"].items()}
        for k in ("serial_reads", "model_reads"):
            self.man[k] = [at[r] for r in self.man[k]]


# =====================================================================================================================
# per-base restatement of the trim walks (find_contig_pos, Longread.cpp:375-420; fix_overlapping_alignments, :430-512)
# =====================================================================================================================
def walk(exp, lr, c, lstep, cstep, lr_pos):
    """-> (lr, c, kept expanded ops, letter the walk stopped at or None when the ops ran out, OTHER bases kept behind the last M)"""
    i = 0
    while i < len(exp):
        if lr == lr_pos:
            break
        ch = exp[i]
        if ch == "M":
            c += cstep; lr += lstep
        elif ch == "I":
            lr += lstep
        else:
            c += cstep
        i += 1
    stop = exp[i] if i < len(exp) else None
    other = 0
    while i >= len(exp) or exp[i] != "M":
        p = exp[i - 1]
        if p == "M":
            c -= cstep; lr -= lstep
        elif p == "I":
            lr -= lstep
        elif p == "D":
            c -= cstep
        else:
            other += 1
        i -= 1
    return lr, c, exp[:i + 1], stop, other


def trim_model(hits):
    """the alignments of one read after the overlap trim, for a read that loses no hit to a filter, the palindrome rule or filter 5:
    (list of dicts with qs, qe, ts, te, nm, nb, index; list of walks as (strand, side, stop letter, OTHER kept behind the last M))"""
    rows = []
    for h in sorted(hits, key=lambda h: (h.qe, h.qs)):
        rows.append({"qs": h.qs, "qe": h.qe, "ts": h.ts, "te": h.te, "nm": h.nm, "nb": h.nb, "rev": h.rev, "index": h.index,
                     "exp": "".join(c * n for n, c in h.runs)})
    walks = []
    for i in range(len(rows) - 1):
        a, b = rows[i], rows[i + 1]
        if not a["qe"] > b["qs"]:
            continue
        ov = a["qe"] - b["qs"]
        tgt = a["qe"] - ov // 2 - 1
        if not a["rev"]:
            lr, c, kept, stop, oth = walk(a["exp"], a["qs"], a["ts"], +1, +1, tgt)
            a["qe"], a["te"], a["exp"] = lr + 1, c + 1, kept
        else:
            lr, c, kept, stop, oth = walk(a["exp"][::-1], a["qs"], a["te"] - 1, +1, -1, tgt)
            a["qe"], a["ts"], a["exp"] = lr + 1, c, kept[::-1]
        a["nb"], a["nm"] = len(a["exp"]), a["exp"].count("M")
        walks.append(("-" if a["rev"] else "+", "first", stop, oth))
        tgt = b["qs"] + (ov - ov // 2)
        if not b["rev"]:
            lr, c, kept, stop, oth = walk(b["exp"][::-1], b["qe"] - 1, b["te"] - 1, -1, -1, tgt)
            b["qs"], b["ts"], b["exp"] = lr, c, kept[::-1]
        else:
            lr, c, kept, stop, oth = walk(b["exp"], b["qe"] - 1, b["ts"], -1, +1, tgt)
            b["qs"], b["te"], b["exp"] = lr, c + 1, kept
        b["nb"], b["nm"] = len(b["exp"]), b["exp"].count("M")
        walks.append(("-" if b["rev"] else "+", "second", stop, oth))
    return rows, walks


# =====================================================================================================================
# families
# =====================================================================================================================
def tiled_read(case, n_hits, overlaps=range(0, 58), q_len=(520, 700), shapes=None, revs=None, tag=None, shuffle=True):
    """a read with n_hits raw hits to distinct fresh contigs, laid out left to right with the given overlaps, both strands (random
    unless revs says), mixed CIGARs; the PAF order is shuffled so that the sort has work to do"""
    rng = case.rng
    r = case.read()
    q = 0
    hits = []
    for k in range(n_hits):
        runs = shapes[k] if shapes is not None else case.shaped(rng.randint(*q_len))
        rev = revs[k] if revs is not None else rng.random() < 0.5
        h = case.hit(r, None, q, runs, rev=rev, tag=tag)
        hits.append(h)
        q = h.qe - (rng.choice(overlaps) if k + 1 < n_hits else 0)
    if shuffle:
        order = list(range(len(hits)))
        rng.shuffle(order)
        case.hits[len(case.hits) - n_hits:] = [hits[i] for i in order]
    return r, hits


def add_hit_counts(case):
    """reads with 1 .. ~1000 raw hits; above 64 the chain kernel takes its one-lane path"""
    for n in (1, 2, 16, 17, 63, 64, 65, 130, 1000):
        r, hits = tiled_read(case, n)
        case.man["n_aln"][r] = n if n > 1 else 0      # a lone hit is dropped (Longread.cpp:184)
        if n > 1:
            case.man["model_reads"].append(r)
        if n > 64:
            case.man["serial_reads"].append(r)
    # 90 raw hits of which filter 1 drops 30: 60 survivors, still the one-lane path (the kernel branches on raw hits)
    rng = case.rng
    r = case.read()
    q = 0
    for k in range(90):
        short = k % 3 == 1
        runs = case.shaped(rng.randint(300, 450) if short else rng.randint(520, 700))
        h = case.hit(r, None, q, runs, rev=rng.random() < 0.5, tag="hc_short" if short else None)
        q = h.qe - rng.randint(0, 40)
    case.man["n_aln"][r] = 60
    case.man["serial_reads"].append(r)
    case.man["dropped"].append("hc_short")


def add_trims(case):
    """overlaps of 0, 1, 2, 3 and large ones; stops in every letter on both strands (many random pairs with dense CIGAR ends);
    CIGARs of 1, 63, 64, 65 and thousands of ops; a hit cut on both sides; a contained hit whose target lies behind its start;
    a trim that leaves a hit below min_aln_block"""
    rng = case.rng
    small = (0, 1, 2, 3, 1, 2, 3, 5, 8, 13, 21, 34, 57)
    for n, reps in ((2, 6), (3, 6), (5, 4), (20, 2), (64, 1), (65, 1), (80, 2)):
        for _ in range(reps):
            r, _ = tiled_read(case, n, overlaps=small)
            case.man["model_reads"].append(r)
            if n > 64:
                case.man["serial_reads"].append(r)
    for n, reps in ((4, 4), (70, 1)):   # large overlaps: 120-301 bases
        for _ in range(reps):
            r, _ = tiled_read(case, n, overlaps=(120, 121, 200, 301), q_len=(900, 1100))
            case.man["model_reads"].append(r)
    # op counts at the lane split of the wave walk: 1 op, 63, 64, 65 and a few thousand, on both sides of overlaps
    for n_ops in (1, 3, 4, 62, 63, 64, 65, 66, 127, 128, 129, 3000):
        for rev in (False, True):
            for reads_hits in (3, 66):
                shapes = [case.shaped(800 if n_ops < 1000 else 12000, n_ops=n_ops) if k == 1 else case.shaped(rng.randint(520, 700))
                          for k in range(reads_hits)]
                revs = [rev if k == 1 else rng.random() < 0.5 for k in range(reads_hits)]
                r, hits = tiled_read(case, reads_hits, overlaps=(7, 33, 57, 2, 3), shapes=shapes, revs=revs)
                case.man["model_reads"].append(r)
                if reads_hits > 64:
                    case.man["serial_reads"].append(r)
    # a contained hit whose cut target lies behind its start, the big hit cut on both sides, and a trim that leaves a hit below
    # min_aln_block (two 130-base overlaps on a 560-base hit), on the wave path and on the one-lane path
    for n_extra in (0, 66):
        r = case.read()
        q = 0
        hits = []
        for _ in range(n_extra // 2):
            hits.append(case.hit(r, None, q, case.shaped(rng.randint(520, 700))))
            q = hits[-1].qe + 10
        p = case.hit(r, None, q, case.shaped(600), tag="tr_p")
        big = case.hit(r, None, p.qe - 40, case.shaped(3000), rev=True)
        case.hit(r, None, big.qs + 1800, case.shaped(600), tag="tr_contained")    # q_end 2400 after big's start: ov/2 = 1200 > 600
        nxt = case.hit(r, None, big.qe - 130, case.shaped(560), tag="tr_below")
        case.hit(r, None, nxt.qe - 130, case.shaped(600))
        q = nxt.qe + 500
        for _ in range(n_extra - n_extra // 2):
            hits.append(case.hit(r, None, q, case.shaped(rng.randint(520, 700))))
            q = hits[-1].qe + 10
        case.man["model_reads"].append(r)
        case.man["unchained"].append("tr_below")
        if n_extra:
            case.man["serial_reads"].append(r)


def add_thresholds(case):
    """filters hit at exact equality, and one step from it"""
    rng = case.rng

    def probe(runs, tag, keep, **kw):
        """a read: anchor, the probe in the middle (interior: filter 5 applies), anchor; no overlaps"""
        r = case.read()
        a = case.hit(r, None, 0, [(600, "M")])
        x = case.hit(r, kw.pop("contig", None), a.qe + 50, runs, tag=tag, **kw)
        case.hit(r, None, x.qe + 50, [(600, "M")])
        case.man["kept" if keep else "dropped"].append(tag)
        return x

    # filter 1: n_block (the PAF field) at min_aln_block and one below
    probe([(500, "M")], "th_nb500", True)
    probe([(499, "M")], "th_nb499", False)
    # filter 2: n_match / n_block equal to min_aln_sim in double precision, and one match short
    for nb in (500, 520, 600, 1000, 2000, 20000):
        nm = nb * 85 // 100
        assert nm / nb == MIN_SIM and (nm - 1) / nb < MIN_SIM
        runs = [(nm // 2, "M"), (nb - nm, "D"), (nm - nm // 2, "M")]
        probe(runs, f"th_sim_eq_{nb}", True)
        probe(runs, f"th_sim_lo_{nb}", False, nm=nm - 1)
    # filter 3: MAPQ at min_aln_mapq and one below
    probe([(600, "M")], "th_mapq55", True, mapq=55)
    probe([(600, "M")], "th_mapq54", False, mapq=54)
    # filter 5: an interior hit covering exactly 0.8 of its contig, and one base less; first and last hits are exempt
    for span, tl in ((800, 1000), (1600, 2000), (4000, 5000)):
        assert span / tl == 0.8 and (span - 1) / tl < 0.8
        probe([(span, "M")], f"th_cov_eq_{tl}", True, tlen=tl, ts=rng.randint(0, tl - span))
        probe([(span - 1, "M")], f"th_cov_lo_{tl}", False, tlen=tl, ts=rng.randint(0, tl - span))
    for first in (True, False):
        r = case.read()
        if first:
            x = case.hit(r, None, 0, [(799, "M")], tlen=1000, ts=100, tag="th_cov_first")
            case.hit(r, None, x.qe + 50, [(600, "M")])
        else:
            a = case.hit(r, None, 0, [(600, "M")])
            case.hit(r, None, a.qe + 50, [(799, "M")], tlen=1000, ts=0, tag="th_cov_last")
    case.man["kept"] += ["th_cov_first", "th_cov_last"]
    # km at the two thresholds and their neighbours: filter 4 (> thr_load), the palindrome rule (< thr_uniq), chaining (> thr_uniq)
    # and edges (<= thr_uniq)
    for name, km, keep, chained in (("load_eq", THR_LOAD, True, False), ("load_up", math.nextafter(THR_LOAD, math.inf), False, False),
                                    ("load_dn", math.nextafter(THR_LOAD, -math.inf), True, False), ("uniq_eq", THR_UNIQ, True, True),
                                    ("uniq_dn", math.nextafter(THR_UNIQ, -math.inf), True, True),
                                    ("uniq_up", math.nextafter(THR_UNIQ, math.inf), True, False)):
        c = case.contig(700, km)
        x = probe([(600, "M")], f"th_km_{name}", keep, contig=c)
        if keep:
            case.man["chained" if chained else "unchained"].append(f"th_km_{name}")
        anchors = [h for h in case.hits if h.read == x.read and h is not x]
        # an edge through the probe exactly when its contig is at or below thr_uniq (and chained)
        for a in anchors:
            case.man["pairs" if chained else "no_pair"].append((min(a.contig, c), max(a.contig, c)))
        if not chained:
            case.man["pairs"].append((anchors[0].contig, anchors[1].contig))
        # the same contig twice in one read: cut at the second hit only when the contig is unique (km < thr_uniq)
        if keep:
            r = case.read()
            hs = [case.hit(r, None, 0, [(600, "M")])]
            hs.append(case.hit(r, c, hs[-1].qe + 50, [(600, "M")]))
            hs.append(case.hit(r, None, hs[-1].qe + 50, [(600, "M")]))
            hs.append(case.hit(r, c, hs[-1].qe + 50, [(600, "M")]))
            hs.append(case.hit(r, None, hs[-1].qe + 50, [(600, "M")]))
            case.man["n_aln"][r] = 3 if km < THR_UNIQ else 5


def add_palindrome(case):
    """the second hit of a unique contig at group positions 1, 16, 63, 64 and 100, on both chain paths"""
    for p, n in ((1, 6), (16, 40), (63, 64), (1, 70), (16, 70), (63, 70), (64, 70), (100, 110)):
        r = case.read()
        q = 0
        hs = []
        for k in range(n):
            if k == p:    # the same contig, CIGAR and strand as an earlier hit
                first = hs[p // 2]
                hs.append(case.hit(r, first.contig, q, first.runs, rev=first.rev, ts=first.ts))
            else:
                hs.append(case.hit(r, None, q, case.shaped(case.rng.randint(520, 600)), rev=k % 3 == 0))
            q = hs[-1].qe + 5
        case.man["n_aln"][r] = p
        if n > 64:
            case.man["serial_reads"].append(r)


def add_ties(case, large=False):
    """equal (q_end, q_start) for different contigs, equal chain weights, q_end of one hit equal to q_start of the next"""
    rng = case.rng
    # equal (q_end, q_start): two hits over the same read interval, in a small group (and, large=True, in groups above 16)
    for n in ((40, 80) if large else (4, 6, 15)):
        r = case.read()
        q = 0
        for k in range(n):
            runs = case.shaped(rng.randint(520, 600))
            h = case.hit(r, None, q, runs, rev=k % 2 == 1)
            if k % 4 == 1 and large or (not large and k == 1):
                case.hit(r, None, h.qs, case.shaped(h.qe - h.qs), rev=k % 2 == 0)     # same (q_start, q_end), PAF order after h
            q = h.qe + 30
        case.man["n_aln"][r] = len([h for h in case.hits if h.read == r])
        if n > 64:
            case.man["serial_reads"].append(r)
    if large:
        case.man["ref_ties"] = False
        return
    # q_end == q_start of the next hit: no trim, and the two chain together (the '<=' of latest_compatible, Longread.cpp:518)
    for n in (3, 70):
        r = case.read()
        q = 0
        for k in range(n):
            h = case.hit(r, None, q, case.shaped(rng.randint(520, 600)), tag="ti_touch" if n == 3 else None)
            q = h.qe
        case.man["model_reads"].append(r)
        case.man["n_aln"][r] = n
        if n > 64:
            case.man["serial_reads"].append(r)
    case.man["chained"].append("ti_touch")
    # equal chain weights: a hit contained in a longer one after its trim, both of weight 600; the strict '>' keeps the earlier
    # (Longread.cpp:576,590). big spans 2000 read bases from Q; `in` ends at Q + 1900 and sorts before it; their overlap of 1900 leaves
    # `in` whole (its cut target lies behind its start) and cuts big to [Q + 950, Q + 2000): 300 M, 450 I, 300 M, weight 600 like `in`
    for n_extra in (0, 66):
        r = case.read()
        q = 0
        for _ in range(n_extra):
            q = case.hit(r, None, q, case.shaped(rng.randint(520, 600))).qe + 10
        p = case.hit(r, None, q, [(600, "M")], tag="ti_w_p")
        big = case.hit(r, None, p.qe + 400, [(1250, "M"), (450, "I"), (300, "M")], nm=1800, tag="ti_w_big")   # (the PAF field passes filter 2)
        case.hit(r, None, big.qs + 1300, [(600, "M")], tag="ti_w_in")
        case.hit(r, None, big.qe + 100, [(600, "M")], tag="ti_w_b")
        case.man["model_reads"].append(r)
        if n_extra:
            case.man["serial_reads"].append(r)
    case.man["chained"] += ["ti_w_p", "ti_w_in", "ti_w_b"]
    case.man["unchained"].append("ti_w_big")


def add_ties_large(case):
    add_ties(case, large=True)


def add_coords(case):
    """one edge with 400 supports (above LDS_SUPP = 384: the coordinate kernel's global-scratch path under the default setting), one
    with exactly 384; the supports' anchor intervals come in two clusters of equal size with many equal t_start / t_end values,
    so the head sweep (last maximum) and the tail sweep (first maximum) choose different clusters; some support CIGARs carry OTHER
    letters. One read chains 300 alignments."""
    rng = case.rng
    for n_supp in (400, 384):
        lc = 2000
        A = case.contig(lc, seq=case.seq(lc))
        B = case.contig(lc, seq=case.seq(lc))
        gap = case.seq(120)
        A_seq, B_seq = case.contigs[A][2], case.contigs[B][2]
        for k in range(n_supp):
            hc, tc = k % 2, (k // 2) % 2
            ts_a = (100 if hc == 0 else 1100) + 50 * rng.randint(0, 1)
            ts_b = (0 if tc == 0 else 1000) + 50 * rng.randint(0, 1)
            runs_a = [(600, "M")] if k % 5 else [(300, "M"), (2, rng.choice(OTHER)), (2, "I"), (298, "M")]
            runs_b = [(600, "M")] if k % 7 else [(250, "M"), (3, "D"), (3, rng.choice(OTHER)), (6, "I"), (344, "M")]
            g = list(gap)
            g[rng.randrange(len(g))] = rng.choice("ACGT")
            seq = A_seq[ts_a:ts_a + 600] + "".join(g) + B_seq[ts_b:ts_b + 600]
            r = case.read(len(seq), seq)
            case.hit(r, A, 0, runs_a, ts=ts_a)
            case.hit(r, B, 600 + len(gap), runs_b, ts=ts_b)
        case.man["edge_records"].append(((A, B), n_supp))
    r, _ = tiled_read(case, 300, overlaps=(0, 0, 1, 2, 17))
    case.man["n_aln"][r] = 300
    case.man["model_reads"].append(r)
    case.man["serial_reads"].append(r)


def fixed_paf_equal(case, ds, chain, ref_text):
    """alignments.fixed.paf: whole lines for hits whose CIGAR holds only M/I/D, the fields before cg:Z: for the rest (the run-length
    codes do not tell the OTHER letters apart)"""
    ours, ref = util.alignments_paf(ds, chain).splitlines(), ref_text.splitlines()
    assert len(ours) == len(ref)
    n_other = 0
    for a, line_o, line_r in zip(chain["hit"], ours, ref):
        if case.hits[int(a)].has_other:
            n_other += 1
            assert line_o.split("\tcg:Z:")[0] == line_r.split("\tcg:Z:")[0]
        else:
            assert line_o == line_r
    return n_other


ADD = {"hit_counts": add_hit_counts, "trims": add_trims, "thresholds": add_thresholds, "palindrome": add_palindrome, "ties": add_ties,
       "ties_large": add_ties_large, "coords": add_coords}


def many_reads_edges(n_reads):
    """read indices on both sides of the scans' ownership edges over the reads (4 per thread, 1 024 per block, 2^20 per block of
    blocks), the first and the last"""
    return [i for i in (0, 1023, 1024, 1025, (1 << 20) - 1, 1 << 20) if i < n_reads - 1] + [n_reads - 1]


def many_reads_at(n_reads):
    """where the ten reads of hit_counts (1, 2, 16, 17, 63, 64, 65, 130, 1000 and 90 raw hits) go among n_reads reads: those with
    alignments and pairs to the indices of many_reads_edges (the 1000-hit read last), the others to small indices in between"""
    e = many_reads_edges(n_reads)
    at = dict(zip((1, 2, 3, 4, 6, 7), e[:-1]))
    at[8] = e[-1]
    free = (i for i in range(2, n_reads) if i not in e)
    return [at[r] if r in at else next(free) for r in range(10)]


def check_many_reads(case, n_reads, chain, edges):
    """the planted reads kept their alignments where they went, and the reads at the scans' edges carry alignments, compact
    alignments and pairs: the three scans over the reads have non-zero values on both sides of every edge"""
    n_aln, n_cmp = np.diff(chain["read_off"]), np.diff(chain["cmp_off"])
    assert len(n_aln) == n_reads
    for r, n in case.man["n_aln"].items():
        assert n_aln[r] == n, f"read {r}: {n_aln[r]} alignments, planted {n}"
    with_pairs = set((edges["lr"][edges["lr"] < 0x80000000]).tolist())
    for r in many_reads_edges(n_reads):
        assert n_aln[r] > 0 and n_cmp[r] > 1 and r in with_pairs, f"read {r} carries nothing across the scan's edge"
    assert int((n_aln > 0).sum()) == len([n for n in case.man["n_aln"].values() if n])


def build(out_dir, names, seed=1, n_reads=None, reads_at=None):
    """write the families `names` into one data set under out_dir; -> (file prefix, Case). n_reads, reads_at: Case.spread"""
    case = Case(seed)
    for n in names:
        ADD[n](case)
    if n_reads is not None:
        case.spread(n_reads, reads_at)
    os.makedirs(out_dir, exist_ok=True)
    return case.write(os.path.join(out_dir, "in")), case
