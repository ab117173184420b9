"""Hand-built inputs for the back half: edge coordinates (Assemble.cpp:24-363), the sub-sequence rule (:528-543), path extraction and
stitching (:607-810). Family `back` of tests/frontcases.py's `Case` builder. The simulator reaches only the common branch of each of
these: every support in both best sets, walks that stop in the middle of an M run, no edge without a bridging read.

Every edge is planted in PATH ORIENTATION: an edge (A, rev1) -> (B, rev2) is left through A's end when rev1 == 0 and through A's start
when rev1 == 1, and enters B at its start when rev2 == 0. A path coordinate on a contig of length L is the column itself on strand 0
and L - 1 - column on strand 1. A support is a read whose head alignment covers the path interval [hs, he] of A with an expanded
CIGAR in path order, then `gap` read bases, then a tail alignment on B; gap < 0 makes the two overlap on the read, so that the front
half trims both before the back half sees them (both ends of the overlap are M runs and the overlap is even: each alignment loses
exactly gap / 2 columns). `flip` writes the reverse complement of that read: its records reach the edge as twin records, which the
reference handles as strand '-' (cases 5-8 of :297-324, the non-flipped ones are cases 1-4). Contig ids grow along every path, so the
reference's work queue (:365-434) hands out each edge in the planted direction.

What each edge plants is recorded in case.man["back"], from a per-base model of the two walks of asm_find_lr_pos:
  edges      {(A, rev1, B, rev2): {"n_supp", "best1", "best2" (the intervals the reference logs, contig coordinates), "supporting",
             "reads": {read id: (case numbers, lr_start, lr_end) as the reference logs them}, "what": walk positions per read}}
  census     how often the reference's logs must show each branch (backlib.census) for the family as a whole
tests/test_back_half_ref.py checks both against the REFERENCE's logs, so a change to this builder cannot quietly turn a case into one
that tests nothing.

Branches of the source that cannot be reached through the reference's own front half (none of the planted inputs reaches them, and
the test asserts that the reference's logs never show them):
  `could not extract subseq` (:333-336)  asm_find_lr_pos returns -1 only when the walk starts beyond the target column (:132). A read is
      walked only when it is in both best sets. A sweep's best set is the set of intervals open at its last new maximum, so every member
      has t_start <= beg_best < t_end. end_best is the first end coordinate that follows, so beg_best < end_best <= t_end of every member
      (a member's own end is among the ends that follow). Both targets, beg_best and end_best - 1, therefore lie in [t_start, t_end - 1]
      of every walked alignment, and a walk starts at t_start (going up) or at t_end - 1 (going down).
  a wrapped sub-sequence (epos + 1 < spos)  the walks return read positions inside the head and the tail alignment (the same bound), the
      head precedes the tail on the read, and after fix_alignments two alignments of a read are disjoint on it: lr_end >= lr_start + 1,
      with equality when both walks stop at the abutting ends (the empty sub-sequence, planted below).
The device-side wrap rule keeps its direct test (test_poa_supports_edge_cases_through_hip).
"""
import collections
import itertools
import os

import frontcases as fc
from backlib import revcomp

WALK_POSITIONS = ("last", "first", "I_before", "D_before", "D_covering")


def rle(exp):
    return [(len(list(g)), c) for c, g in itertools.groupby(exp)]


class Back:
    """plants edges into a frontcases.Case and keeps the manifest"""

    def __init__(self, case):
        self.case = case
        self.oriented = {}
        self.pending = collections.OrderedDict()   # edge key -> list of support models
        self.man = case.man.setdefault("back", {"edges": {}, "census": collections.Counter(), "records": []})

    def contig(self, length, km=fc.UNIQ_KM):
        c = self.case.contig(length, km, seq=self.case.seq(length))
        return c

    def seq_of(self, c, rev):
        if (c, rev) not in self.oriented:
            s = self.case.contigs[c][2]
            self.oriented[(c, rev)] = revcomp(s) if rev else s
        return self.oriented[(c, rev)]

    def bases(self, c, rev, start, exp):
        s, out, p = self.seq_of(c, rev), [], start
        for ch in exp:
            if ch == "M":
                out.append(s[p]); p += 1
            elif ch == "I":
                out.append(self.case.rng.choice("ACGT"))
            else:
                p += 1
        return "".join(out), p - 1    # read bases, last path column covered

    def side(self, c, rev, ps, pe, exp):
        """(t_start, runs in contig order) of the alignment over path columns [ps, pe]"""
        L = self.case.contigs[c][0]
        assert 0 <= ps <= pe < L and exp[0] == "M" and exp[-1] == "M"
        return (ps, rle(exp)) if rev == 0 else (L - 1 - pe, rle(exp[::-1]))

    def support(self, A, ra, B, rb, hs, hx, ts, tx, gap, flip, gap_seq="", what=None):
        case = self.case
        assert A < B or (A == B and ra != rb), "contig ids grow along a path"
        hb, he = self.bases(A, ra, hs, hx)
        tb, te = self.bases(B, rb, ts, tx)
        if gap >= 0:
            g = (gap_seq * (gap // max(1, len(gap_seq)) + 1))[:gap] if gap_seq else case.seq(gap)
            fwd = hb + g + tb
        else:
            ov = -gap
            assert ov % 2 == 0 and set(hx[-ov:]) == {"M"} and set(tx[:ov]) == {"M"}, "both ends of an overlap are M runs"
            fwd = hb + tb[ov:]
        R = len(fwd)
        h_qs, h_qe = 0, len(hb)
        t_qs, t_qe = h_qe + gap, R
        seq = revcomp(fwd) if flip else fwd
        r = case.read(R, seq)
        a_ts, a_runs = self.side(A, ra, hs, he, hx)
        b_ts, b_runs = self.side(B, rb, ts, te, tx)
        if not flip:
            case.hit(r, A, h_qs, a_runs, rev=bool(ra), ts=a_ts)
            case.hit(r, B, t_qs, b_runs, rev=bool(rb), ts=b_ts)
        else:
            case.hit(r, B, R - t_qe, b_runs, rev=not rb, ts=b_ts)
            case.hit(r, A, R - h_qe, a_runs, rev=not ra, ts=a_ts)
        cut = max(0, -gap) // 2     # what the front half's overlap trim takes from each alignment
        m = {"read": r, "flip": flip, "hs": hs, "he": he - cut, "hx": hx[:len(hx) - cut], "h_qs": h_qs, "ts": ts + cut, "te": te, "tx": tx[cut:],
             "t_qe": t_qe, "what": what, "trimmed": cut > 0}
        self.pending.setdefault((A, ra, B, rb), []).append(m)
        return m

    def triple(self, X, rx, M, rm, Z, rz, xs, xx, mx, zx, ov, flip):
        """a read over three contigs of a path, X from path column xs, the whole of M, Z from its first column, neighbours overlapping
        by ov read bases: the front half trims the middle alignment on BOTH sides, so that as the tail of X -> M and as the head of
        M -> Z its walk starts at an end where q_start / t_start (or q_end / t_end) no longer match the CIGAR's first (last) op"""
        case = self.case
        assert X < M < Z and ov % 2 == 0 and ov > 0
        cut = ov // 2
        for e in (xx[-cut - 1:], mx[:cut + 1], mx[-cut - 1:], zx[:cut + 1]):
            assert set(e) == {"M"}, "what the trim takes, and the base it stops on, are M"
        (xb, xe), (mb, me), (zb, ze) = self.bases(X, rx, xs, xx), self.bases(M, rm, 0, mx), self.bases(Z, rz, 0, zx)
        assert me == case.contigs[M][0] - 1, "an interior hit covers its contig (Longread.cpp:207)"
        fwd = xb + mb[ov:] + zb[ov:]
        R = len(fwd)
        q = [(0, len(xb)), (len(xb) - ov, len(xb) - ov + len(mb)), (R - len(zb), R)]
        r = case.read(R, revcomp(fwd) if flip else fwd)
        parts = [(X, rx, xs, xe, xx), (M, rm, 0, me, mx), (Z, rz, 0, ze, zx)]
        hits = []
        for (c, rev, ps, pe, exp), (qs, qe) in zip(parts, q):
            ts, runs = self.side(c, rev, ps, pe, exp)
            hits.append((c, qs if not flip else R - qe, runs, bool(rev) != flip, ts))
        for c, qs, runs, rev, ts in (hits[::-1] if flip else hits):
            case.hit(r, c, qs, runs, rev=rev, ts=ts)
        mid = {"hs": cut, "he": me - cut, "hx": mx[cut:len(mx) - cut], "h_qs": q[1][0] + cut, "ts": cut, "te": me - cut, "tx": mx[cut:len(mx) - cut],
               "t_qe": q[1][1] - cut}
        first = {"read": r, "flip": flip, "what": None, "trimmed": True, "hs": xs, "he": xe - cut, "hx": xx[:len(xx) - cut], "h_qs": 0,
                 "ts": mid["ts"], "te": mid["te"], "tx": mid["tx"], "t_qe": mid["t_qe"]}
        second = {"read": r, "flip": flip, "what": None, "trimmed": True, "hs": mid["hs"], "he": mid["he"], "hx": mid["hx"], "h_qs": mid["h_qs"],
                  "ts": cut, "te": ze, "tx": zx[cut:], "t_qe": R}
        self.pending.setdefault((X, rx, M, rm), []).append(first)
        self.pending.setdefault((M, rm, Z, rz), []).append(second)

    def plain(self, A, ra, B, rb, n=3, gap=50, span=600):
        """n supports over the last `span` path columns of A and the first of B"""
        LA = self.case.contigs[A][0]
        g = self.case.seq(gap)
        for k in range(n):
            self.support(A, ra, B, rb, LA - span, "M" * span, 0, "M" * span, gap, flip=k % 2 == 1, gap_seq=g)

    def chain(self, nodes, **kw):
        for (a, ra), (b, rb) in zip(nodes, nodes[1:]):
            self.plain(a, ra, b, rb, **kw)

    # ---- the model
    @staticmethod
    def walk_head(m, P1):
        lr, c = m["h_qs"], m["hs"]
        steps = 0
        for ch in m["hx"]:
            if c == P1:
                break
            lr += ch in "MI"
            c += ch in "MD"
            steps += 1
        return lr, steps

    @staticmethod
    def walk_tail(m, P2):
        lr, c = m["t_qe"] - 1, m["te"]
        steps = 0
        for ch in reversed(m["tx"]):
            if c == P2:
                break
            lr -= ch in "MI"
            c -= ch in "MD"
            steps += 1
        return lr, steps

    def close(self, key, best=None, expect_all=True):
        """finish an edge: model its coordinates into the manifest. best: indices (planting order) of the supports expected in both best
        sets when not all are; an empty list plants `supproting_lr: 0`"""
        A, ra, B, rb = key
        ms = self.pending.pop(key)
        LA, LB = self.case.contigs[A][0], self.case.contigs[B][0]
        hairpin = A == B
        e = {"n_supp": len(ms) * (2 if hairpin else 1), "what": {}, "reads": {}}
        if best is None and not hairpin:
            best = list(range(len(ms)))
        if best is not None:
            e["supporting"] = len(best)
        if best and expect_all:     # every support in both best sets: the targets are where the first head ends and the last tail begins
            P1, P2 = min(m["he"] for m in ms), max(m["ts"] for m in ms)
            assert max(m["hs"] for m in ms) <= P1 and P2 <= min(m["te"] for m in ms), "every begin precedes every end"
            e["contig1_pos"] = P1 if ra == 0 else LA - 1 - P1
            e["contig2_pos"] = P2 if rb == 0 else LB - 1 - P2
            for m in ms:
                (ls, n1), (le, n2) = self.walk_head(m, P1), self.walk_tail(m, P2)
                cases = (5 if m["flip"] else 1) + ra, (7 if m["flip"] else 3) + rb
                e["reads"][m["read"]] = (cases, ls + 1, le - 1)
                if m["what"]:
                    assert (m["what"] == "first") == (n1 == 0) == (n2 == 0), "zero steps exactly at walk position `first`"
                    e["what"][m["read"]] = (m["what"], m["trimmed"])
                self.man["census"]["empty_subseq"] += le - 1 + 1 == ls + 1
                for k in cases:
                    self.man["census"][f"case{k}"] += 1
            self.man["census"]["all_empty_edge"] += all(epos + 1 == spos for _, spos, epos in e["reads"].values())
        self.man["census"]["supporting_0"] += best == []
        self.man["census"]["hairpin"] += hairpin
        self.man["census"]["edges"] += 1
        self.man["edges"][key] = e
        return e


# =================================================================================================================================
def walk_shapes(pos, side, n=600):
    """expanded CIGAR in path order and the offset of its first column from the target column, for the head (side 1: walked along the
    path, towards the gap) or the tail (side 2: walked against the path, towards the gap)"""
    if pos == "last":        # the target is the last column the walk reaches: the end of the alignment that faces the gap
        exp, before = "M" * 300 + "I" * 2 + "M" * 150 + "D" * 3 + "M" * 150, 602
    elif pos == "first":     # the walk starts on the target column: zero steps
        exp, before = "M" * n, 0
    elif pos == "I_before":  # the walk meets an I run right before it would step onto the target column: it stops in front of the run
        exp, before = "M" * 500 + "I" * 3 + "M" * 100, 500
    elif pos == "D_before":  # a D run brings the walk onto the target column
        exp, before = "M" * 498 + "D" * 2 + "M" * 100, 500
    else:                    # the target column lies inside a D run
        exp, before = "M" * 499 + "D" * 3 + "M" * 100, 500
    cols = sum(ch in "MD" for ch in exp)
    if side == 1:
        return exp, -before, cols
    return exp[::-1], -(cols - 1 - before), cols


def add_walks(bk):
    """asm_find_lr_pos at its edges: a two-contig path for each of the four strand combinations, untrimmed and trimmed by the front
    half; on every edge each of the five walk positions on both sides, read on both strands - all eight cases of :269-324"""
    for ra, rb in itertools.product((0, 1), repeat=2):
        for ov in (0, 40):
            A, B = bk.contig(2600), bk.contig(2600)
            P1, P2 = 1500, 1000
            g = bk.case.seq(90)
            for k, pos in enumerate(WALK_POSITIONS):
                for flip in (False, True):
                    hx, d1, _ = walk_shapes(pos, 1)
                    tx, d2, _ = walk_shapes(pos, 2)
                    hs, ts = P1 + d1, P2 + d2
                    if pos == "last":
                        assert hs + sum(c in "MD" for c in hx) - 1 == P1 and ts == P2
                    if ov:   # the columns the overlap trim will take: M runs at the two ends that face the gap
                        hx, tx, ts = hx + "M" * (ov // 2), "M" * (ov // 2) + tx, ts - ov // 2
                    bk.support(A, ra, B, rb, hs, hx, ts, tx, -ov if ov else 40 + 10 * k, flip, gap_seq=g, what=pos)
            bk.close((A, ra, B, rb))
            bk.man["records"].append(1)


def add_trimmed_starts(bk):
    """paths X -> M -> Z read by reads that cover all three contigs with overlaps at both junctions: the middle alignment is trimmed on both
    sides. Its CIGAR carries an I run and a D run within the trimmed length of each cut, so that a walk which took the trimmed coordinates
    with the untrimmed CIGAR (or the other way round) would come out shifted. All strands '+' (cases 1, 3, 5, 7) and all '-'"""
    ov = 30
    for rev in (0, 1):
        X, M, Z = bk.contig(1500), bk.contig(700), bk.contig(1500)
        for k in range(4):
            near = ov // 2 + 1 + 3 * k   # after the trim 1, 4, 7, 10 M columns lie between an end of the alignment and its first indel
            mx = "M" * near + "I" * 2 + "M" * 10 + "D" * (1 + k) + "M" * 8
            mid = 700 - 2 * sum(c in "MD" for c in mx)
            mx = mx + "M" * mid + mx[::-1]
            xx = "M" * 300 + "D" * 2 + "M" * (320 + k)
            zx = "M" * (300 + 2 * k) + "I" * 3 + "M" * 330
            xs = 1500 - sum(c in "MD" for c in xx)
            bk.triple(X, rev, M, rev, Z, rev, xs, xx, mx, zx, ov, flip=k % 2 == 1)
        bk.close((X, rev, M, rev)); bk.close((M, rev, Z, rev))
        bk.man["records"].append(1)
        bk.man["trimmed_both"] = bk.man.get("trimmed_both", []) + [(X, rev, M, rev), (M, rev, Z, rev)]


def interval(bk, c, rev, lo, hi):
    """path interval [ps, pe] of the contig columns [lo, hi)"""
    L = bk.case.contigs[c][0]
    return (lo, hi - 1) if rev == 0 else (L - hi, L - 1 - lo)


def support_at(bk, A, ra, B, rb, ia, ib, gap, flip, g):
    """a support whose head covers the contig columns ia = (lo, hi) of A and whose tail covers ib of B, plain M"""
    hs, he = interval(bk, A, ra, *ia)
    ts, te = interval(bk, B, rb, *ib)
    return bk.support(A, ra, B, rb, hs, "M" * (he - hs + 1), ts, "M" * (te - ts + 1), gap, flip, gap_seq=g)


def add_empty_intersection(bk):
    """paths W -> A -> B -> Z whose middle edge has its best interval on A carried by reads 3-5 (two disjoint groups of equal support:
    the head sweep keeps the later) and its best interval on B by reads 0-2 (the tail sweep keeps the earlier): no read in both,
    `supproting_lr: 0`, head_end / tail_beg at the contigs' ends, and the stitcher breaks the path there. Once for each (rev1, rev2); the
    path through (1, 1) starts on a reverse-strand source contig"""
    for ra, rb in itertools.product((0, 1), repeat=2):
        rw = ra     # the path's first contig on A's strand: strand 1 is the reverse-strand source (:663, :693)
        W, A, B, Z = bk.contig(1500), bk.contig(2400), bk.contig(2400), bk.contig(1500)
        bk.plain(W, rw, A, ra)
        g = bk.case.seq(70)
        for k in range(6):
            early = k < 3
            ia = (200 + 10 * k, 800 + 10 * k) if early else (1300 + 10 * k, 1900 + 10 * k)
            ib = (300 + 7 * k, 900 + 7 * k) if early else (1400 + 7 * k, 2000 + 7 * k)
            support_at(bk, A, ra, B, rb, ia, ib, 70, k % 2 == 1, g)
        bk.plain(B, rb, Z, 0)
        bk.close((W, rw, A, ra)); bk.close((B, rb, Z, 0))
        e = bk.close((A, ra, B, rb), best=[])
        e["best1"], e["best2"] = (1350, 1930), (314, 900)     # last begin of the later group .. first end; last begin of the earlier ..
        bk.man["census"]["breaking"] += 1
        bk.man["records"].append(2)


def add_ties(bk):
    """the sweeps at their ties, on two-contig paths. Supports 0-2 form group 1, 3-5 group 2 (and 6-7 group 3)"""
    same = (100, 700)
    plans = {
        # two disjoint groups of equal support on contig 1, one interval on contig 2: the later group (`>=`, :45); the sweep ends with
        # the interval still open (:66-69)
        "head_later": ([(200, 800)] * 3 + [(1200, 1800)] * 3, [same] * 6, [3, 4, 5], (1200, 1800), same),
        # ... on contig 2: the earlier group (`>`, :97); the best interval is closed inside the loop (:108-112)
        "tail_earlier": ([(1700, 2300)] * 6, [(200, 800)] * 3 + [(1200, 1800)] * 3, [0, 1, 2], (1700, 2300), (200, 800)),
        # a begin equal to an end: the end is taken first (:41, :93), so the groups never count together; a third, smaller group follows,
        # so that the head sweep closes its best interval inside the loop (:56-60)
        "begin_equals_end": ([(200, 800)] * 3 + [(800, 1400)] * 3 + [(1500, 2100)] * 2, [same] * 8, [3, 4, 5], (800, 1400), same),
        "begin_equals_end_tail": ([(1700, 2300)] * 8, [(200, 800)] * 3 + [(800, 1400)] * 3 + [(1500, 2100)] * 2, [0, 1, 2], (1700, 2300), (200, 800)),
    }
    for (name, (ias, ibs, best, b1, b2)), (ra, rb) in zip(plans.items(), ((0, 0), (1, 0), (0, 1), (1, 1))):
        A, B = bk.contig(2400), bk.contig(2400)
        g = bk.case.seq(60)
        for k, (ia, ib) in enumerate(zip(ias, ibs)):
            support_at(bk, A, ra, B, rb, ia, ib, 60, k % 2 == 1, g)
        e = bk.close((A, ra, B, rb), best=best, expect_all=False)
        e["best1"], e["best2"], e["name"] = b1, b2, name
        bk.man["records"].append(1)


def add_empty_supports(bk):
    """head and tail alignment abut on the read and both walks stop at the abutting ends: lr_end == lr_start + 1, an empty sub-sequence.
    For one support of an edge; and for every support, where the consensus is empty and the stitcher joins the contigs across it
    (:709-722). Half of the abutting reads abut only after the front half trimmed an overlap"""
    for every, (ra, rb) in ((False, (0, 0)), (True, (0, 1)), (True, (1, 0))):
        A, B = bk.contig(2000), bk.contig(2000)
        g = bk.case.seq(45)
        for k in range(4):
            gap = (0 if k % 2 == 0 else -30) if every or k == 0 else 45
            hx, tx, ts = "M" * 700, "M" * 650, 300
            if gap < 0:
                hx, tx, ts = hx + "M" * 15, "M" * 15 + tx, ts - 15
            bk.support(A, ra, B, rb, 1000, hx, ts, tx, gap, k >= 2, gap_seq=g)
        bk.close((A, ra, B, rb))
        bk.man["records"].append(1)


def add_hairpins(bk):
    """an edge that is its own twin, H:+ -> H:- and H:- -> H:+: reads that run along a contig and come back on its other strand. Both
    records of a read land in the one support vector, and both push_backs of :330-331 in the one cns_supp. The contig's k-mer mean sits
    exactly on the uniqueness threshold: below it the front half cuts a read at the second hit of a contig (Longread.cpp:187-202)"""
    for rh in (0, 1):
        H = bk.contig(2400, km=fc.THR_UNIQ)
        g = bk.case.seq(80)
        for k in range(4):
            # out along the path columns [1700 + 5k, 2300], back over [0, 600 - 7k] of the other strand's path (the same contig columns)
            bk.support(H, rh, H, 1 - rh, 1700 + 5 * k, "M" * (601 - 5 * k), 99, "M" * (601 - 7 * k), 80, False, gap_seq=g)
        bk.close((H, rh, H, 1 - rh))
        bk.man["records"].append(1)


def add_shapes(bk):
    """path shapes: a node with two arcs on each side (a singleton path, :766-772) whose four arms are too long to be tips, and a cycle
    of two contigs, which asm_extract_all_simple_paths never yields: every node of it is a plain link (:761-765)"""
    X = bk.contig(1800)
    arms = [[bk.contig(1500) for _ in range(5)] for _ in range(4)]
    for k, arm in enumerate(arms):
        if k < 2:     # X -> arm
            bk.chain([(X, 0)] + [(c, k % 2) for c in arm])
        else:         # the arm leaves X through its start
            bk.chain([(X, 1)] + [(c, k % 2) for c in arm])
    for k, arm in enumerate(arms):
        nodes = [(X, 0 if k < 2 else 1)] + [(c, k % 2) for c in arm]
        for a, b in zip(nodes, nodes[1:]):
            bk.close(a + b)
    bk.man["census"]["singleton_paths"] += 1
    bk.man["records"] += [1] * 5       # X alone, and its four arms
    C1, C2 = bk.contig(1600), bk.contig(1600)
    bk.plain(C1, 0, C2, 0)
    bk.plain(C1, 1, C2, 1)      # C2:+ -> C1:+, seen from its lower vertex
    bk.close((C1, 0, C2, 0)); bk.close((C1, 1, C2, 1))
    bk.man["cycle"] = (C1, C2)


def add_back(case):
    bk = Back(case)
    add_walks(bk)
    add_trimmed_starts(bk)
    add_empty_intersection(bk)
    add_ties(bk)
    add_empty_supports(bk)
    add_hairpins(bk)
    add_shapes(bk)
    assert not bk.pending
    c = bk.man["census"]
    c["could_not_extract"] = c["wrapped_subseq"] = 0
    c["records"] = sum(bk.man["records"])
    c["simple_paths"] = len(bk.man["records"])


fc.ADD["back"] = add_back


def build(out_dir, seed=1):
    """the `back` family as a data set of its own; -> (file prefix, Case)"""
    return fc.build(out_dir, ["back"], seed)
