"""Seeded POA input sets for the unrestricted heaviest-bundle pass of the tuned kernel (kernels/poa_graph.inl, bundle_pass_free: 64 ranks at
a time; a rank whose heaviest in-edge stands alone at its weight takes it without looking at a score and its score follows by pointer
jumping along the chosen in-edges inside the chunk; a rank whose maximal weight is shared by several in-edges - a TIED rank - waits for
its sources' scores and is finished in rank order). Every family is built around one thing that pass can get wrong.
tests/test_poa_bundle_ref.py states each family's premise on the CPU, from the restatement's final graph and a plain forward pass over it;
tests/test_poa_bundle_gpu.py runs the same sets through the kernel.

    BUILT   [(family, name, set)]; a set is a list of 2-8 upper-case ACGT strings of at most 700 bases, aligned in the given order

Everything is a pure function of the seed below."""
import random

MAX_READS, MAX_LEN = 8, 700
CHUNK = 64
CHAIN_NODES = (1, 63, 64, 65, 128, 129)
FAMILIES = ("asym_bubble", "bubble_run", "chain", "fallback", "mid_source", "sym_bubble", "wide_row")


def _rand(rnd, n, letters="ACGT"):
    return "".join(rnd.choice(letters) for _ in range(n))


def _other(rnd, c, but=""):
    return rnd.choice([b for b in "ACGT" if b != c and b not in but])


def _plain(rnd, n):
    """n random bases without two equal neighbours: a deleted or inserted base has one place to go"""
    out = [rnd.choice("ACGT")]
    while len(out) < n:
        out.append(_other(rnd, out[-1]))
    return "".join(out)


def chains(rnd):
    """identical reads: a graph of exactly n nodes, every rank with one in-edge from the rank before it - a chunk is one chain of 64 links,
    which takes all six jumping rounds; 1, 63 .. 129 nodes end a chunk one short of, at and one past its last lane"""
    out = [("chain", "nodes_%d" % n, [t] * rnd.choice([2, 3])) for n in CHAIN_NODES for t in [_rand(rnd, n)]]
    t = _rand(rnd, 230)
    return out + [("chain", "nodes_230", [t, t])]


def _bubble(rnd, length, at, len_a, len_b, reads=(2, 2)):
    """two reads through branch a, then two through branch b, between a shared prefix and a shared suffix: the node after the bubble
    has two in-edges of one weight, a's first"""
    t = _plain(rnd, length)
    a = _plain(rnd, len_a)
    b = "".join(_other(rnd, c) for c in a[:len_b]) if len_b <= len_a else None
    assert b is not None
    ra, rb = t[:at] + a + t[at:], t[:at] + b + t[at:]
    return [ra] * reads[0] + [rb] * reads[1]


def symmetric_bubbles(rnd):
    """branches of equal length: equal weights and equal source scores, the later in-edge wins (spoa's <=)"""
    out = []
    for k, (length, at, n) in enumerate(((40, 20, 1), (90, 61, 1), (150, 64, 2), (150, 63, 3), (200, 126, 1), (70, 5, 2))):
        out.append(("sym_bubble", "sym_%d" % k, _bubble(rnd, length, at, n, n)))
    return out


def asymmetric_bubbles(rnd):
    """the first branch is the longer one: equal weights into the node after the bubble, and the EARLIER in-edge's source scores more"""
    out = []
    for k, (length, at, la, lb) in enumerate(((40, 20, 2, 1), (90, 60, 3, 1), (150, 63, 3, 2), (200, 127, 2, 1), (140, 70, 4, 2))):
        out.append(("asym_bubble", "asym_%d" % k, _bubble(rnd, length, at, la, lb)))
    return out


def bubble_runs(rnd):
    """a substitution site every 7-11 bases, at each of them two of the four reads (chosen anew) carry the other letter: a tied rank every
    few ranks, each with tied ranks among its ancestors, on both sides of whatever rank a chunk begins at"""
    out = []
    for k, length in enumerate((240, 420, 640, 700, 699, 655)):
        t = _plain(rnd, length)
        reads = [list(t) for _ in range(4)]
        at = rnd.randrange(3, 9)
        while at < length - 3:
            alt = _other(rnd, t[at], but=t[at - 1] + t[at + 1])
            for r in rnd.sample(range(4), 2):
                reads[r][at] = alt
            at += rnd.randrange(7, 12)
        out.append(("bubble_run", "run_%d" % length if k < 4 else "run_%d_%d" % (length, k), ["".join(r) for r in reads]))
    return out


def wide_rows(rnd):
    """reads that lack 4, 3, 2, 1 and 0 bases in front of one node, in that order: the node collects five in-edges of one weight and the
    fifth - from the node right before it - has the source that scores most; with the first and the last read twice, two in-edges of weight 4
    stand at the first and the fifth place; six and seven in-edges likewise"""
    out = []
    for k, (length, h, dels) in enumerate(((60, 30, (4, 3, 2, 1, 0)), (120, 64, (4, 3, 2, 1, 0, 4, 0)), (150, 70, (6, 5, 4, 3, 2, 1, 0)),
                                           (150, 66, (5, 4, 3, 2, 1, 0, 5, 0)), (100, 40, (0, 1, 2, 3, 4)), (200, 130, (1, 2, 3, 4, 5, 0, 3, 5)))):
        t = _plain(rnd, length)
        out.append(("wide_row", "wide_%d" % k, [t[:h - d] + t[h:] for d in dels]))
    return out


def mid_order_sources(rnd):
    """a shared core behind prefixes of different lengths, by turns of A / C and of G / T so that the second read's cannot join the first's
    (and, in two sets, in front of unrelated tails): a later prefix starts on a node without in-edges that the rank order puts between the
    nodes of the earlier ones"""
    out = []
    for k, (core, prefixes, tails) in enumerate(((80, (30, 12, 45), (0, 0, 0)), (150, (70, 5, 64, 20), (0, 0, 0, 0)), (60, (100, 130, 90), (0, 9, 4)),
                                                 (200, (10, 66, 3, 129, 40), (0, 0, 7, 0, 0)))):
        c = _rand(rnd, core)
        out.append(("mid_source", "prefixes_%d" % k, [_rand(rnd, p, ("AC", "GT")[i % 2]) + c + _rand(rnd, q) for i, (p, q) in enumerate(zip(prefixes, tails))]))
    return out


def fallbacks(rnd):
    """the heaviest node is not a sink (a long body L under two reads, then three reads of a short other start and the shared tail Z: Z's
    first node takes the heavier in-edge and scores less than L's end), and two equally heavy ends (the reads differ in their last letters)"""
    out = []
    for k, (body, start, tail) in enumerate(((200, 5, 10), (130, 3, 20), (300, 8, 6))):
        L, S, Z = _rand(rnd, body, "ACG"), "T" * start, _rand(rnd, tail)   # (the other start shares no letter with the body: it joins none of its nodes)
        out.append(("fallback", "inner_max_%d" % k, [L + Z, L + Z, S + Z, S + Z, S + Z]))
    for k, (length, ends) in enumerate(((50, ("A", "C")), (127, ("GA", "GC", "GA", "GC")), (64, ("A", "C", "G")), (190, ("AC", "CA")))):
        t = _plain(rnd, length)
        out.append(("fallback", "two_ends_%d" % k, [t + e for e in ends]))
    return out


def _build():
    rnd = random.Random(90417)
    return chains(rnd) + symmetric_bubbles(rnd) + asymmetric_bubbles(rnd) + bubble_runs(rnd) + wide_rows(rnd) + mid_order_sources(rnd) + fallbacks(rnd)


BUILT = _build()


def forward_pass(order, in_edges):
    """spoa's traverse_heaviest_bundle forward pass. order: node ids in a topological order; in_edges[n]: [(source, weight)] in in-edge order.
    Returns (score, pred) by node: the in-edge that is heavier wins, among equally heavy ones the source that scores at least as much (the
    later one on a full tie); a node without in-edges scores -1"""
    score, pred = {}, {}
    for n in order:
        s, p = -1, -1
        for f, w in in_edges[n]:
            if s < w or (s == w and score[p] <= score[f]):
                s, p = w, f
        score[n], pred[n] = (s + score[p] if p != -1 else s), p
    return score, pred


def chunked_pass(order, in_edges, offset=0):
    """the scheme of bundle_pass_free on the same input, in chunks of 64 ranks of which the first holds 64 - offset (the order shifted by
    `offset` ranks). Returns (score, pred, rounds per chunk, tied ranks per chunk)."""
    rank = {n: r + offset for r, n in enumerate(order)}
    at = {r: n for n, r in rank.items()}
    score, pred, rounds, tied = {}, {}, [], []
    for r0 in range(0, len(order) + offset, CHUNK):
        lanes = [at[r] for r in range(r0, r0 + CHUNK) if r in at]
        val, link, pending = {}, {}, []
        for n in lanes:                                     # load + classify: no score of this chunk is looked at
            es = in_edges[n]
            if not es:
                val[n], link[n], pred[n] = -1, None, -1
                continue
            wmax = max(w for _, w in es)
            top = [f for f, w in es if w == wmax]
            if len(top) > 1:
                pending.append(n)
                val[n], link[n] = 0, None
            elif rank[top[0]] < r0:
                val[n], link[n], pred[n] = wmax + score[top[0]], None, top[0]
            else:
                val[n], link[n], pred[n] = wmax, top[0], top[0]
        k = 0
        while True:                                         # jump: every lane looks at the lane it hangs off, all at once
            nv, nl, changed = dict(val), dict(link), False
            for n in lanes:
                if link[n] is not None and link[n] not in pending:
                    nv[n], nl[n], changed = val[n] + val[link[n]], link[link[n]], True
            if not changed:
                break
            val, link, k = nv, nl, k + 1
            assert k <= 6
        rounds.append(k)
        tied.append(len(pending))
        for n in pending:                                   # the tied ranks, in rank order
            es = in_edges[n]
            wmax = max(w for _, w in es)
            bs, bp = None, -1
            for f, w in es:
                if w != wmax:
                    continue
                assert rank[f] < r0 or link[f] is None     # every source has its score by now
                s = score[f] if rank[f] < r0 else val[f]
                if bs is None or s >= bs:
                    bs, bp = s, f
            val[n], pred[n] = wmax + bs, bp
            for m in lanes:                                 # the lanes that hang off it
                if link[m] == n:
                    val[m], link[m] = val[m] + val[n], None
        for n in lanes:
            assert link[n] is None
            score[n] = val[n]
    return score, pred, rounds, tied
