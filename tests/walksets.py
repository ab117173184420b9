"""Seeded POA input sets for the direction-nibble traceback of kernels/poa.hip: the walk through tiles of 64 rows x 32 columns whose moves
all lanes decode into a table before the walk starts. Every set is built so that its LAST alignment takes the walk somewhere particular -
tile entries at odd and even columns, a first tile of fewer than 32 columns, vertical runs longer than a tile's rows, horizontal runs across
the tile's columns and the rotation of the table's registers, tiles left through their rows, moves into a third or later predecessor, rows
with more than 4 predecessors, the tail in the virtual row 0. tests/test_poa_walk_tiles_ref.py checks that premise on the CPU restatement
(premise_holds: what the last alignment must look like); tests/test_poa_walk_tiles_gpu.py runs the same sets through the kernel.

    BUILT       [(family, name, set, premise)]; a set is a list of 3-5 upper-case ACGT strings, aligned in the given order
    corpus_picks(stats)   the sets of poasets.CORPUS chosen for later predecessors and for wide rows, from the restatement's statistics

Everything is a pure function of the seeds below."""
import random

import poasets

SHORT_LENGTHS = (1, 2, 30, 31, 32, 33, 63, 64, 65, 95, 96, 97, 129)
ACG = "ACG"   # the templates of the insertion families have no T: a run of T matches nothing


def _rand(rnd, n, letters="ACGT"):
    return "".join(rnd.choice(letters) for _ in range(n))


def _noisy(rnd, t, err, letters="ACGT"):
    """copy of t with deletions, substitutions and insertions at rate err / 3 each; never empty"""
    out = []
    for c in t:
        r = rnd.random()
        if r < err / 3:
            continue
        if r < 2 * err / 3:
            out.append(rnd.choice(letters))
        elif r < err:
            out.append(c + rnd.choice(letters))
        else:
            out.append(c)
    return "".join(out) or t[:1]


def short_templates(rnd):
    """template, two noisy copies, the template again: the last alignment pairs every base of the template with a node"""
    out = []
    for n in SHORT_LENGTHS:
        t = _rand(rnd, n)
        out.append(("short", "len_%d" % n, [t, _noisy(rnd, t, 0.12), _noisy(rnd, t, 0.12), t], ("all_pairs", n)))
    return out


def long_deletions(rnd):
    """the last read lacks 70 / 140 bases of the template's middle: a run of nodes without a base longer than one / two tiles' rows. (The
    lost stretch is all T in a template of A, C and G, and the copies carry it unchanged: no base of the last read can sit inside it, so
    the gap is not taken apart by the ties of a linear gap score.)"""
    out = []
    for cut, run in ((70, 65), (140, 129)):
        head, tail = _rand(rnd, 100, ACG), _rand(rnd, 220 - cut, ACG)
        t = head + "T" * cut + tail
        copies = [_noisy(rnd, head, 0.06, ACG) + "T" * cut + _noisy(rnd, tail, 0.06, ACG) for _ in range(2)]
        out.append(("deletion", "cut_%d" % cut, [t] + copies + [head + tail], ("node_run", run)))
    return out


def long_insertions(rnd):
    """the last read carries 40 / 100 T in a template without T: a run of bases without a node across the tiles' columns"""
    out = []
    for ins in (40, 100):
        t = _rand(rnd, 200, ACG)
        last = t[:90] + "T" * ins + t[90:]
        copies = [_noisy(rnd, t[:60], 0.06, ACG) + t[60:120] + _noisy(rnd, t[120:], 0.06, ACG) for _ in range(2)]   # (no spare node next to the run for a T to sit on)
        out.append(("insertion", "ins_%d" % ins, [t] + copies + [last], ("base_run", ins)))
    return out


def three_letter_branches(rnd):
    """`every_3rd`: three reads with three different letters at every 3rd position, the third read again. `dense`: four reads with four
    different letters at two of every three positions, the fourth again - more than two ranks per column, so that the walk leaves its
    tiles of 64 rows x 32 columns through their rows. The premise asks for the nodes: at least 4 / 3 and 2 per column."""
    out = []
    for name, branched, shifts, floor in (("every_3rd", (0,), (0, 1, 2), 4 / 3), ("dense", (0, 1), (0, 1, 2, 3), 2)):
        n = 240
        t = _rand(rnd, n)
        reads = ["".join("ACGT"[("ACGT".index(c) + shift) % 4] if p % 3 in branched else c for p, c in enumerate(t)) for shift in shifts]
        out.append(("branch", name, reads + [reads[-1]], ("pairs_nodes", n, int(floor * n))))
    return out


def row0_tail(rnd):
    """the last read begins with 50 bases the graph does not have: the walk ends in the virtual row 0 with 50 columns left"""
    t = _rand(rnd, 150, ACG)
    copies = [t[:30] + _noisy(rnd, t[30:], 0.06, ACG) for _ in range(2)]   # (no spare node at the graph's beginning for a T to sit on)
    return [("row0", "lead_50", [t] + copies + ["T" * 50 + t], ("lead", 50))]


def _build():
    rnd = random.Random(9051)
    return short_templates(rnd) + long_deletions(rnd) + long_insertions(rnd) + three_letter_branches(rnd) + row0_tail(rnd)


BUILT = _build()

# corpus sets small enough to look at one by one (bases in the set), and how many of each kind are taken
CORPUS_MAX_BASES = 12000
CORPUS_TAKE = 4
CANDIDATES = [(f, k, [poasets.as_read(q) for q in st]) for f, k, st in poasets.CORPUS if sum(len(q) for q in st) <= CORPUS_MAX_BASES]


def corpus_picks(stats):
    """stats: the restatement's statistics of CANDIDATES, in order. -> (later, wide): up to CORPUS_TAKE sets each whose graph has a row with a
    third or fourth predecessor but none with more than 4, and whose graph has rows with more than 4 (most wide rows first)"""
    later = [c for c, s in zip(CANDIDATES, stats) if s["max_in_degree"] in (3, 4) and s["wide_rows"] == 0]
    wide = [c for _, c in sorted(((-s["wide_rows"], k), c) for k, (c, s) in enumerate(zip(CANDIDATES, stats)) if s["wide_rows"] > 0 and s["max_in_degree"] <= 16)]
    return later[:CORPUS_TAKE], wide[:CORPUS_TAKE]


def longest_run(flags):
    best = cur = 0
    for f in flags:
        cur = cur + 1 if f else 0
        best = max(best, cur)
    return best


def premise_holds(premise, aln):
    """aln: the last alignment as (node | -1, position | -1) pairs, first column first"""
    kind = premise[0]
    pairs = sum(1 for a, b in aln if a >= 0 and b >= 0)
    if kind == "all_pairs":   # every base of the last read on a node (nodes the noisy copies added are passed without a base)
        return pairs == premise[1] and all(a >= 0 for a, _ in aln)
    if kind == "pairs_nodes":   # ... and the graph has at least premise[2] nodes: the last read walks its own, which were added last
        return pairs == premise[1] and all(a >= 0 for a, _ in aln) and max(a for a, _ in aln) + 1 >= premise[2]
    if kind == "node_run":
        return longest_run(a >= 0 and b < 0 for a, b in aln) >= premise[1]
    if kind == "base_run":
        return longest_run(a < 0 and b >= 0 for a, b in aln) >= premise[1]
    if kind == "lead":
        return [(a, b) for a, b in aln[:premise[1]]] == [(-1, p) for p in range(premise[1])] and aln[premise[1]][0] >= 0
    raise ValueError(kind)
