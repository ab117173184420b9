"""The seeded inputs of the exhaustive reference (tests/exhlib.py): the smallest shapes at which the loops over a row's predecessors and
the start and end rules of the general POA path can go wrong, each with so few source-to-sink paths per add (at most exhlib.CAP) that
every path can be scored by a pairwise DP. Everything is a pure function of the seeds below.

    TINY        40 sets: a template of 8-16 bases, 4-7 members at 18 % substitutions, one-base insertions and deletions; a third of the
                members lose 0-2 bases at either end, so that local and overlap graphs get several sources and sinks
    FAN_IN      four sets: all four letters at one column, deletions of 1, 2 and 3 bases and an insertion (or a deletion of 4 bases) in
                front of the same next node: in every set that node collects 7 predecessors or more
    LONG_GAPS   deletions and insertions of 5-12 bases across a bubble of substitutions: under scores such as (5, -4, -8, -6, -24, -1)
                the second convex piece wins, and the vertical gap passes nodes with several predecessors
    LANE_EDGES  longest sequences of 63, 64, 65, 129 and 257 bases (a lane of the 64-lane instance holds 16 columns), at most 6 variant
                sites: the first and the last column, one of columns 62-65 and one of 127-128 where the length reaches them, the rest
                drawn from a pool of lane edges
    WIDTHS      one set per workgroup width: (lanes, model, longest sequence, type, set), the shortest longest sequence that selects the
                width (tests/test_poa_phase_gpu.py, WIDTHS), 3 members, at most 3 variant sites
    CORPUS      the sets of poasets.CORPUS named in CORPUS_UNDER_CAP, those whose every add stays under the cap under every type and score
                set below (113 of 265), less the eight of CORPUS_TOO_SLOW, left out by name for their cost
    SCORES      the ten score sets: grflib's three defaults; unit scores, (2, -3, -5, -1), and two convex sets whose second piece opens dear and
                extends at -1, (3, -5, -4, -3, -9, -1) and (5, -4, -8, -6, -24, -1); three of gscorelib (mismatch 0, nothing positive, the ends
                of int8)"""
import random

import grflib
import gscorelib
import poasets

ACGT = "ACGT"
MODES = ["sw", "nw", "ov"]
MODELS = ["linear", "affine", "convex"]
SCORES = [grflib.LINEAR, grflib.AFFINE, grflib.CONVEX,
          (1, -1, -1, -1, -1, -1), (2, -3, -5, -1, -5, -1), (3, -5, -4, -3, -9, -1), (5, -4, -8, -6, -24, -1),
          gscorelib.scores_of("mismatch_0", "convex"), gscorelib.scores_of("nothing_positive", "affine"), gscorelib.scores_of("int8_ends", "linear")]
SCORES_OF_MODEL = {name: [s for s in SCORES if grflib.model_of(s) == k] for k, name in enumerate(MODELS)}
assert all(len(v) >= 3 for v in SCORES_OF_MODEL.values())


def _rand(rnd, n):
    return "".join(rnd.choice(ACGT) for _ in range(n))


def _other(rnd, c):
    return rnd.choice([b for b in ACGT if b != c])


def _edited(rnd, t, rate):
    """a copy of t with substitutions, one-base insertions and one-base deletions at `rate` in all, never empty"""
    out = []
    for c in t:
        r = rnd.random()
        if r < rate / 3:
            continue
        if r < 2 * rate / 3:
            out.append(_other(rnd, c))
        elif r < rate:
            out.append(c + rnd.choice(ACGT))
        else:
            out.append(c)
    return "".join(out) or t[:1]


def tiny(seed, n_sets=40):
    rnd = random.Random(seed)
    sets = []
    for _ in range(n_sets):
        t = _rand(rnd, rnd.randrange(8, 17))
        members = []
        for _ in range(rnd.randrange(4, 8)):
            q = _edited(rnd, t, 0.18)
            if rnd.random() < 1 / 3:
                a, b = rnd.randrange(0, 3), rnd.randrange(0, 3)
                q = q[a:len(q) - b] or q
            members.append(q)
        sets.append(members)
    return sets


def fan_in_set(rnd, length=22, ins=True):
    """template t, column c in its middle: t, the three other letters at c, t without its 1, 2 and 3 bases in front of c + 1, and (ins) t
    with a base inserted in front of c + 1, or (not ins) t without its 4 bases in front of c + 1: seven predecessors of c + 1 either way"""
    t = _rand(rnd, length)
    c = length // 2
    while len(set(t[c - 4:c + 3])) < 4 or t[c] == t[c + 1]:   # (the deleted bases and their neighbours differ: a deletion has one best place)
        t = _rand(rnd, length)
    members = [t] + [t[:c] + b + t[c + 1:] for b in ACGT if b != t[c]] + [t[:c + 1 - d] + t[c + 1:] for d in ((1, 2, 3) if ins else (1, 2, 3, 4))]
    if ins:
        members.append(t[:c + 1] + _other(rnd, t[c + 1]) + t[c + 1:])
        members.append(t[:c] + _other(rnd, t[c]) + _other(rnd, t[c + 1]) + t[c + 1:])
    return members


def fan_in(seed):
    rnd = random.Random(seed)
    return [fan_in_set(rnd, 22, True), fan_in_set(rnd, 22, False), fan_in_set(rnd, 30, True), fan_in_set(rnd, 17, True)]


def long_gap_set(rnd):
    """a template of 36-48 bases; two members with 2 substitutions each inside a window of its middle (the bubble), then members that delete or
    insert 5-12 bases inside or across that window, some with a substitution of their own"""
    n = rnd.randrange(36, 49)
    t = _rand(rnd, n)
    lo, hi = n // 2 - 7, n // 2 + 7
    members = [t]
    for _ in range(2):
        q = list(t)
        for p in rnd.sample(range(lo, hi), 2):
            q[p] = _other(rnd, q[p])
        members.append("".join(q))
    for kind in ("del", "ins", "del"):
        q = list(members[rnd.randrange(len(members[:3]))])
        k, p = rnd.randrange(5, 13), rnd.randrange(lo, hi - 4)
        if kind == "del":
            q[p:p + k] = []
        else:
            q[p:p] = list(_rand(rnd, k))
        members.append("".join(q))
    return members


def long_gaps(seed, n_sets=8):
    rnd = random.Random(seed)
    return [long_gap_set(rnd) for _ in range(n_sets)]


LANE_LENGTHS = (63, 64, 65, 129, 257)
SITE_POOL = (0, 1, 15, 16, 17, 31, 32, 47, 48, 62, 63, 64, 65, 127, 128, 255, 256)   # (and the last column of every length, below)


LANE_EDGE_COLUMNS = ((62, 63, 64, 65), (127, 128))   # the columns either side of the 64-lane instance's lanes 3 | 4 and 7 | 8, as sequence positions and as matrix columns


def lane_edge_set(rnd, length, members=5, n_sites=6):
    """(the set, the sites at which a member differs from the template). A template of `length` bases; at most n_sites sites of the pool
    that lie inside it: always the first and the last column and one of each group of LANE_EDGE_COLUMNS that lies inside, the rest drawn;
    per site ONE alternative (another letter, or the base deleted), which a member takes with probability 1/2 and the member behind the
    template always at the forced ones: at most 2 ^ n_sites paths, and a few more where two sites touch. The template itself comes
    second, so that the longest sequence is aligned and not only added; where the first member lacks a base, the template meets an
    insertion."""
    t = _rand(rnd, length)
    pool = sorted(set(p for p in SITE_POOL if 0 < p < length - 1))
    forced = [0, length - 1] + [rnd.choice([p for p in grp if p in pool]) for grp in LANE_EDGE_COLUMNS if any(p in pool for p in grp)]
    rest = [p for p in pool if p not in forced]
    sites = sorted(forced + rnd.sample(rest, min(n_sites - len(forced), len(rest))))
    alt = {}
    for p in sites:
        kind = rnd.choice(["sub", "del"]) if 0 < p < length - 1 else "sub"
        alt[p] = _other(rnd, t[p]) if kind == "sub" else ""
    out, varied = [], set()
    for k in range(members):
        take = set() if k == 1 else set(forced) | {p for p in sites if rnd.random() < 0.5} if k == 2 else {p for p in sites if rnd.random() < 0.5}
        varied |= take
        out.append("".join(alt[p] if p in take else c for p, c in enumerate(t)))
    return out, sorted(varied)


def lane_edges(seed):
    rnd = random.Random(seed)
    made = [lane_edge_set(rnd, n) for n in LANE_LENGTHS for _ in range(2)]
    sets = [st for st, _ in made]
    assert [max(len(q) for q in st) for st in sets] == [n for n in LANE_LENGTHS for _ in range(2)]
    for st, varied in made:   # every set varies at its first and last column and at a lane-edge column of every group its length reaches
        n = max(len(q) for q in st)
        assert 0 in varied and n - 1 in varied and len(varied) <= 6
        assert all(any(p in varied for p in grp) for grp in LANE_EDGE_COLUMNS if n - 1 >= grp[0])
    return sets


# (lanes, model, the longest sequence, type): the table of tests/test_poa_phase_gpu.py, one line per width (the 64-lane instance once)
WIDTH_TABLE = [(64, "convex", 149, "ov"), (128, "convex", 1024, "nw"), (256, "linear", 1024, "ov"), (512, "affine", 4096, "nw"), (1024, "linear", 8192, "nw")]


LANES = {"linear": (64, 256, 256, 1024), "affine": (64, 256, 512, 1024), "convex": (64, 128, 256, 512)}   # per instance of gscorelib.COLUMNS


def lanes_of(longest, model):
    """the workgroup width of the instance that holds a longest sequence"""
    return LANES[model][gscorelib.COLUMNS[model].index(gscorelib.columns_of(["A" * longest], model))]


def width_set(rnd, length):
    """3 members over a template of `length` bases with 3 variant sites (substitutions and one deleted base, so that the template, which
    comes second, stays the longest): at most 8 paths in front of the third member"""
    t = _rand(rnd, length)
    sites = sorted(rnd.sample(range(length // 8, length - length // 8), 3))
    a, b = list(t), list(t)
    a[sites[0]] = _other(rnd, t[sites[0]])
    a[sites[1]] = ""
    b[sites[1]] = _other(rnd, t[sites[1]])
    b[sites[2]] = _other(rnd, t[sites[2]])
    b[sites[0]] = a[sites[0]]
    return ["".join(a), t, "".join(b)]


def widths(seed):
    rnd = random.Random(seed)
    out = [(lanes, model, lmax, mode, width_set(rnd, lmax)) for lanes, model, lmax, mode in WIDTH_TABLE]
    for lanes, model, lmax, _, st in out:   # the set selects the width, and a longest sequence of one base less a narrower one
        assert max(len(q) for q in st) == lmax and lanes_of(lmax, model) == lanes and (lanes == 64 or lanes_of(lmax - 1, model) < lanes)
    return out


TINY = tiny(9107)
FAN_IN = fan_in(9102)
LONG_GAPS = long_gaps(9101)
LANE_EDGES = lane_edges(9103)
WIDTHS = widths(9105)

# the sets of poasets.CORPUS whose every add stays under the cap under every type and score set above, by (family, index): 113 of its 265
# sets. The list was made by counting (not enumerating) the paths of every add of every set of the corpus under the 30 combinations, which
# takes ten minutes and is therefore no test; tests/test_poa_exhaustive_ref.py asserts that every set named here does stay under the cap.
CORPUS_UNDER_CAP = [("homopolymers", 0), ("homopolymers", 4), ("homopolymers", 5), ("homopolymers", 6), ("homopolymers", 7), ("homopolymers", 8),
                    ("homopolymers", 13), ("homopolymers", 14), ("homopolymers", 15), ("homopolymers", 16), ("homopolymers", 17),
                    ("homopolymers", 18), ("homopolymers", 19), ("homopolymers", 20), ("homopolymers", 22), ("homopolymers", 24),
                    ("homopolymers", 25), ("homopolymers", 26), ("homopolymers", 27), ("homopolymers", 31), ("homopolymers", 32),
                    ("homopolymers", 33), ("homopolymers", 34), ("homopolymers", 35), ("tandem_repeats", 2), ("tandem_repeats", 4),
                    ("tandem_repeats", 6), ("tandem_repeats", 7), ("tandem_repeats", 15), ("tandem_repeats", 17), ("tandem_repeats", 19),
                    ("tandem_repeats", 22), ("tandem_repeats", 26), ("tandem_repeats", 31), ("tandem_repeats", 34), ("two_letters", 2),
                    ("two_letters", 5), ("two_letters", 10), ("two_letters", 12), ("two_letters", 14), ("two_letters", 16), ("two_letters", 17),
                    ("two_letters", 18), ("two_letters", 21), ("two_letters", 23), ("two_letters", 24), ("unrelated", 11), ("unrelated", 18),
                    ("unrelated", 21), ("haplotypes", 0), ("haplotypes", 1), ("haplotypes", 2), ("haplotypes", 3), ("haplotypes", 6),
                    ("haplotypes", 7), ("haplotypes", 8), ("haplotypes", 10), ("haplotypes", 16), ("haplotypes", 17), ("haplotypes", 18),
                    ("haplotypes", 20), ("haplotypes", 21), ("haplotypes", 22), ("haplotypes", 23), ("haplotypes", 24), ("haplotypes", 26),
                    ("haplotypes", 27), ("haplotypes", 28), ("haplotypes", 29), ("haplotypes", 30), ("haplotypes", 31), ("haplotypes", 33),
                    ("haplotypes", 35), ("fragments", 2), ("fragments", 5), ("fragments", 17), ("other_letters", 0), ("other_letters", 3),
                    ("other_letters", 4), ("other_letters", 5), ("other_letters", 9), ("other_letters", 10), ("other_letters", 14),
                    ("other_letters", 16), ("other_letters", 18), ("other_letters", 19), ("other_letters", 20), ("other_letters", 21),
                    ("other_letters", 22)] + [("walk_edges", k) for k in range(24)]
# the eight of them that are left out for their cost, by name: haplotypes of 12-38 members of 700 bases, with the seconds that the restatement
# and the path count alone took per set over the 30 combinations (on a shared CPU; the pairwise DP over 700 x 700 cells x up to 64 paths x up
# to 37 adds comes on top). A test here has a few seconds for all of its sets. The 700-base pair haplotypes 3 and the six sets of 250 bases stay.
CORPUS_TOO_SLOW = {("haplotypes", 0): 20.4, ("haplotypes", 7): 27.1, ("haplotypes", 8): 51.1, ("haplotypes", 17): 80.9, ("haplotypes", 18): 91.3,
                   ("haplotypes", 21): 93.6, ("haplotypes", 27): 87.2, ("haplotypes", 29): 44.5}
assert all(c in CORPUS_UNDER_CAP for c in CORPUS_TOO_SLOW)
CORPUS = [(f, k, st) for f, k, st in poasets.CORPUS if (f, k) in set(CORPUS_UNDER_CAP) and (f, k) not in CORPUS_TOO_SLOW]
assert len(CORPUS) == len(CORPUS_UNDER_CAP) - len(CORPUS_TOO_SLOW) == 105

# [(family, index in the family, set)]: what every type and score set is tried on (the width sets run under their own model and type)
INPUTS = ([("tiny", k, st) for k, st in enumerate(TINY)] + [("fan_in", k, st) for k, st in enumerate(FAN_IN)] + [("long_gaps", k, st) for k, st in enumerate(LONG_GAPS)]
          + [("lane_edges", k, st) for k, st in enumerate(LANE_EDGES)] + [("corpus:" + f, k, st) for f, k, st in CORPUS])
# the sets that meet no graph: an empty set, empty members, a single member
EXCLUDED = [("excluded", k, st) for k, st in enumerate([[], [""], ["", "ACGT", "", "ACGA", ""], ["ACGTTGCA"], ["", ""]])]

COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def rc(s):
    return "".join(COMP[grflib.read(c)] for c in reversed(s))


def half_reversed(sets):
    """the sets with every second member after the first reverse-complemented: both orientations win in turn"""
    return [[rc(q) if k % 2 == 1 else q for k, q in enumerate(st)] for st in sets]


# the corpus sets that the strand-ambiguous inputs leave out, by name. fragments 2: with every second member reverse-complemented its graph
# is another one, and one add meets more than 2 048 paths (kNW, the convex defaults). The others for their cost, with the seconds the strand
# restatement and both optima took per set under one type and score set, single-threaded (all other corpus sets together: 0.5 s; a strand
# test runs three to ten score sets and has a few seconds for all of its sets)
STRAND_LEFT_OUT = {("fragments", 2): None, ("haplotypes", 35): 0.71, ("tandem_repeats", 6): 0.28, ("haplotypes", 10): 0.28, ("haplotypes", 31): 0.24,
                   ("tandem_repeats", 2): 0.21, ("haplotypes", 20): 0.18, ("tandem_repeats", 17): 0.13}
assert all(c in CORPUS_UNDER_CAP for c in STRAND_LEFT_OUT)
STRAND_INPUTS = [(f, k, st) for (f, k, _), st in zip(INPUTS, half_reversed([st for _, _, st in INPUTS])) if (f.replace("corpus:", ""), k) not in STRAND_LEFT_OUT or not f.startswith("corpus:")] + EXCLUDED
