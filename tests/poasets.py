"""A seeded corpus of POA input sets whose graphs are NOT near-chains: the shapes on which the kernels' tie rules, in-degree limits and
wide-row pools decide the result. Every other POA input of the suite is uniform random ACGT with independent noise and at most 6
members per set; there end-node ties are rare and never large, no node has more than a handful of in-edges, and a wrong tie-break
mostly goes unseen (tests/test_poa_hard_ref.py measures both corpora).

    FAMILIES    {family name: list of sets}; a set is a list of strings, aligned in the given order
    CORPUS      [(family, index in the family, set)] over all families, in a fixed order
    SLOW_SETS   the sets that take seconds each in the CPU restatements (kept apart: one pass each)

Everything is a pure function of the seeds below (random.Random: random(), randrange(), choice() and shuffle() give the same streams on
every Python 3). Every set is a legal input of every entry point: at least one member, members of 1 to 1 200 characters."""
import random

ACGT = "ACGT"


def _rand(rnd, n, letters=ACGT):
    return "".join(rnd.choice(letters) for _ in range(n))


def _noisy(rnd, t, err, letters=ACGT):
    """copy of t with deletions, substitutions and insertions at rate err / 3 each, never empty"""
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


def _other(rnd, c):
    return rnd.choice([b for b in ACGT if b != c])


def homopolymers(rnd, n_sets=36):
    """runs of one letter whose lengths differ between the members: every run end is a choice between equally good gap placements"""
    sets = []
    for k in range(n_sets):
        n_runs = rnd.choice([1, 2, 3, 8, 20, 60])
        runs, last = [], ""
        for _ in range(n_runs):
            b = rnd.choice([x for x in ACGT if x != last])
            runs.append((b, rnd.randrange(1, 14)))
            last = b
        members = []
        for _ in range(rnd.randrange(2, 25)):
            members.append("".join(b * max(1, ln + rnd.choice([-2, -1, 0, 0, 0, 1, 2, 3])) for b, ln in runs))
        sets.append(members)
    return sets


def tandem_repeats(rnd, n_sets=36):
    """a unit of 1-6 bases, repeated a number of times that differs between the members, between random flanks"""
    sets = []
    for k in range(n_sets):
        unit = _rand(rnd, rnd.randrange(1, 7))
        left, right = _rand(rnd, rnd.choice([0, 3, 20, 80])), _rand(rnd, rnd.choice([0, 3, 20, 80]))
        base = rnd.randrange(2, 60)
        members = []
        for _ in range(rnd.randrange(2, 30)):
            s = left + unit * max(1, base + rnd.randrange(-6, 7)) + right
            members.append(_noisy(rnd, s, 0.03) if rnd.random() < 0.4 else s)
        sets.append(members)
    return sets


def two_letters(rnd, n_sets=36):
    """templates and noise over two letters only: half of all mismatching placements score alike"""
    sets = []
    for k in range(n_sets):
        letters = "".join(rnd.sample(ACGT, 2))
        t = _rand(rnd, rnd.choice([3, 10, 40, 120, 300, 600]), letters)
        sets.append([_noisy(rnd, t, rnd.choice([0.05, 0.15, 0.3]), letters) for _ in range(rnd.randrange(2, 41))])
    return sets


def unrelated(rnd, n_sets=24):
    """members that share nothing: the graph is what mismatches and gaps make of them"""
    return [[_rand(rnd, rnd.randrange(3, rnd.choice([12, 60, 250, 500]))) for _ in range(rnd.randrange(2, 20))] for _ in range(n_sets)]


def haplotypes(rnd, n_sets=36):
    """two haplotypes (substitutions, a deleted and an inserted block between them) in an exact half / half split: the heaviest bundle
    meets equal weights at every difference; in blocks, alternating, or shuffled"""
    sets = []
    for k in range(n_sets):
        a = _rand(rnd, rnd.choice([20, 80, 250, 700]))
        b = list(a)
        for _ in range(rnd.randrange(1, 6)):
            p = rnd.randrange(len(b))
            b[p] = _other(rnd, b[p])
        b = "".join(b)
        if rnd.random() < 0.5 and len(b) > 30:
            p = rnd.randrange(5, len(b) - 12)
            b = b[:p] + b[p + rnd.randrange(1, 8):]
        if rnd.random() < 0.5:
            p = rnd.randrange(len(b))
            b = b[:p] + _rand(rnd, rnd.randrange(1, 8)) + b[p:]
        half = rnd.randrange(1, 21)
        err = rnd.choice([0, 0, 0.02, 0.08])
        ma = [_noisy(rnd, a, err) if err else a for _ in range(half)]
        mb = [_noisy(rnd, b, err) if err else b for _ in range(half)]
        order = k % 3
        if order == 0:
            members = ma + mb
        elif order == 1:
            members = [x for pair in zip(mb, ma) for x in pair]
        else:
            members = ma + mb
            rnd.shuffle(members)
        sets.append(members)
    return sets


def fragments(rnd, n_sets=36):
    """prefixes, suffixes and inner pieces of one template, shortest first: the graph grows at both ends and a global alignment of a
    longer piece has many equally good sinks to end on"""
    sets = []
    for k in range(n_sets):
        t = _rand(rnd, rnd.choice([30, 100, 400, 800]))
        members = []
        for _ in range(rnd.randrange(3, 41)):
            kind, n = rnd.randrange(3), rnd.randrange(3, len(t) + 1)
            p = 0 if kind == 0 else len(t) - n if kind == 1 else rnd.randrange(0, len(t) - n + 1)
            piece = t[p:p + n]
            members.append(_noisy(rnd, piece, 0.04) if rnd.random() < 0.3 else piece)
        members.sort(key=len)
        sets.append(members)
    return sets


def fan_in(rnd):
    """150 or more members of (random prefix + shared core) and of (core with a random insert in its middle): the first core node and
    the node after the insert collect an in-edge per distinct neighbour, beyond the 16 that the direction bytes hold"""
    sets = []
    for n_members, max_prefix, core_len in ((150, 40, 60), (200, 25, 40), (160, 60, 90)):
        core = _rand(rnd, core_len)
        sets.append([_rand(rnd, rnd.randrange(1, max_prefix)) + core for _ in range(n_members)])
    for n_members, max_insert, core_len in ((150, 30, 80), (180, 12, 50)):
        core = _rand(rnd, core_len)
        h = core_len // 2
        sets.append([core[:h] + _rand(rnd, rnd.randrange(1, max_insert)) + core[h:] for _ in range(n_members)])
    core = _rand(rnd, 50)
    sets.append([_rand(rnd, rnd.randrange(1, 30)) + core + _rand(rnd, rnd.randrange(1, 30)) for _ in range(150)])
    return sets


def prefix_mismatch_set(rnd, length, others=1, shuffled=False):
    """a template T and the members T[:n] + (a base other than T[n]): every member ends on a fresh sink beside T[n], and a later member's
    last column finds the sinks of the earlier ones"""
    t = _rand(rnd, length)
    members = []
    for n in range(3, length):
        bases = [b for b in ACGT if b != t[n]]
        rnd.shuffle(bases)
        members += [t[:n] + b for b in bases[:others]]
    if shuffled:
        rnd.shuffle(members)
    return [t] + members


def prefix_mismatch(rnd):
    return [prefix_mismatch_set(rnd, 300), prefix_mismatch_set(rnd, 300, 3, True), prefix_mismatch_set(rnd, 120, 2, True)]


def many_members(rnd):
    """100-400 noisy copies of one template"""
    return [[_noisy(rnd, t, err) for _ in range(n)] for t, err, n in ((_rand(rnd, 150), 0.1, 400), (_rand(rnd, 300), 0.06, 150), (_rand(rnd, 60), 0.2, 250),
                                                                      (_rand(rnd, 500), 0.03, 100))]


def other_letters(rnd, n_sets=24):
    """lower case (read as upper case) and letters other than ACGT (read as A): lower-case copies, N runs, IUPAC codes and punctuation"""
    sets = []
    for k in range(n_sets):
        t = _rand(rnd, rnd.choice([5, 40, 150, 400]))
        members = []
        for _ in range(rnd.randrange(2, 12)):
            s = list(_noisy(rnd, t, 0.06))
            kind = rnd.randrange(4)
            if kind == 0:
                s = [c.lower() for c in s]
            elif kind == 1:
                p = rnd.randrange(len(s))
                s[p:p + rnd.randrange(1, 10)] = "N" * rnd.randrange(1, 10)
            elif kind == 2:
                for _ in range(1 + len(s) // 10):
                    s[rnd.randrange(len(s))] = rnd.choice("NRYKMSWBDHVUnacgt-*.")
            members.append("".join(s))
        sets.append(members)
    return sets


WALK_EDGE_LENGTHS = (63, 64, 65, 127, 128, 129)


def walk_edges(rnd):
    """second members whose traceback meets the walk's edges, around the 64 entries the tile walk (kernels/poa_traceback.inl) keeps in registers
    before it stores them: per template t of n bases (an A, random bases, an A or a T: a "CG" before or behind it matches nothing at its ends)
    [t, t] a walk of exactly n entries to the origin; [t, "CG" + t] n entries, then two columns left in the virtual row; [t, t[2:]] a walk that
    ends through two vertical moves into a source; [t, t + "CG"] a walk that starts with horizontal moves"""
    sets = []
    for n in WALK_EDGE_LENGTHS:
        t = "A" + _rand(rnd, n - 2) + rnd.choice("AT")
        sets += [[t, t], [t, "CG" + t], [t, t[2:]], [t, t + "CG"]]
    return sets


def as_read(seq):
    """the sequence as every entry point reads it: A, C, G, T in either case are those letters, every other character is an A (the
    reference's table: Compressed_sequence.cpp:10-19 with "& 3")"""
    return "".join(c.upper() if c in "ACGTacgt" else "A" for c in seq)


def _build():
    fam = {}
    for seed, (name, fn) in enumerate([("homopolymers", homopolymers), ("tandem_repeats", tandem_repeats), ("two_letters", two_letters), ("unrelated", unrelated),
                                       ("haplotypes", haplotypes), ("fragments", fragments), ("fan_in", fan_in), ("prefix_mismatch", prefix_mismatch),
                                       ("many_members", many_members), ("other_letters", other_letters)]):
        fam[name] = fn(random.Random(7100 + seed))
    fam["walk_edges"] = walk_edges(random.Random(7311))   # (appended last, a seed of its own: the families above keep their streams and their places in CORPUS)
    return fam


FAMILIES = _build()
CORPUS = [(name, k, st) for name, sets in FAMILIES.items() for k, st in enumerate(sets)]
SLOW_SETS = [prefix_mismatch_set(random.Random(7201), 1200)]   # (the seed: a tie of 12 candidates; most seeds stay at 6-9)


def sub_sample(step, offset=0):
    """every step-th set of the corpus, starting at offset: at least one set of every family with step <= 3"""
    return CORPUS[offset::step]
