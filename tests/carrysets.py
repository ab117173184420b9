"""Seeded POA input sets for the carry hand-over of the wave pipeline (kernels/poa_dp.inl, dp_rows: a wave takes the carries of its left
neighbour a batch of rows at a time - at least CARRY_MIN, at most CARRY_BATCH, never across a record batch of 64 rows - out of a mailbox of
WAVE_MBOX entries whose producer must not lap its consumer). Every set is built so that its LAST alignment has a particular number of graph
rows and so many columns that the cluster shapes of test_poa_hard_gpu.SHAPES run several waves, and several members, with real columns.
tests/test_poa_carry_batches_ref.py checks that premise on the CPU restatement and by plain arithmetic;
tests/test_poa_carry_batches_gpu.py runs the same sets through the kernel.

    BUILT   [(family, name, set, premise)]; a set is a list of 3-6 upper-case ACGT strings, aligned in the given order
            premise = ("rows", n): the graph has exactly n rows when the last read is aligned; ("rows_between", lo, hi); the families
            `sit_out` and `first_longest` carry what their reads' lengths must be

Everything is a pure function of the seed below."""
import random

# the constants of kernels/poa_dp.inl the sets are built around
CARRY_MIN, CARRY_BATCH, RECORD_BATCH, WAVE_MBOX = 4, 32, 64, 64
SMALL_ROWS = (1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 128, 129)
# columns per wave and per member of the three cluster shapes whose members are narrower than these reads (test_poa_hard_gpu.SHAPES:
# poa_member_lanes x poa_cluster_cols), and the most members each may have (poa_cluster_max)
CLUSTER_SHAPES = {"cluster_64x8": (64 * 8, 64 * 8, 8), "cluster_128x4": (64 * 4, 128 * 4, 4), "cluster_256x2": (64 * 2, 256 * 2, 8)}
MIN_LEN, MAX_LEN = 600, 1100


def _rand(rnd, n, letters="ACGT"):
    return "".join(rnd.choice(letters) for _ in range(n))


def _noisy(rnd, t, err):
    """copy of t with deletions, substitutions and insertions at rate err / 3 each; never empty"""
    out = []
    for c in t:
        r = rnd.random()
        if r < err / 3:
            continue
        if r < 2 * err / 3:
            out.append(rnd.choice("ACGT"))
        elif r < err:
            out.append(c + rnd.choice("ACGT"))
        else:
            out.append(c)
    return "".join(out) or t[:1]


def small_graphs(rnd):
    """a template of n bases twice - a graph of exactly n nodes - and then a long read that has a stretch of the template in it: n rows
    around CARRY_MIN, CARRY_BATCH and the record batch of 64, under 600-1100 columns"""
    out = []
    for k, n in enumerate(SMALL_ROWS):
        t = _rand(rnd, n)
        length = (MIN_LEN + 1, 777, 1023, 1024, 1025, MAX_LEN, 640, 897)[k % 8]
        at = rnd.randrange(0, length - n)
        body = _rand(rnd, length)
        last = body[:at] + t + body[at + n:]
        out.append(("small", "rows_%d" % n, [t, t, last], ("rows", n)))
    return out


def wrapping_graphs(rnd):
    """about 700 and about 1 500 rows under reads of 600-1 100 bases: the mailbox of 64 entries wraps ten and twenty times, a cached
    "consumed" count is refreshed and reused. (The 1 500 rows come from two halves that share only their middle: the reads stay short.)"""
    t = _rand(rnd, 690)
    a = [t, _noisy(rnd, t, 0.04), _noisy(rnd, t, 0.04), _noisy(rnd, t, 0.10) + _rand(rnd, 150)]
    u = _rand(rnd, 1500)
    b = [u[:1000], u[500:], _noisy(rnd, u[:1000], 0.04), _noisy(rnd, u[450:], 0.04), _noisy(rnd, u[200:1270], 0.08)]
    return [("wrap", "rows_700", a, ("rows_between", 10 * WAVE_MBOX + 1, 800)), ("wrap", "rows_1500", b, ("rows_between", 20 * WAVE_MBOX + 1, 1900))]


def sitting_out(rnd):
    """long, short, long: the waves beyond the short read's columns sit its DP out and come back for the next one, whose carries run under
    tags that went on counting meanwhile"""
    t = _rand(rnd, 1000)
    st = [t, _noisy(rnd, t[:100], 0.05), _noisy(rnd, t, 0.06), _noisy(rnd, t[:96], 0.05), _noisy(rnd, t, 0.06)]
    return [("sit_out", "long_short_long", st, ("lengths", "LSLSL"))]


def first_longest(rnd):
    """the first read is the longest: the pipeline is sized by a read every later alignment is narrower than"""
    t = _rand(rnd, MAX_LEN)
    st = [t, _noisy(rnd, t[:900], 0.06), _noisy(rnd, t[100:800], 0.06), _noisy(rnd, t[:MIN_LEN + 30], 0.06)]
    return [("first_longest", "longest_first", st, ("lengths", "first"))]


def _build():
    rnd = random.Random(40617)
    return small_graphs(rnd) + wrapping_graphs(rnd) + sitting_out(rnd) + first_longest(rnd)


BUILT = _build()


def rows_of_last_alignment(cells_all, cells_but_last, last_len):
    """graph rows under the last read, from the restatement's cell counts (sums of rows x columns over the alignments)"""
    assert (cells_all - cells_but_last) % last_len == 0
    return (cells_all - cells_but_last) // last_len


def pipeline_of(length, shape):
    """(waves, members) with at least one real column - columns 0 .. length - of a read under a cluster shape"""
    per_wave, per_member, _ = CLUSTER_SHAPES[shape]
    ncol = length + 1
    return -(-ncol // per_wave), -(-ncol // per_member)


def mailbox_wraps(rows):
    return rows // WAVE_MBOX
