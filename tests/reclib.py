"""Builder and plain restatement for the edge-record kernels (kernels/edges.hip, kernels/primitives.hip): the packed exchange layout,
what hx_edge_records_import must return for any packed input, and seeded generators of inputs the simulator never produces. numpy
only, no GPU.

The packed layout (include/haslr_hip.h, the comment block above pack_side in edges.hip): a forward record and its twin travel as one
unit of 22 dwords.
   0    low half of the forward key  = the vertex entered at the tail anchor (v2 = contig << 1 | is_rev)
   1    high half of the forward key = the vertex left at the head anchor   (v1)
   2    long-read id                 3    cmp_head | cmp_tail << 16
   4-12 head anchor, 13-21 tail anchor: q_start, q_end, t_start, t_end, cg_begin low, cg_begin high, cg_end - cg_begin, cg_skip_front,
        cg_skip_back
The twin's key is ((v2 ^ 1) << 32) | (v1 ^ 1), its read id has bit 31 set, its head and tail are the forward record's tail and head;
an anchor's is_rev is the low bit of its key half in the forward record, in both records.

A pair's two records cannot be chosen independently, which shapes the generators: a hairpin pair (v1 = t, v2 = t ^ 1) is the only
kind whose two records share a key, so runs of equal keys in import order have even length, and a key with an odd number of records
needs a second key (its twin's) with the same number.

Every generator returns (words, manifest); `check` recomputes from the words what the manifest claims, so that a builder change cannot
quietly turn a case into one that tests nothing. Vertices are always below 2 * n_contigs (the sort ignores higher bits) and read ids
below 2^31.
"""
import random
import zlib

import numpy as np

WORDS = 22
M32 = np.uint64(0xffffffff)
U32MAX = 0xffffffff
FIELDS32 = ("q_start", "q_end", "t_start", "t_end", "cg_skip_front", "cg_skip_back")
SIDE_WORD = {"q_start": 0, "q_end": 1, "t_start": 2, "t_end": 3, "cg_skip_front": 7, "cg_skip_back": 8}   # word of an anchor; 4, 5, 6: the CIGAR range


def n_bits(n_contigs):
    """key bits the sort looks at in each half (hx_api.hip, finish_edges)"""
    bits = 1
    while bits < 32 and (1 << bits) < 2 * max(1, n_contigs):
        bits += 1
    return bits


def n_passes(n_contigs):
    """radix passes per key half, 8 bits each"""
    return (n_bits(n_contigs) + 7) // 8


# =====================================================================================================================
# layout
# =====================================================================================================================
def pack(pairs):
    """forward records (dict of arrays as hx_edges_out names them: key, lr, cmp_head, cmp_tail, head_* and tail_*) -> uint32[P, 22].
    is_rev is not stored: it is the low bit of the anchor's key half."""
    key = np.asarray(pairs["key"], dtype=np.uint64)
    w = np.zeros((len(key), WORDS), dtype=np.uint32)
    w[:, 0] = (key & M32).astype(np.uint32)
    w[:, 1] = (key >> np.uint64(32)).astype(np.uint32)
    w[:, 2] = pairs["lr"]
    w[:, 3] = np.asarray(pairs["cmp_head"], dtype=np.uint32) | (np.asarray(pairs["cmp_tail"], dtype=np.uint32) << np.uint32(16))
    for side, base in (("head_", 4), ("tail_", 13)):
        for f, k in SIDE_WORD.items():
            w[:, base + k] = pairs[side + f]
        cb, ce = np.asarray(pairs[side + "cg_begin"], dtype=np.uint64), np.asarray(pairs[side + "cg_end"], dtype=np.uint64)
        w[:, base + 4] = (cb & M32).astype(np.uint32)
        w[:, base + 5] = (cb >> np.uint64(32)).astype(np.uint32)
        w[:, base + 6] = ((ce - cb) & M32).astype(np.uint32)
    return w


def unpack(words):
    """uint32[P, 22] -> the 2P records in import order (forward, twin, forward, twin ...), named as hx_edges_out names them"""
    w = np.asarray(words, dtype=np.uint32).reshape(-1, WORDS)
    n = 2 * len(w)
    v2, v1 = w[:, 0].astype(np.uint64), w[:, 1].astype(np.uint64)
    one = np.uint64(1)
    r = {"key": np.zeros(n, np.uint64), "lr": np.zeros(n, np.uint32), "cmp_head": np.zeros(n, np.uint32), "cmp_tail": np.zeros(n, np.uint32)}
    r["key"][0::2] = (v1 << np.uint64(32)) | v2
    r["key"][1::2] = ((v2 ^ one) << np.uint64(32)) | (v1 ^ one)
    r["lr"][0::2] = w[:, 2]
    r["lr"][1::2] = w[:, 2] | np.uint32(0x80000000)
    ih, it = w[:, 3] & np.uint32(0xffff), w[:, 3] >> np.uint32(16)
    r["cmp_head"][0::2], r["cmp_head"][1::2] = ih, it
    r["cmp_tail"][0::2], r["cmp_tail"][1::2] = it, ih
    # the forward record's head is words 4-12 and its tail words 13-21; the twin's head is 13-21 and its tail 4-12
    for base, rev, fwd_side, twin_side in ((4, v1 & one, "head_", "tail_"), (13, v2 & one, "tail_", "head_")):
        cb = w[:, base + 4].astype(np.uint64) | (w[:, base + 5].astype(np.uint64) << np.uint64(32))
        vals = {f: w[:, base + k] for f, k in SIDE_WORD.items()}
        vals.update(is_rev=rev.astype(np.uint8), cg_begin=cb, cg_end=cb + w[:, base + 6].astype(np.uint64))
        for f, v in vals.items():
            for side, start in ((fwd_side, 0), (twin_side, 1)):
                r.setdefault(side + f, np.zeros(n, v.dtype))[start::2] = v
    return r


def forward(rec):
    """the forward records of a record set, in its order"""
    keep = rec["lr"] < np.uint32(0x80000000)
    return {k: v[keep] for k, v in rec.items() if k not in ("edge_key", "edge_off")}


def expect(words):
    """what hx_edge_records_import returns for these packed records: every field in the stable order of the keys, the distinct keys
    and where their runs start (plus n)"""
    rec = unpack(words)
    order = np.argsort(rec["key"], kind="stable")
    out = {k: v[order] for k, v in rec.items()}
    key = out["key"]
    n = len(key)
    starts = np.flatnonzero(np.concatenate(([True], key[1:] != key[:-1]))) if n else np.zeros(0, np.int64)
    out["edge_key"] = key[starts]
    out["edge_off"] = np.concatenate((starts, [n])).astype(np.uint64)
    return out


# =====================================================================================================================
# generators
# =====================================================================================================================
def _rng(name, n_contigs, n, seed):
    return np.random.default_rng([seed, zlib.crc32(name.encode()), n_contigs, n])


def payload(rng, P):
    """P pairs with pseudo-random words 2-21 and distinct read ids below 2^31; the keys are still to be set"""
    w = rng.integers(0, 1 << 32, size=(P, WORDS), dtype=np.uint64).astype(np.uint32)
    first = int(rng.integers(0, 1 << 31))
    w[:, 2] = ((np.arange(P, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(first)) & np.uint64(0x7fffffff)).astype(np.uint32)   # odd multiplier: a bijection
    return w


def _with_keys(w, v1, v2):
    w[:, 1], w[:, 0] = np.asarray(v1, dtype=np.uint32), np.asarray(v2, dtype=np.uint32)
    return w


def _digit_range(n_contigs, d):
    """(largest value of 8-bit digit d of a vertex, largest value the bits below it may take when the digit is at its largest)"""
    V, npass = 2 * n_contigs, n_passes(n_contigs)
    if d < npass - 1:
        return 255, (1 << (8 * d)) - 1
    return (V - 1) >> (8 * d), (V - 1) & ((1 << (8 * d)) - 1)


def uniform(n_contigs, n, seed=1):
    rng = _rng("uniform", n_contigs, n, seed)
    P, V = n // 2, 2 * n_contigs
    w = _with_keys(payload(rng, P), rng.integers(0, V, P), rng.integers(0, V, P))
    return w, {"n": n, "varied_passes": P >= 64}


def one_key(n_contigs, n, seed=1):
    """every pair the hairpin of the last contig: n records, one edge, and the expected order is the import order"""
    rng = _rng("one_key", n_contigs, n, seed)
    P, V = n // 2, 2 * n_contigs
    w = _with_keys(payload(rng, P), np.full(P, V - 2), np.full(P, V - 1))
    return w, {"n": n, "n_keys": min(1, P), "identity_order": True}


TWO_KEY_PERIODS = (1, 63, 64, 65, 255, 256, 257, 2047, 2048)   # in pairs: the runs are twice as many records


def two_keys(n_contigs, n, seed=1, period=1):
    """two hairpin keys, `period` pairs of one, then `period` pairs of the other"""
    rng = _rng(f"two_keys{period}", n_contigs, n, seed)
    P, V = n // 2, 2 * n_contigs
    ta, tb = V - 1, int(rng.integers(0, V - 1))
    t = np.where((np.arange(P) // period) % 2 == 0, ta, tb)
    w = _with_keys(payload(rng, P), t, t ^ 1)
    return w, {"n": n, "n_keys": min(2, -(-P // period)), "import_run": 2 * period}


def descending(n_contigs, n, seed=1):
    """keys in descending import order: all distinct while the vertices last (n <= 2 n_contigs), else every vertex's hairpin key in turn"""
    rng = _rng("descending", n_contigs, n, seed)
    P, V = n // 2, 2 * n_contigs
    if n <= V:
        u = V - 1 - np.arange(n)
        v1, v2, nk = u[0::2], u[1::2] ^ 1, n          # forward (u0, u1 ^ 1) > twin (u1, u0 ^ 1) > next forward (u2, ...)
    else:
        v1 = V - 1 - (np.arange(P) * V) // P
        v2, nk = v1 ^ 1, min(P, V)
    return _with_keys(payload(rng, P), v1, v2), {"n": n, "n_keys": nk, "non_increasing": True}


def one_digit(n_contigs, n, seed=1, p=0):
    """keys that differ only inside one digit. p < passes: the tail vertex varies in digit p, so the forward keys differ in pass p of the
    low half and the twins in pass p of the high half; p >= passes: the head vertex varies in digit p - passes, the mirror image.
    p = "strand": the tail vertex varies in bit 0 only."""
    rng = _rng(f"one_digit{p}", n_contigs, n, seed)
    P, V, npass = n // 2, 2 * n_contigs, n_passes(n_contigs)
    const = np.full(P, int(rng.integers(0, V)))
    if p == "strand":
        d, tail = 0, True
        vary = (int(rng.integers(0, V)) & ~1) | rng.integers(0, 2, P)
    else:
        d, tail = p % npass, p < npass
        top, low_max = _digit_range(n_contigs, d)
        above = ((V - 1) >> (8 * d + 8))
        base = (int(rng.integers(0, above)) << (8 * d + 8) if above else 0) | int(rng.integers(0, low_max + 1))
        vary = base | (rng.integers(0, top + 1, P) << (8 * d))
    w = _with_keys(payload(rng, P), const if tail else vary, vary if tail else const)
    return w, {"n": n, "one_digit_shift": 8 * d + (0 if tail else 32), "min_digits": 2 if P >= 8 else min(P, 1)}


def digit_edges(n_contigs, n, seed=1, p=0, reverse=False):
    """the low half's digit p is 0 in every record but a few forward ones, which hold the largest value the digit can take (255
    where the digit is full); reverse: the largest value everywhere but in a few forward records. Every other digit of the tail
    vertex is 0, and the head vertex is chosen so that the twins' low halves hold the common digit too."""
    rng = _rng(f"digit_edges{p}{reverse}", n_contigs, n, seed)
    P = n // 2
    top, _ = _digit_range(n_contigs, p)
    common, rare = (top, 0) if reverse else (0, top)
    at = sorted({0, P - 1} | set(rng.integers(0, P, 3).tolist())) if P else []
    digit = np.full(P, common)
    digit[at] = rare
    head = ((common << (8 * p)) ^ 1)   # the twin's low half is head ^ 1
    w = _with_keys(payload(rng, P), np.full(P, head), digit << (8 * p))
    return w, {"n": n, "edge_shift": 8 * p, "common": common, "rare": rare, "n_rare": len(at)}


BOUNDARY_STARTS = (1023, 1024, 1025, 2047, 2048, 4096, (1 << 20) - 1, 1 << 20, (1 << 20) + 1)


def boundary_starts(n_contigs, n):
    """the sorted indices at which `boundaries` makes an edge begin, besides 0, 1 and n - 1 (one contig has four keys: one index)"""
    return [t for t in (BOUNDARY_STARTS if n_contigs > 1 else BOUNDARY_STARTS[:1]) if t <= n - 1]


def boundaries(n_contigs, n, seed=1):
    """runs of equal keys chosen so that edges begin at the sorted indices of boundary_starts; the first and the last record are
    edges of their own. Even runs are hairpin keys; runs of one record come in twin pairs. Imported in shuffled order."""
    rng = _rng("boundaries", n_contigs, n, seed)
    P, V = n // 2, 2 * n_contigs
    want = boundary_starts(n_contigs, n)
    if P == 0:
        return payload(rng, 0), {"n": 0, "starts": []}
    cuts = sorted({0, 1, n - 1, n} | set(want))
    runs = []
    for a, b in zip(cuts, cuts[1:]):
        runs += [1, b - a - 1] if (b - a) % 2 and b - a > 1 else [b - a]
    if V == 2:                              # keys (0,0) < (0,1) < (1,0) < (1,1): the outer two are each other's twins, the inner two hairpins
        assert len(runs) <= 4 and runs[0] == runs[-1] == 1
        v1 = [0] + [0] * (runs[1] // 2 if len(runs) > 2 else 0) + [1] * (runs[2] // 2 if len(runs) > 3 else 0)
        v2 = [0] + [1] * (runs[1] // 2 if len(runs) > 2 else 0) + [0] * (runs[2] // 2 if len(runs) > 3 else 0)
    else:
        high = sorted(random.Random(int(rng.integers(0, 1 << 30))).sample(range(V), len(runs)))   # one high half per run, ascending
        single = [high[j] for j, ln in enumerate(runs) if ln == 1]
        assert len(single) % 2 == 0
        v1 = single[0::2] + [h for h, ln in zip(high, runs) if ln > 1 for _ in range(ln // 2)]
        v2 = [h ^ 1 for h in single[1::2]] + [h ^ 1 for h, ln in zip(high, runs) if ln > 1 for _ in range(ln // 2)]
    order = rng.permutation(P)
    w = _with_keys(payload(rng, P), np.array(v1, dtype=np.uint64)[order], np.array(v2, dtype=np.uint64)[order])
    return w, {"n": n, "starts": [0] + ([1] if n > 1 else []) + want + [n - 1], "n_keys": len(runs)}


# what the `extremes` payload must contain when all of its rows fit (6 pairs), per field of the record set
def extreme_values(n_contigs):
    vmax = 2 * n_contigs - 1
    d = {side + f: [0, U32MAX] for side in ("head_", "tail_") for f in FIELDS32}
    for side in ("head_", "tail_"):
        d[side + "cg_begin"] = [(1 << 32) - 1, 1 << 32, (1 << 40) + 5]
        d[side + "cg_len"] = [0, (1 << 32) - 1]
    d.update(cmp_head=[0, 9999, 65535], cmp_tail=[0, 9999, 65535], lr=[0, (1 << 31) - 1], vertex=[vmax])
    return d


def _extreme_rows(n_contigs):
    vmax, big, cap = 2 * n_contigs - 1, U32MAX, (1 << 40) + 5
    lo, hi, alt, tla = [0] * 6, [big] * 6, [0, big] * 3, [big, 0] * 3
    #        fields of head / tail   head cg_begin, len    tail cg_begin, len    cmp_head, cmp_tail   lr           v1, v2
    return [(lo, lo,                 big, 0,               1 << 32, big,         0, 0,                0,            vmax, vmax),
            (hi, hi,                 cap, big,             big, big,             65535, 65535,        (1 << 31) - 1, vmax, 0),
            (alt, tla,               1 << 32, 0,           cap, 0,               9999, 0,             (1 << 31) - 1, 0, vmax),
            (tla, alt,               0, big,               0, 0,                 0, 9999,             0,            0, 0),
            (hi, lo,                 big, big,             1 << 32, 0,           65535, 0,            1,            vmax ^ 1, vmax),
            (lo, hi,                 cap, 0,               big, 0,               0, 65535,            (1 << 31) - 2, vmax, vmax ^ 1)]


def extremes(n_contigs, n, seed=1):
    """uniform keys and a random payload whose first pairs (and, where there is room, last pairs too) are the rows of _extreme_rows:
    every 32-bit field at 0 and 0xFFFFFFFF, cg_begin at 2^32 - 1, 2^32 and 2^40 + 5, cg_end - cg_begin at 0 and 2^32 - 1, compact
    indices at 0, 9 999 and 65 535, read ids at 0 and 2^31 - 1, the largest vertex. Built as records and packed with pack()."""
    rng = _rng("extremes", n_contigs, n, seed)
    P, V = n // 2, 2 * n_contigs
    pairs = forward(unpack(_with_keys(payload(rng, P), rng.integers(0, V, P), rng.integers(0, V, P))))
    rows = _extreme_rows(n_contigs)
    where = list(range(min(P, len(rows)))) + (list(range(P - len(rows), P)) if P >= 2 * len(rows) else [])
    for i in where:
        fh, ft, hb, hl, tb, tl, ch, ct, lr, v1, v2 = rows[i % len(rows) if i < len(rows) else i - (P - len(rows))]
        for side, vals, cb, ln in (("head_", fh, hb, hl), ("tail_", ft, tb, tl)):
            for f, v in zip(FIELDS32, vals):
                pairs[side + f][i] = v
            pairs[side + "cg_begin"][i], pairs[side + "cg_end"][i] = cb, cb + ln
        pairs["cmp_head"][i], pairs["cmp_tail"][i], pairs["lr"][i], pairs["key"][i] = ch, ct, lr, (v1 << 32) | v2
    return pack(pairs), {"n": n, "extreme_rows": min(P, len(rows))}


def check(words, man, n_contigs):
    """the contract of every case (shape, vertex and read-id ranges) and what its manifest claims, recomputed from the words"""
    w = np.asarray(words)
    assert w.dtype == np.uint32 and w.ndim == 2 and w.shape[1] == WORDS
    n, V = 2 * len(w), 2 * n_contigs
    assert n == man["n"]
    assert n == 0 or (int(w[:, 0].max()) < V and int(w[:, 1].max()) < V), "a vertex outside the contract"
    assert n == 0 or int(w[:, 2].max()) < 1 << 31, "a read id with bit 31 set"
    rec = unpack(w)
    key = rec["key"]
    fwd, twin = key[0::2], key[1::2]
    skey = np.sort(key)
    starts = np.flatnonzero(np.concatenate(([True], skey[1:] != skey[:-1]))) if n else np.zeros(0, np.int64)
    if "extreme_rows" not in man:
        assert len(np.unique(w[:, 2])) == len(w), "read ids are distinct per pair"
    if "n_keys" in man:
        assert len(starts) == man["n_keys"]
    if man.get("identity_order"):
        assert np.array_equal(np.argsort(key, kind="stable"), np.arange(n))
    if man.get("varied_passes"):
        for half in (0, 32):
            for d in range(n_passes(n_contigs)):
                top, _ = _digit_range(n_contigs, d)
                if top >= 15:
                    assert len(np.unique((key >> np.uint64(half + 8 * d)) & np.uint64(255))) >= 8
    if "import_run" in man and n:
        edges = np.flatnonzero(key[1:] != key[:-1]) + 1
        runs = np.diff(np.concatenate(([0], edges, [n])))
        assert np.all(runs[:-1] == man["import_run"]) and 0 < runs[-1] <= man["import_run"]
    if man.get("non_increasing"):
        assert np.all(key[1:] <= key[:-1])
    if "one_digit_shift" in man and n:
        s = man["one_digit_shift"]
        for keys, shift in ((fwd, s), (twin, (s + 32) % 64)):
            assert not np.any((keys ^ keys[0]) & ~(np.uint64(255) << np.uint64(shift))), "keys differ outside the digit"
            assert len(np.unique((keys >> np.uint64(shift)) & np.uint64(255))) >= man["min_digits"]
    if "edge_shift" in man and n:
        dig = lambda k: (k >> np.uint64(man["edge_shift"])) & np.uint64(255)
        assert np.all(dig(twin) == man["common"])
        assert int((dig(fwd) == man["rare"]).sum()) == (man["n_rare"] if man["rare"] != man["common"] else n // 2)
        assert int((dig(fwd) == man["common"]).sum()) == (n // 2 - man["n_rare"] if man["rare"] != man["common"] else n // 2)
        assert not np.any((key & M32) & ~(np.uint64(255) << np.uint64(man["edge_shift"]))), "another digit of the low half is not 0"
    if "starts" in man and n:
        assert set(man["starts"]) <= set(starts.tolist()), sorted(set(man["starts"]) - set(starts.tolist()))
        assert starts[0] == 0 and (n == 1 or len(starts) > 1 and starts[1] == 1) and starts[-1] == n - 1   # first and last: runs of one
    if "extreme_rows" in man:
        have = {k: set(v.tolist()) for k, v in rec.items()}
        for side in ("head_", "tail_"):
            have[side + "cg_len"] = set((rec[side + "cg_end"] - rec[side + "cg_begin"]).tolist())
        have["vertex"] = set(w[:, 0].tolist()) | set(w[:, 1].tolist())
        have["lr"] = set(w[:, 2].tolist())
        if man["extreme_rows"] == len(_extreme_rows(n_contigs)):
            for f, vals in extreme_values(n_contigs).items():
                assert set(vals) <= have[f], (f, vals)
        elif n:
            assert 2 * n_contigs - 1 in have["vertex"]
    return True


def patterns(n_contigs, large=False):
    """the cases of one n_contigs: (id, generator, keyword arguments). large: the three patterns of the sizes around 2^20"""
    out = [("uniform", uniform, {}), ("one_key", one_key, {}), ("boundaries", boundaries, {})]
    if large:
        return out
    npass = n_passes(n_contigs)
    out += [(f"two_keys[{p}]", two_keys, {"period": p}) for p in TWO_KEY_PERIODS]
    out += [("descending", descending, {}), ("extremes", extremes, {})]
    out += [(f"one_digit[{p}]", one_digit, {"p": p}) for p in list(range(2 * npass)) + ["strand"]]
    out += [(f"digit_edges[{p}{'r' if rev else ''}]", digit_edges, {"p": p, "reverse": rev}) for p in range(npass) for rev in (False, True)]
    return out


GROUPS = ("uniform", "one_key", "two_keys", "descending", "one_digit", "digit_edges", "boundaries", "extremes")
N_CONTIGS = (1, 128, 129, 32768, 32769, (1 << 23) + 1)          # 1, 1, 2, 2, 3 and 4 passes per half; 128 and 32 768 fill the top digit
SMALL_N = (0, 2, 254, 256, 258, 2046, 2048, 2050, 8190, 8192, 8194)
LARGE_N = ((1 << 20) - 2, 1 << 20, (1 << 20) + 1030)
LARGE_N_CONTIGS = (129, (1 << 23) + 1)
