"""tests/reclib.py pinned to the oracle, which is itself pinned to the reference: the oracle's forward edge records of a simulated
data set, packed and put through reclib.expect, are the oracle's own edge output; pack and unpack invert each other on the extreme
values; and every generator's manifest holds at every size the GPU tests use (test_edge_records_gpu.py)."""
import numpy as np
import pytest

import orclib
import reclib
from haslr_amd import host

SIM_ARGS = ("--genome-len", "150000", "--seed", "21", "--variant-per-mb", "30")   # the first of test_gpu_parity.CASES


def oracle_edges(pre):
    """the oracle's edge stage on a data set: (edges_out() with sides, its forward records in emission order)"""
    ds = host.Dataset(pre + ".contigs.fa", pre + ".reads.fa", pre + ".paf")
    be = orclib.OracleBackend(ds, 4)
    run = host.Run(ds, ds.params(), be.table, None)
    run.chain()
    run.graph()
    edges = run.edges_out()
    run.close(); be.close(); ds.close()
    fwd = reclib.forward(edges)
    order = np.lexsort((fwd["cmp_head"], fwd["lr"]))   # read ascending, pair ascending
    return edges, {k: v[order] for k, v in fwd.items()}


def test_restatement_equals_the_oracle(sim):
    edges, fwd = oracle_edges(sim(*SIM_ARGS))
    assert len(fwd["key"]) > 1000 and 2 * len(fwd["key"]) == len(edges["key"])
    exp = reclib.expect(reclib.pack(fwd))
    assert set(exp) == set(edges)
    for k in edges:
        assert exp[k].dtype == edges[k].dtype and np.array_equal(exp[k], edges[k]), k


@pytest.mark.parametrize("n_contigs", reclib.N_CONTIGS)
def test_pack_and_unpack_invert_each_other_on_the_extremes(n_contigs):
    words, man = reclib.extremes(n_contigs, 256)
    reclib.check(words, man, n_contigs)
    assert man["extreme_rows"] == 6
    rec = reclib.unpack(words)
    assert np.array_equal(reclib.pack(reclib.forward(rec)), words)
    again = reclib.unpack(reclib.pack(reclib.forward(rec)))
    for k in rec:
        assert np.array_equal(again[k], rec[k]), k
    # spot values, spelled out: the twin of the second row
    vmax = 2 * n_contigs - 1
    assert int(rec["key"][3]) == (1 << 32) | (vmax ^ 1) and int(rec["lr"][3]) == 0xffffffff
    assert int(rec["tail_cg_begin"][3]) == (1 << 40) + 5 and int(rec["tail_cg_end"][3]) == (1 << 40) + 5 + 0xffffffff
    assert int(rec["head_is_rev"][3]) == 0 and int(rec["tail_is_rev"][3]) == 1 and int(rec["cmp_head"][3]) == 65535


@pytest.mark.parametrize("n_contigs", reclib.N_CONTIGS)
def test_every_manifest_holds_at_the_small_sizes(n_contigs):
    for n in reclib.SMALL_N:
        for name, gen, kw in reclib.patterns(n_contigs):
            words, man = gen(n_contigs, n, **kw)
            assert reclib.check(words, man, n_contigs), (name, n)
            again, _ = gen(n_contigs, n, **kw)
            assert np.array_equal(words, again), (name, n, "not deterministic")
    # what the sizes are there for, spelled out once
    passes = {1: 1, 128: 1, 129: 2, 32768: 2, 32769: 3, (1 << 23) + 1: 4}[n_contigs]
    assert reclib.n_passes(n_contigs) == passes
    assert len([p for p in reclib.patterns(n_contigs) if p[0].startswith("one_digit")]) == 2 * passes + 1
    if n_contigs > 1:
        _, man = reclib.boundaries(n_contigs, 8194)
        assert {0, 1, 1023, 1024, 1025, 2047, 2048, 4096, 8193} <= set(man["starts"])
    words, _ = reclib.one_key(n_contigs, 8194)
    exp, rec = reclib.expect(words), reclib.unpack(words)
    assert len(exp["edge_key"]) == 1 and all(np.array_equal(exp[k], rec[k]) for k in rec)   # one edge, in import order
    if n_contigs in (128, 32768):   # the top digit is full: 255 is reached
        _, man = reclib.digit_edges(n_contigs, 2050, p=passes - 1)
        assert man["rare"] == 255


@pytest.mark.parametrize("n_contigs", reclib.LARGE_N_CONTIGS)
def test_every_manifest_holds_at_the_large_sizes(n_contigs):
    for n in reclib.LARGE_N:
        for name, gen, kw in reclib.patterns(n_contigs, large=True):
            words, man = gen(n_contigs, n, **kw)
            assert reclib.check(words, man, n_contigs), (name, n)
    _, man = reclib.boundaries(n_contigs, (1 << 20) + 1030)
    assert {(1 << 20) - 1, 1 << 20, (1 << 20) + 1} <= set(man["starts"])
    _, man = reclib.boundaries(n_contigs, 1 << 20)
    assert (1 << 20) - 1 in man["starts"]
