"""The device-wide scan, the radix sort and the edge-record kernels (kernels/primitives.hip, kernels/edges.hip) on their own, through
hx_edge_records_import / hx_edge_records_export: packed records of tests/reclib.py's generators go in, and every array that comes
back must equal reclib.expect, the plain restatement (stable argsort by key), exactly. hx_upload of a stub data set sets the number
of contigs and with it the number of radix passes. The manifests of the cases are checked on the CPU (test_edge_records_ref.py) and
again here before anything is compared.

What reaches what:
  radix passes per key half   1: n_contigs 1 and 128    2: 129 and 32 768    3: 32 769    4: 2^23 + 1
  scan depth                  1: up to 1 024 records (segment scan), up to 4 sort tiles (histogram scan)
                              2: the sizes from 2 046 to 2^20 records (2^20: the exact fit), 8 194 records (5 tiles: histogram scan)
                              3: 2^20 + 1 030 records (1 026 blocks, then 2, then 1), segment scan; the chain-side scans at
                                 2^20 + 1 030 reads (test_chain_scans_past_2_20_reads)
Not run: the third level of the histogram scan (more than 4 096 sort tiles, 8.4 M records), and the copy after an odd number of
passes at the end of radix_sort_pairs (its only caller sorts the same number of bits in both halves)."""
import ctypes as C

import numpy as np
import pytest
import torch

import frontcases as fc
import orclib
import reclib
from haslr_amd import ctypes_defs as T
from haslr_amd import hip, host
from test_edge_records_ref import SIM_ARGS, oracle_edges

pytestmark = pytest.mark.gpu
BIG = (1 << 23) + 1


class Stub:
    """a data set of n_contigs contigs, one dummy read and no hits, as hx_upload takes it"""

    def __init__(self, n_contigs):
        self._keep = [np.full(n_contigs, 30.0), np.full(n_contigs, 1000, dtype=np.uint32), np.array([4], dtype=np.uint32),
                      np.array([0, 1], dtype=np.uint64), np.array([0x1b], dtype=np.uint8), np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint8),
                      np.zeros(1, dtype=np.uint64), np.zeros(2, dtype=np.uint64)]
        km, ln, rlen, roff, packed, z32, z8, z64, rho = self._keep
        self.contigs = T.Contigs(n_contigs, km.ctypes.data_as(T.f64p), ln.ctypes.data_as(T.u32p))
        self.reads = T.Reads(1, rlen.ctypes.data_as(T.u32p), roff.ctypes.data_as(T.u64p), packed.ctypes.data_as(T.u8p))
        p32, p8 = z32.ctypes.data_as(T.u32p), z8.ctypes.data_as(T.u8p)
        self.hits = T.Hits(0, *([p32] * 9), p8, p8, z64.ctypes.data_as(T.u64p), p32)
        self.read_hit_off = rho.ctypes.data_as(T.u64p)


class Ports:
    """contexts with a stub of the wanted number of contigs resident: one for 2^23 + 1 (about 100 MB, uploaded once per module), one
    for every other number (uploaded again when the number changes)"""

    def __init__(self):
        self.small, self.small_n, self.big = hip.HipContext(0), None, None

    def at(self, n_contigs):
        if n_contigs == BIG:
            if self.big is None:
                self.big = hip.HipContext(0)
                self.big.upload(Stub(BIG))
            return self.big
        if self.small_n != n_contigs:
            self.small.upload(Stub(n_contigs))
            self.small_n = n_contigs
        return self.small

    def close(self):
        for c in (self.small, self.big):
            if c is not None:
                c.close()


@pytest.fixture(scope="module")
def ports(built):
    p = Ports()
    yield p
    p.close()


def round_trip(ctx, words, what, exp=None):
    """import the packed records, compare every array with the restatement, export them again: the same bytes"""
    n = 2 * len(words)
    dev = torch.from_numpy(np.ascontiguousarray(words).view(np.uint8).reshape(-1)).cuda() if n else torch.zeros(16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    got = ctx.edge_records_import(C.c_void_p(dev.data_ptr()), n)
    exp = reclib.expect(words) if exp is None else exp
    assert set(got) == set(exp), what
    for k in exp:
        assert got[k].dtype == exp[k].dtype and np.array_equal(got[k], exp[k]), f"{what}: {k} differs from the restatement"
    back = torch.full((max(n // 2 * reclib.WORDS * 4, 16),), 0xa5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.edge_records_export(C.c_void_p(back.data_ptr()), n)
    assert torch.equal(back[: dev.numel()] if n else back[:0], dev if n else dev[:0]), f"{what}: the exported bytes are not the imported ones"
    if n == 0:
        assert got["edge_off"].tolist() == [0] and len(got["edge_key"]) == 0 and bool((back == 0xa5).all()), what


def case(n_contigs, n, name, gen, kw):
    words, man = gen(n_contigs, n, **kw)
    assert reclib.check(words, man, n_contigs)
    return words, f"{name} n_contigs={n_contigs} n={n}"


def test_record_size():
    assert hip.records_bytes() * 2 == reclib.WORDS * 4


@pytest.mark.parametrize("group", reclib.GROUPS)
@pytest.mark.parametrize("n_contigs", reclib.N_CONTIGS)
def test_small_sizes(n_contigs, group, ports):
    """every pattern of the group at 0, 2 and around 256, 2 048 and 8 192 records: one and several sort tiles, a last round of 254, 0
    and 2 valid lanes, and at 8 194 the histogram scan on two levels"""
    ctx = ports.at(n_contigs)
    ran = 0
    for name, gen, kw in reclib.patterns(n_contigs):
        if name.split("[")[0] != group:
            continue
        for n in reclib.SMALL_N:
            round_trip(ctx, *case(n_contigs, n, name, gen, kw))
            ran += 1
    assert ran >= len(reclib.SMALL_N)


@pytest.mark.parametrize("n", reclib.LARGE_N)
@pytest.mark.parametrize("n_contigs", reclib.LARGE_N_CONTIGS)
def test_large_sizes(n_contigs, n, ports):
    """2^20 - 2, 2^20 (the exact fit of the scan's second level) and 2^20 + 1 030 records (its third level)"""
    ctx = ports.at(n_contigs)
    for name, gen, kw in reclib.patterns(n_contigs, large=True):
        round_trip(ctx, *case(n_contigs, n, name, gen, kw))


@pytest.mark.parametrize("n_contigs", reclib.LARGE_N_CONTIGS)
def test_sizes_in_turn_in_one_context(n_contigs, ports):
    """a large set, then small ones, then the large one again in the same context: nothing of one call is left in the workspace or
    the scratch buffers for the next (Workspace::reset allocates anew after growth)"""
    ctx = ports.at(n_contigs)
    large = case(n_contigs, (1 << 20) + 1030, "uniform", reclib.uniform, {})
    exp = reclib.expect(large[0])
    for n, gen in ((8194, reclib.boundaries), (0, reclib.uniform), (2050, reclib.descending)):
        round_trip(ctx, *case(n_contigs, n, gen.__name__, gen, {}))
        round_trip(ctx, *large, exp=exp)
        round_trip(ctx, *case(n_contigs, n, gen.__name__, gen, {}))


def test_emitted_records_export_as_pack_writes_them(sim, ports):
    """edge_emit and edge_records_export on a simulated data set: the bytes are reclib.pack of the oracle's forward records"""
    pre = sim(*SIM_ARGS)
    _, fwd = oracle_edges(pre)
    words = reclib.pack(fwd)
    ds = host.Dataset(pre + ".contigs.fa", pre + ".reads.fa", pre + ".paf")
    ctx = ports.small
    ports.small_n = None
    ctx.upload(ds)
    prm = ds.params()
    ctx.chain_reads(prm)
    n = ctx.edge_emit(prm)
    assert n == 2 * len(words) > 2000
    out = torch.zeros(n * hip.records_bytes(), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.edge_records_export(C.c_void_p(out.data_ptr()), n)
    assert np.array_equal(out.cpu().numpy().view(np.uint32).reshape(-1, reclib.WORDS), words)
    ds.close()


@pytest.mark.parametrize("n_reads", [1025, (1 << 20) + 1030])
def test_chain_scans_past_2_20_reads(n_reads, ports, tmp_path):
    """the scans over the reads in hx_chain_reads (alignments and compact alignments per read) and hx_edge_emit (pairs per read) at
    three levels: the hit_counts family among 2^20 + 1 030 reads, its reads on both sides of the first tile edges, of 2^20 and at
    the last index, against the oracle. 1 025 reads: two levels, and a last tile that holds one read"""
    pre, cs = fc.build(str(tmp_path / "in"), ["hit_counts"], n_reads=n_reads, reads_at=fc.many_reads_at(n_reads))
    ds = host.Dataset(pre + ".contigs.fa", pre + ".reads.fa", pre + ".paf")
    assert ds.reads.n == n_reads
    ob = orclib.OracleBackend(ds, 4)
    ro = host.Run(ds, ds.params(), ob.table, None)
    ro.chain(); ro.graph()
    chain, edges = ro.chain_out(), ro.edges_out()
    fc.check_many_reads(cs, n_reads, chain, edges)
    ctx = ports.small
    ports.small_n = None
    ctx.upload(ds)
    rg = host.Run(ds, ds.params(), ctx.backend(), None)
    rg.chain(); rg.graph()
    for what, a, b in (("chain", chain, rg.chain_out()), ("edges", edges, rg.edges_out())):
        assert set(a) == set(b)
        for k in a:
            assert np.array_equal(a[k], b[k]), f"{what}.{k} differs between the HIP path and the oracle"
    rg.close(); ro.close(); ob.close(); ds.close()
