"""GPU parity tests proper: the HIP path, called through the C-ABI (libhaslr_hip.so), against the CPU oracle on
the same seeded inputs — bit-exact for every stage — plus golden fixtures, edge cases, size-independent
properties, and the drop-in CLI."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import orclib
import util
from haslr_amd import ctypes_defs as T
from haslr_amd import hip, host

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def ctx(built):
    c = hip.HipContext(0)   # raises without a device: these tests never run on a fallback
    yield c
    c.close()


def both(ds, ctx, out_o, out_g, params=None, threads=8):
    prm = params or ds.params()
    ob = orclib.OracleBackend(ds, threads)
    ro = host.Run(ds, prm, ob.table, out_o)
    ro.all()
    ctx.upload(ds)
    rg = host.Run(ds, prm, ctx.backend(), out_g)
    rg.all()
    return ro, rg, ob


def assert_same_arrays(a, b, what):
    for k in a:
        assert np.array_equal(a[k], b[k]), f"{what}.{k} differs between the HIP path and the oracle"


CASES = [("--genome-len", "150000", "--seed", "21", "--variant-per-mb", "30"),
         ("--genome-len", "120000", "--seed", "22", "--variant-per-mb", "30", "--model", "nanopore"),
         ("--genome-len", "100000", "--seed", "23", "--model", "perfect", "--cov", "15"),
         ("--genome-len", "90000", "--seed", "24", "--variant-per-mb", "40", "--cov", "40", "--read-median", "4000")]


@pytest.mark.parametrize("args", CASES, ids=lambda a: "_".join(a[1:4:2]))
def test_every_stage_bit_exact(args, sim, ctx, tmp_path):
    pre = sim(*args)
    ds = host.Dataset(pre + ".contigs.fa", pre + ".reads.fa", pre + ".paf")
    ro, rg, ob = both(ds, ctx, str(tmp_path / "o"), str(tmp_path / "g"))
    assert_same_arrays(ro.chain_out(), rg.chain_out(), "chain")
    assert_same_arrays(ro.edges_out(), rg.edges_out(), "edges")
    assert_same_arrays(ro.coords_out(), rg.coords_out(), "coords")
    assert ro.cns_out() == rg.cns_out()
    assert ro.cns_stats() == rg.cns_stats()
    assert util.compare_dirs(str(tmp_path / "o"), str(tmp_path / "g")) == []
    assert os.path.getsize(tmp_path / "g" / "asm.final.fa") > 0


@pytest.mark.parametrize("lds_supp", ["0", "3"])
def test_coords_through_the_global_scratch(lds_supp, sim, ctx, tmp_path):
    """K5 keeps the sorted lists and event records of an edge in LDS up to 384 supports; option coords_lds_supp sends every edge (0) or every edge with
    more than three supports through the global scratch path that only an edge with hundreds of supports would take - same coordinates either way
    (hairpins included: their output slices are doubled)"""
    pre = sim("--genome-len", "150000", "--seed", "22", "--variant-per-mb", "20", "--hairpin-frac", "0.05")
    ds = host.Dataset(pre + ".contigs.fa", pre + ".reads.fa", pre + ".paf")
    with ctx.options(coords_lds_supp=lds_supp):
        ro, rg, ob = both(ds, ctx, None, None)
    assert_same_arrays(ro.coords_out(), rg.coords_out(), "coords")
    assert ro.cns_out() == rg.cns_out()


@pytest.mark.parametrize("block", [64, 128, 512, 1024])
def test_poa_block_sizes_agree(block, sim, ctx, tmp_path):
    pre = sim("--genome-len", "100000", "--seed", "25", "--variant-per-mb", "20")
    ds = host.Dataset(pre + ".contigs.fa", pre + ".reads.fa", pre + ".paf")
    ctx.set_poa_block(block)
    try:
        ro, rg, ob = both(ds, ctx, None, None)
        assert ro.cns_out() == rg.cns_out()
    finally:
        ctx.set_poa_block(0)


def test_nondefault_parameters(sim, ctx, tmp_path):
    pre = sim("--genome-len", "150000", "--seed", "21", "--variant-per-mb", "30")
    ds = host.Dataset(pre + ".contigs.fa", pre + ".reads.fa", pre + ".paf")
    prm = ds.params(min_aln_block=900, min_aln_sim=0.87, min_edge_sup=2, max_uniq_dev=0.1)
    ro, rg, ob = both(ds, ctx, str(tmp_path / "o"), str(tmp_path / "g"), prm)
    assert_same_arrays(ro.chain_out(), rg.chain_out(), "chain")
    assert_same_arrays(ro.edges_out(), rg.edges_out(), "edges")
    assert util.compare_dirs(str(tmp_path / "o"), str(tmp_path / "g")) == []


@pytest.mark.parametrize("case", sorted(d for d in os.listdir(GOLD) if os.path.isfile(os.path.join(GOLD, d, "manifest.json"))))
def test_golden_fixtures_through_hip(case, sim, ctx, tmp_path):
    """front-half outputs of the HIP path against the files the compiled reference produced; and its back half (edge coordinates,
    sub-sequences, stitching) against what the reference's whole program wrote with the oracle's consensus strings (tests/backlib.py)"""
    import gzip
    cd = os.path.join(GOLD, case)
    man = json.load(open(os.path.join(cd, "manifest.json")))
    pre = sim(*man["hxsim_args"])
    for k, h in man["inputs"].items():
        if util.sha256_file(pre + k) != h:
            pytest.skip("generator bytes differ from fixture")
    ds = host.Dataset(pre + ".contigs.fa", pre + ".reads.fa", pre + ".paf")
    ctx.upload(ds)
    out = str(tmp_path / "g")
    run = host.Run(ds, ds.params(), ctx.backend(), out)
    run.chain()
    run.graph()
    exp = os.path.join(cd, "expected")
    for f in sorted(os.listdir(exp)):
        if f.endswith(".skel"):
            assert util.sha256_file(os.path.join(out, f[:-5])) == man["outputs"][f[:-5]], f
        elif not f.endswith(".gz") and f != "uniq_freq.txt":
            assert open(os.path.join(out, f)).read() == open(os.path.join(exp, f)).read(), f
    assert util.sha256_bytes(util.alignments_paf(ds, run.chain_out()).encode()) == man["outputs"]["alignments.fixed.paf"]
    assert util.edge_supp_text(run.edges_out(sides=False)) == gzip.open(os.path.join(exp, "edge_supp.01.txt.gz"), "rt").read()
    import backlib
    run.coords()
    run.consensus()
    run.assemble()
    backlib.golden_back_check(man["back"], os.path.join(cd, "expected_back"), run, out)


def test_cli_with_threaded_cleaning_equals_the_reference_fixture(sim, built, tmp_path):
    """SURVEY 8f #3 under the driver's eyes: the haslr_assemble binary on the fixture where all four cleaning passes fire (tips, simple / super / small
    bubbles), with the host-parallel formulation of the passes forced on (HASLR_CLEAN_THREADS=16; by default it starts at 200 000 nodes), against
    the GFA / stat / log files the COMPILED REFERENCE wrote for these inputs"""
    cd = os.path.join(GOLD, "nanopore_rich_300k_s5")
    man = json.load(open(os.path.join(cd, "manifest.json")))
    pre = sim(*man["hxsim_args"])
    for k, h in man["inputs"].items():
        if util.sha256_file(pre + k) != h:
            pytest.skip("generator bytes differ from fixture")
    exe = os.path.join(ROOT, "haslr_amd", "bin", "haslr_assemble")
    out = tmp_path / "cli16"
    r = subprocess.run([exe, "-t", "16", "-c", pre + ".contigs.fa", "-l", pre + ".reads.fa", "-m", pre + ".paf", "-d", str(out)],
                       capture_output=True, text=True, env=dict(os.environ, HASLR_CLEAN_THREADS="16", HASLR_GRAPH_DEBUG="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert "cleaning passes on 16 threads" in r.stderr, r.stderr[-2000:]
    exp = os.path.join(cd, "expected")
    checked = 0
    for f in sorted(os.listdir(exp)):
        if f.endswith(".skel"):
            assert util.sha256_file(os.path.join(out, f[:-5])) == man["outputs"][f[:-5]], f
            checked += 1
        elif not f.endswith(".gz") and f != "uniq_freq.txt":
            assert open(os.path.join(out, f)).read() == open(os.path.join(exp, f)).read(), f
            checked += 1
    assert checked >= 18
    for log, what in (("backbone.03.tip.log", 1), ("backbone.04.simplebubble.log", 1), ("backbone.05.superbubble.log", 1), ("backbone.06.smallbubble.log", 1)):
        assert os.path.getsize(os.path.join(out, log)) > 0, log   # every pass did something on this graph


def test_against_compiled_reference_front_half(sim, ctx, ref_front, tmp_path):
    pre = sim("--genome-len", "110000", "--seed", "31", "--variant-per-mb", "40", "--cov", "14")
    rd = tmp_path / "ref"
    rd.mkdir()
    subprocess.check_call([ref_front, "-c", pre + ".contigs.fa", "-l", pre + ".reads.fa", "-m", pre + ".paf", "-d", str(rd)], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    ds = host.Dataset(pre + ".contigs.fa", pre + ".reads.fa", pre + ".paf")
    ctx.upload(ds)
    run = host.Run(ds, ds.params(), ctx.backend(), str(tmp_path / "g"))
    run.chain()
    run.graph()
    assert util.compare_dirs(str(rd), str(tmp_path / "g")) == []
    assert util.alignments_paf(ds, run.chain_out()) == open(rd / "alignments.fixed.paf").read()
    assert util.edge_supp_text(run.edges_out(sides=False)) == open(rd / "edge_supp.01.txt").read()


def test_cli_drop_in(sim, built, tmp_path):
    """the haslr_assemble binary with haslr.py's argv (bin/haslr.py:66) reproduces the oracle-backed run"""
    pre = sim("--genome-len", "100000", "--seed", "25", "--variant-per-mb", "20")
    exe = os.path.join(ROOT, "haslr_amd", "bin", "haslr_assemble")
    out = tmp_path / "cli"
    r = subprocess.run([exe, "-t", "4", "-c", pre + ".contigs.fa", "-l", pre + ".reads.fa", "-m", pre + ".paf", "-d", str(out),
                        "--aln-block", "500", "--aln-sim", "0.85", "--edge-sup", "3"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    ds = host.Dataset(pre + ".contigs.fa", pre + ".reads.fa", pre + ".paf")
    ob = orclib.OracleBackend(ds, 8)
    ro = host.Run(ds, ds.params(), ob.table, str(tmp_path / "o"))
    ro.all()
    names = [f for f in os.listdir(tmp_path / "o")]
    assert "asm.final.fa" in names and "backbone.06.smallbubble.gfa" in names
    assert util.compare_dirs(str(tmp_path / "o"), str(out), names) == []


def test_pipeline_driver_with_the_real_assembler(sim, built, tmp_path):
    """haslr.py (haslr_amd/driver/haslr_pipeline.py) end to end: stand-ins only for the external tools (fastutils hands the reads on,
    minimap2 hands over the simulator's PAF), the real minia_nooverlap and the real MI355X haslr_assemble; the assembly it leaves in
    asm_*/asm.final.fa is the oracle-backed one, and a second run finds everything done"""
    import driverlib
    pre = sim("--genome-len", "120000", "--seed", "27")
    bindir, out = str(tmp_path / "bin"), str(tmp_path / "out")
    real = {t: os.path.join(ROOT, "haslr_amd", "bin", t) for t in ("haslr_assemble", "minia_nooverlap")}
    driverlib.make_bin(bindir, os.path.join(ROOT, "haslr_amd", "bin", "haslr.py"), real=real)
    data = os.path.dirname(pre)
    args = ["-o", out, "-g", "120k", "-l", pre + ".reads.fa", "-x", "pacbio", "-c", pre + ".contigs.fa", "-t", "4", "--cov-lr", "0"]
    r = driverlib.run(bindir, data, out, args, extra_env={"STUB_PAF": pre + ".paf"})
    assert r["rc"] == 0, r["stdout"] + r["tree"].get("asm_contigs_k49_a3_c250_lrall_b500_s3_sim0.85.err", "")
    assert [c["tool"] for c in r["calls"]] == ["fastutils", "fastutils", "minimap2"]       # the two real tools do not record
    ds = host.Dataset(pre + ".contigs.fa", pre + ".reads.fa", pre + ".paf")
    ob = orclib.OracleBackend(ds, 8)
    ro = host.Run(ds, ds.params(), ob.table, None)
    ro.all()
    asm = r["tree"]["asm_contigs_k49_a3_c250_lrall_b500_s3_sim0.85/asm.final.fa"]
    assert asm == ro.assembly_fasta() and asm.count(">") >= 1
    r2 = driverlib.run(bindir, data, out, args, extra_env={"STUB_PAF": pre + ".paf"})
    assert r2["rc"] == 0 and r2["calls"] == [] and r2["stdout"].count("already exists") == 5
    ro.close(); ob.close(); ds.close()


def test_edge_cases(ctx, built, tmp_path):
    """empty PAF, reads without hits, a read with a single hit (dropped, Longread.cpp:184), ragged sizes"""
    c = tmp_path / "c.fa"
    seqs = ["ACGT" * 300, "TTGCA" * 250, "GATTACA" * 200]
    c.write_text("".join(f">{i} LN:i:{len(s)} KC:i:{30 * len(s)} km:f:30.0\n{s}\n" for i, s in enumerate(seqs)))
    r = tmp_path / "r.fa"
    r.write_text(">0\n" + "ACGT" * 900 + "\n>1\nACGTA\n>2\n" + "G" * 3000 + "\n")
    p = tmp_path / "m.paf"
    p.write_text("")
    for paf_text in ("", "0\t3600\t0\t1200\t+\t0\t1200\t0\t1200\t1200\t1200\t60\tcg:Z:1200M\n"):
        p.write_text(paf_text)
        ds = host.Dataset(str(c), str(r), str(p))
        ro, rg, ob = both(ds, ctx, str(tmp_path / "o"), str(tmp_path / "g"))
        assert_same_arrays(ro.chain_out(), rg.chain_out(), "chain")
        assert rg.chain_out()["cmp_aln"].size == 0 and rg.n_edges == 0
        assert util.compare_dirs(str(tmp_path / "o"), str(tmp_path / "g")) == []
        assert open(tmp_path / "g" / "compact_uniq.txt").read() == ">0\t\n>1\t\n>2\t\n"


def test_error_free_reads_reassemble_genome_on_gpu(sim, ctx, tmp_path):
    """size-independent property: with perfect reads every consensus is exact, so each assembled contig is a
    substring of the truth genome (either strand)"""
    pre = sim("--genome-len", "400000", "--seed", "41", "--model", "perfect", "--no-variants", "--cov", "15")
    ds = host.Dataset(pre + ".contigs.fa", pre + ".reads.fa", pre + ".paf")
    ctx.upload(ds)
    run = host.Run(ds, ds.params(), ctx.backend(), None)
    run.all()
    genome = open(pre + ".genome.fa").read().split("\n")[1]
    comp = str.maketrans("ACGT", "TGCA")
    recs = [l for l in run.assembly_fasta().split("\n") if l and not l.startswith(">")]
    assert recs and sum(map(len, recs)) > 0.6 * len(genome)
    for s in recs:
        assert s in genome or s.translate(comp)[::-1] in genome


def test_full_size_properties(sim, ctx, tmp_path):
    """BASELINE configs[1] size (4.6 Mb, 25x): too big for the oracle in a test, so check invariants:
    twin symmetry of the edge multiset, sortedness, idempotence of a second run, identity vs truth."""
    # no planted variant molecules here: their novel segments are not part of genome.fa, so identity vs truth would measure the planted
    # haplotype differences rather than consensus quality (the bench data set keeps them; its parity is covered by the smaller cases)
    pre = sim("--genome-len", "4600000", "--seed", hex(0x4841534C + 1), "--no-variants")
    ds = host.Dataset(pre + ".contigs.fa", pre + ".reads.fa", pre + ".paf")
    ctx.upload(ds)
    prm = ds.params()
    out = str(tmp_path / "g")
    run = host.Run(ds, prm, ctx.backend(), out)
    run.all()
    e = run.edges_out(sides=False)
    assert np.all(e["key"][1:] >= e["key"][:-1])
    twin = ((e["edge_key"] & 0xffffffff) ^ 1) << np.uint64(32) | ((e["edge_key"] >> np.uint64(32)) ^ np.uint64(1))
    cnt = dict(zip(e["edge_key"].tolist(), np.diff(e["edge_off"]).tolist()))
    for k, t in zip(e["edge_key"].tolist(), twin.tolist()):
        assert cnt[t] == cnt[k]          # every edge has a twin with the same support
    c = run.chain_out()
    for a, b in zip(c["cmp_off"][:-1], c["cmp_off"][1:]):
        q = c["cmp_aln"][int(a):int(b)]
        assert np.all(c["q_end"][q][:-1] <= c["q_start"][q][1:])   # chained hits never overlap on the read
    fasta1 = run.assembly_fasta()
    run2 = host.Run(ds, prm, ctx.backend(), None)
    run2.all()
    assert run2.assembly_fasta() == fasta1                           # idempotent / deterministic
    o = subprocess.check_output([os.path.join(ROOT, "tools", "hxident"), pre + ".genome.fa", os.path.join(out, "asm.final.fa")], text=True)
    ident = float(o.strip().split("\n")[-1].split()[1])
    assert ident >= 0.998, o[-500:]


def test_record_exchange_roundtrip(sim, ctx):
    """multi-GPU plumbing on one GPU: emit two read shards separately, pack, concatenate in rank order, import:
    identical to the unsharded edge multiset"""
    import torch
    pre = sim("--genome-len", "150000", "--seed", "21", "--variant-per-mb", "30")
    ds = host.Dataset(pre + ".contigs.fa", pre + ".reads.fa", pre + ".paf")
    prm = ds.params()
    ctx.upload(ds)
    ctx.chain_reads(prm)
    whole = ctx.edge_support(prm)
    from haslr_amd import distributed as hd
    b = hd.shard_bounds(ds.read_hit_off, ds.reads.n, 3)
    rb = hip.records_bytes()
    parts = []
    for r in range(3):
        ctx.set_read_shard(b[r], b[r + 1])
        ctx.chain_reads(prm)
        n = ctx.edge_emit(prm)
        t = torch.empty(max(n, 1) * rb, dtype=torch.uint8, device="cuda")
        ctx.edge_records_export(C.c_void_p(t.data_ptr()), n)
        parts.append(t[: n * rb])
    merged = torch.cat(parts).contiguous()
    torch.cuda.synchronize()
    got = ctx.edge_records_import(C.c_void_p(merged.data_ptr()), merged.numel() // rb)
    ctx.set_read_shard(0, ds.reads.n)
    for k in whole:
        assert np.array_equal(whole[k], got[k]), k


@pytest.mark.parametrize("seed", [51, 52, 53, 54, 55, 56])
def test_consensus_bit_exact_many_seeds(seed, sim, ctx):
    """more POA instances (different graph shapes, end-node ties, hairpins of the generator's variants) at small size"""
    pre = sim("--genome-len", "70000", "--seed", str(seed), "--variant-per-mb", "40", "--cov", "30")
    ds = host.Dataset(pre + ".contigs.fa", pre + ".reads.fa", pre + ".paf")
    ro, rg, ob = both(ds, ctx, None, None)
    assert_same_arrays(ro.coords_out(), rg.coords_out(), "coords")
    assert ro.cns_out() == rg.cns_out()
    assert ro.assembly_fasta() == rg.assembly_fasta()


def test_score_matrix_traceback_matches_direction_bytes(sim, ctx):
    """the two traceback sources of the POA kernel (1-byte direction codes vs the int32 score matrix) give the same consensus"""
    pre = sim("--genome-len", "100000", "--seed", "25", "--variant-per-mb", "20")
    ds = host.Dataset(pre + ".contigs.fa", pre + ".reads.fa", pre + ".paf")
    ctx.upload(ds)
    prm = ds.params()
    a = host.Run(ds, prm, ctx.backend(), None)
    a.all()
    ctx.set_poa_traceback(0)
    try:
        b = host.Run(ds, prm, ctx.backend(), None)
        b.all()
    finally:
        ctx.set_poa_traceback(1)
    assert a.cns_out() == b.cns_out() and a.assembly_fasta() == b.assembly_fasta()


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [("300", "64", "8", "8", "0"), ("300", "64", "4", "3", "100"), ("500", "128", "4", "4", "2"), ("400", "256", "8", "8", "100"),
                                 ("300", "64", "4", "3", "0"), ("400", "256", "8", "8", "0"),
                                 # two columns per lane (round 6: the members of the few-edge regime's shared edges): 256-lane members, wide members, members without a column
                                 ("300", "256", "2", "8", "0"), ("200", "256", "2", "3", "100"), ("400", "256", "2", "16", "2"),
                                 # exact pruning inside shared edges (off by default; the members run DP attempts, a missed threshold is repeated by all of them): an honest
                                 # threshold, an optimistic one (most alignments repeated), wide members, 2 / 4 / 8 columns per lane
                                 ("300", "64", "8", "8", "0", "95"), ("300", "128", "4", "4", "2", "108"), ("300", "256", "2", "8", "100", "95"), ("400", "256", "8", "8", "0", "104")])
def test_shared_edges_cluster_mode(sim, ctx, cfg):
    """cluster mode: the DP columns of an edge spread over several workgroups (forced here on short gaps with small members, so that
    every variant — single-wave members, multi-wave members, members without columns for a short read, sink rows in another member —
    is exercised) gives the consensus of the oracle, bit for bit. Last knob: how many of the costliest shared edges run with WIDE members
    (1024-lane workgroups whose first waves do the DP and all of whose waves work in member 0's graph phases): none, some, all"""
    import os
    pre = sim("--genome-len", "150000", "--seed", "31", "--variant-per-mb", "15")
    ds = host.Dataset(pre + ".contigs.fa", pre + ".reads.fa", pre + ".paf")
    prm = ds.params()
    be = orclib.OracleBackend(ds, 8)
    ro = host.Run(ds, prm, be.table, None)
    ro.all()
    ctx.upload(ds)
    keys = ("poa_cluster_min", "poa_member_lanes", "poa_cluster_cols", "poa_cluster_max", "poa_wide_members", "poa_prune_shared")
    with ctx.options(**dict(zip(keys, cfg))):
        rg = host.Run(ds, prm, ctx.backend(), None)
        rg.all()
    assert ro.cns_out() == rg.cns_out()
    assert ro.assembly_fasta() == rg.assembly_fasta()
    assert ro.cns_stats()["dp_cells"] == rg.cns_stats()["dp_cells"]
    rg.close(); ro.close(); be.close(); ds.close()


@pytest.mark.gpu
def test_in_degree_retry_with_score_matrix(sim, ctx):
    """direction bytes carry a 4-bit predecessor slot; an edge whose graph grows a node with more in-edges comes back from the kernel
    and is redone with the score-matrix traceback. Forced here by lowering the limit to 2: results (and the reported cell count) stay
    those of the oracle"""
    pre = sim("--genome-len", "120000", "--seed", "33", "--variant-per-mb", "15")
    ds = host.Dataset(pre + ".contigs.fa", pre + ".reads.fa", pre + ".paf")
    prm = ds.params()
    be = orclib.OracleBackend(ds, 8)
    ro = host.Run(ds, prm, be.table, None)
    ro.all()
    ctx.upload(ds)
    with ctx.options(poa_max_indeg=2):
        rg = host.Run(ds, prm, ctx.backend(), None)
        rg.all()
    assert ro.cns_out() == rg.cns_out()
    assert ro.cns_stats()["dp_cells"] == rg.cns_stats()["dp_cells"]
    rg.close(); ro.close(); be.close(); ds.close()


_FAR_ROW_ORACLE = {}


@pytest.mark.gpu
@pytest.mark.parametrize("far_rows,shape", [("0", {}), ("1", {}), ("0", {"HX_POA_CLUSTER_MIN": "300", "HX_POA_MEMBER_LANES": "128", "HX_POA_CLUSTER_MAX": "3"}),
                                            ("2", {"HX_POA_WAVE_MAX": "4096"}), ("1", {"HX_POA_BATCHES": "3"}),
                                            ("-1", {"HX_POA_NODE_EST_PCT": "3"}), ("1", {"HX_POA_NODE_EST_PCT": "20", "HX_POA_BATCHES": "2"}),
                                            # persistent workgroups (what thousands of edges get): 1-3 workspace slots per launch class, every workgroup works through many edges
                                            ("-1", {"HX_POA_SLOTS": "1"}), ("1", {"HX_POA_SLOTS": "2"}), ("0", {"HX_POA_SLOTS": "3", "HX_POA_NODE_EST_PCT": "20"}),
                                            ("-1", {"HX_POA_SLOTS": "2", "HX_POA_CLUSTER_MIN": "100000", "HX_POA_COLS": "8"}),
                                            # the pruned row loop (what calls of thousands of edges get; forced here): plain, far rows forced, persistent workgroups with 8 / 4 columns per
                                            # lane, two-wave workgroups, an optimistic threshold (every other alignment is repeated), no ring (every kept row through HBM)
                                            ("-1", {"HX_POA_PRUNE": "95", "HX_POA_WAVE_MAX": "128"}), ("1", {"HX_POA_PRUNE": "95", "HX_POA_WAVE_MAX": "64", "HX_POA_COLS": "8"}),
                                            ("0", {"HX_POA_PRUNE": "90", "HX_POA_WAVE_MAX": "128", "HX_POA_SLOTS": "2", "HX_POA_CLUSTER_MIN": "100000", "HX_POA_COLS": "8"}),
                                            ("2", {"HX_POA_PRUNE": "104", "HX_POA_WAVE_MAX": "128", "HX_POA_SLOTS": "3", "HX_POA_CLUSTER_MIN": "100000"}),
                                            ("-1", {"HX_POA_PRUNE": "110", "HX_POA_WAVE_MAX": "64", "HX_POA_CLUSTER_MIN": "100000", "HX_POA_RING_KB": "1"}),
                                            ("-1", {"HX_POA_PRUNE": "95", "HX_POA_WAVE_MAX": "128", "HX_POA_CLUSTER_MIN": "100000", "HX_POA_RING_ZERO": "1"}),
                                            # column passes (the unshared multi-wave edges of a pruned call): windows of 64 / 128 lanes x 4 or 8 columns taken one after the other by one
                                            # workgroup, the carries between windows through HBM; with far rows forced, persistent slots, no pruning to speak of (threshold 1 %), repeats
                                            ("-1", {"HX_POA_PRUNE": "95", "HX_POA_WAVE_MAX": "64", "HX_POA_PASS_LANES": "64", "HX_POA_CLUSTER_MIN": "100000"}),
                                            ("1", {"HX_POA_PRUNE": "95", "HX_POA_WAVE_MAX": "64", "HX_POA_PASS_LANES": "128", "HX_POA_CLUSTER_MIN": "100000", "HX_POA_COLS": "8", "HX_POA_SLOTS": "2"}),
                                            ("0", {"HX_POA_PRUNE": "1", "HX_POA_WAVE_MAX": "64", "HX_POA_PASS_LANES": "64", "HX_POA_CLUSTER_MIN": "100000", "HX_POA_PRUNE_LAZY": "0"}),
                                            ("2", {"HX_POA_PRUNE": "108", "HX_POA_WAVE_MAX": "128", "HX_POA_PASS_LANES": "128", "HX_POA_SLOTS": "3", "HX_POA_RING_KB": "1"}),
                                            # ... with the workgroup width chosen by the edge's estimated chain time (the default of a pruned call; caps that a small data set
                                            # reaches, so that every width from 64 lanes up gets edges), the need buckets of an instance in one launch, few slots per bucket
                                            ("-1", {"HX_POA_PRUNE": "95", "HX_POA_WAVE_MAX": "64", "HX_POA_CHAIN_MS": "1", "HX_POA_CLUSTER_MIN": "100000"}),
                                            ("1", {"HX_POA_PRUNE": "95", "HX_POA_WAVE_MAX": "64", "HX_POA_CHAIN_MS": "4", "HX_POA_CLUSTER_MIN": "100000", "HX_POA_SLOTS": "2"}),
                                            ("-1", {"HX_POA_PRUNE": "100", "HX_POA_WAVE_MAX": "128", "HX_POA_CHAIN_MS": "20", "HX_POA_SLOTS": "3", "HX_POA_RING_KB": "1"})])
def test_far_row_estimate_overflow_is_retried(sim, ctx, far_rows, shape):
    """with direction bytes H keeps only the rows that a successor reads after they left the LDS ring, in as many rows as the host
    estimated; an edge that needs more comes back and is redone with room for every row. Forced here by an estimate of 0..2 rows
    (long gaps with deep coverage produce far rows): results and cell counts stay those of the oracle. Likewise the node estimate: a graph
    that outgrows it (forced by scaling the estimate to 3 % / 20 %) is redone with twice the room until it fits"""
    pre = sim("--genome-len", "150000", "--seed", "34", "--cov", "40", "--gap-median", "2500")
    ds = host.Dataset(pre + ".contigs.fa", pre + ".reads.fa", pre + ".paf")
    prm = ds.params()
    if "oracle" not in _FAR_ROW_ORACLE:   # (one oracle pass for the two dozen launch shapes: it was most of every case's time)
        be = orclib.OracleBackend(ds, 8)
        ro = host.Run(ds, prm, be.table, None)
        ro.all()
        _FAR_ROW_ORACLE["oracle"] = (ro.cns_out(), ro.cns_stats()["dp_cells"])
        ro.close(); be.close()
    want_cns, want_cells = _FAR_ROW_ORACLE["oracle"]
    ctx.upload(ds)
    with ctx.options(**dict(shape, HX_POA_FAR_ROWS=far_rows)):   # (the old environment spellings name the same options: hx_set_option)
        rg = host.Run(ds, prm, ctx.backend(), None)
        rg.all()
    assert want_cns == rg.cns_out()
    assert want_cells == rg.cns_stats()["dp_cells"]
    assert rg.n_edges > 0
    rg.close(); ds.close()


@pytest.mark.gpu
def test_persistent_workgroups_on_many_edges(sim, ctx):
    """hundreds of edges through 4 persistent workgroups per launch class (the mode of the 140 Mb / 400 Mb runs, forced at test size): slots sized for
    their first edge and the largest of the rest, edges pulled through the class's counter - every consensus the oracle's"""
    pre = sim("--genome-len", "1200000", "--seed", "58", "--variant-per-mb", "10", "--cov", "22")
    ds = host.Dataset(pre + ".contigs.fa", pre + ".reads.fa", pre + ".paf")
    prm = ds.params()
    be = orclib.OracleBackend(ds, os.cpu_count() or 8)
    ro = host.Run(ds, prm, be.table, None)
    ro.all()
    ctx.upload(ds)
    with ctx.options(poa_slots=4):
        rg = host.Run(ds, prm, ctx.backend(), None)
        rg.all()
        ws_few = ctx.poa_workspace_bytes()
    assert rg.n_edges > 60
    assert ro.cns_out() == rg.cns_out() and ro.assembly_fasta() == rg.assembly_fasta()
    assert ro.cns_stats()["dp_cells"] == rg.cns_stats()["dp_cells"]
    assert ws_few > 0
    rg.close(); ro.close(); be.close(); ds.close()


@pytest.mark.gpu
def test_need_buckets_with_edges_redone_in_one_component(sim, ctx):
    """the launch of a call with column passes: the need buckets of one kernel instance share it, and a workgroup serves its bucket and every smaller one out
    of its own slot. An edge that is redone with a multiple of the H rows (far rows outgrew the estimate) or of the wide-row pool is small in total bytes and
    large in ONE component - the slot of a larger bucket must still hold it (round 5's fuzz case: one persistent slot per class, a node estimate starved to 2 %,
    pruning and passes on, forced block size 128 - a GPU memory access fault until every bucket's slot took the component-wise maximum over the smaller ones)"""
    pre = sim("--genome-len", "1000000", "--seed", "331118", "--model", "pacbio", "--cov", "70", "--variant-per-mb", "0", "--gap-median", "6000", "--hairpin-frac", "0.1")
    ds = host.Dataset(pre + ".contigs.fa", pre + ".reads.fa", pre + ".paf")
    prm = ds.params(min_aln_block=500, min_aln_sim=0.85, min_edge_sup=3, max_uniq_dev=0.15)
    be = orclib.OracleBackend(ds, os.cpu_count() or 8)
    ro = host.Run(ds, prm, be.table, None)
    ro.all()
    ctx.upload(ds)
    ctx.set_poa_block(128)
    try:
        with ctx.options(poa_slots=1, poa_prune=95, poa_prune_lanes=128, poa_node_est_pct=2):
            rg = host.Run(ds, prm, ctx.backend(), None)
            rg.all()
    finally:
        ctx.set_poa_block(0)
    assert rg.n_edges > 30
    assert ro.cns_out() == rg.cns_out() and ro.assembly_fasta() == rg.assembly_fasta()
    rg.close(); ro.close(); be.close(); ds.close()


@pytest.mark.gpu
def test_cli_reuses_index_caches(sim, built, tmp_path):
    """like the reference (main.cpp:39-103) the binary leaves index.contig / index.longread in -d and a second run loads them instead of
    the text files (which may be gone): same outputs"""
    pre = sim("--genome-len", "100000", "--seed", "27", "--variant-per-mb", "20")
    exe = os.path.join(ROOT, "haslr_amd", "bin", "haslr_assemble")
    out = tmp_path / "cli"
    args = ["-t", "4", "-d", str(out), "--aln-block", "500", "--aln-sim", "0.85", "--edge-sup", "3"]
    r = subprocess.run([exe, "-c", pre + ".contigs.fa", "-l", pre + ".reads.fa", "-m", pre + ".paf"] + args, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert os.path.getsize(out / "index.contig") > 16 and os.path.getsize(out / "index.longread") > 32
    keep = {f: open(out / f, "rb").read() for f in os.listdir(out) if not f.startswith("index.") and not f.startswith("log_")}
    for f in keep:
        os.remove(out / f)
    r = subprocess.run([exe, "-c", "/nonexistent/c.fa", "-l", "/nonexistent/r.fa", "-m", "/nonexistent/m.paf"] + args, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "reading contig index" in r.stderr and "reading long read and alignment index" in r.stderr
    for f, data in keep.items():
        assert open(out / f, "rb").read() == data, f


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(8))
def test_random_data_sets_and_launch_shapes(sim, ctx, case):
    """a seeded slice of tools/dev_fuzz.py (which has run hundreds of such cases): random generator settings, pipeline parameters and
    POA launch shapes; consensus strings and the assembly equal the oracle's"""
    import random
    rng = random.Random(1000 + case)
    pre = sim("--genome-len", str(rng.choice([60000, 90000, 150000])), "--seed", str(rng.randrange(1, 10**6)), "--model", rng.choice(["pacbio", "nanopore"]),
              "--cov", str(rng.choice([8, 15, 25, 40])), "--variant-per-mb", str(rng.choice([0, 5, 30])), "--gap-median", str(rng.choice([300, 600, 1500, 3000])))
    knobs = ("HX_POA_CLUSTER_MIN", "HX_POA_MEMBER_LANES", "HX_POA_CLUSTER_COLS", "HX_POA_CLUSTER_MAX", "HX_POA_MAX_INDEG", "HX_POA_WAVE_MAX")
    shape = ["default", "small-members", "one-wave", "block"][case % 4]
    env, block = {}, 0
    if shape == "small-members":
        env = {"HX_POA_CLUSTER_MIN": str(rng.choice([200, 400, 800])), "HX_POA_MEMBER_LANES": str(rng.choice([64, 128, 256])),
               "HX_POA_CLUSTER_COLS": str(rng.choice([4, 8])), "HX_POA_CLUSTER_MAX": str(rng.choice([2, 3, 8]))}
    elif shape == "one-wave":
        env = {"HX_POA_WAVE_MAX": str(rng.choice([128, 256, 2048])), "HX_POA_MAX_INDEG": str(rng.choice([2, 3, 16]))}
    elif shape == "block":
        block = rng.choice([64, 128, 256, 512, 1024])
    pk = dict(min_aln_block=rng.choice([250, 500, 1000]), min_aln_sim=rng.choice([0.8, 0.85, 0.9]), min_edge_sup=rng.choice([2, 3, 5]))
    ds = host.Dataset(pre + ".contigs.fa", pre + ".reads.fa", pre + ".paf")
    be = orclib.OracleBackend(ds, 8)
    ro = host.Run(ds, ds.params(**pk), be.table, None)
    ro.all()
    ctx.upload(ds)
    try:
        ctx.set_poa_block(block)
        with ctx.options(**env):
            rg = host.Run(ds, ds.params(**pk), ctx.backend(), None)
            rg.all()
    finally:
        ctx.set_poa_block(0)
    assert ro.cns_out() == rg.cns_out(), (shape, env, block, pk)
    assert ro.assembly_fasta() == rg.assembly_fasta()
    rg.close(); ro.close(); be.close(); ds.close()


# ---------------------------------------------------------------------------------------------- round 2
def test_edge_shards_merge_on_one_gpu(sim, ctx, tmp_path):
    """multi-GPU phase 2 on one GPU: three runs take a third of the work queue each (dealt by estimated cost), exchange their results
    blobs, and every one of them stitches the assembly of the unsharded run; before the exchange stitching is refused"""
    pre = sim("--genome-len", "400000", "--seed", "61", "--variant-per-mb", "30", "--cov", "12")
    ds = host.Dataset(pre + ".contigs.fa", pre + ".reads.fa", pre + ".paf")
    prm = ds.params()
    ctx.upload(ds)
    whole = host.Run(ds, prm, ctx.backend(), str(tmp_path / "whole"))
    whole.all()
    parts, blobs = [], []
    for r in range(3):
        run = host.Run(ds, prm, ctx.backend(), str(tmp_path / f"part{r}"))
        run.set_edge_shard(r, 3)
        run.chain(); run.graph(); run.coords(); run.consensus()
        assert 0 < run.n_edges < whole.n_edges and run.n_edges_total == whole.n_edges
        with pytest.raises(host.HostError):
            run.assemble()
        blobs.append(run.results_export())
        parts.append(run)
    assert sum(p.n_edges for p in parts) == whole.n_edges
    for r, run in enumerate(parts):
        run.results_import(b"".join(blobs))          # concatenation of every rank's blob, own included
        assert run.results_missing == 0
        run.assemble()
        assert run.assembly_fasta() == whole.assembly_fasta()
        assert util.compare_dirs(str(tmp_path / "whole"), str(tmp_path / f"part{r}")) == []


def _full_size_against_oracle(sim, ctx, args, min_edges):
    pre = sim(*args)
    ds = host.Dataset(pre + ".contigs.fa", pre + ".reads.fa", pre + ".paf")
    prm = ds.params()
    # the oracle leg runs BESIDE the GPU leg, on min(64, cores) threads: its row kernels are memory-bound (full int32 matrices per thread), and 256 threads
    # take twice as long as 64 on the GPU box's host (bench.py cpu_baseline: 95 s against 47 s at 140 Mb)
    import threading
    ob = orclib.OracleBackend(ds, min(64, os.cpu_count() or 8))
    ro = host.Run(ds, prm, ob.table, None)
    oracle_error = []

    def oracle_leg():
        try:
            ro.all()
        except Exception as e:  # noqa: BLE001
            oracle_error.append(e)
    th = threading.Thread(target=oracle_leg)
    th.start()
    ctx.upload(ds)
    rg = host.Run(ds, prm, ctx.backend(), None)
    rg.all()
    th.join()
    assert not oracle_error, oracle_error
    assert rg.n_edges >= min_edges
    assert_same_arrays(ro.chain_out(), rg.chain_out(), "chain")
    assert_same_arrays(ro.edges_out(), rg.edges_out(), "edges")
    assert_same_arrays(ro.coords_out(), rg.coords_out(), "coords")
    assert ro.cns_out() == rg.cns_out()
    assert ro.assembly_fasta() == rg.assembly_fasta()
    rg.close(); ro.close(); ob.close(); ds.close()


def test_configs2_full_size_against_oracle(sim, ctx):
    """BASELINE configs[2] at full size (12 Mb genome, Nanopore-like 25x: bench.py's default data set): every stage and every consensus
    identical to the oracle's"""
    _full_size_against_oracle(sim, ctx, ("--genome-len", "12000000", "--seed", hex(0x4841534C + 2), "--model", "nanopore", "--cov", "25", "--variant-per-mb", "1.5"), 800)


def test_configs1_bench_dataset_against_oracle(sim, ctx):
    """BASELINE configs[1] at full size WITH the planted variants (bench.py's E. coli-size data set): identical to the oracle's"""
    _full_size_against_oracle(sim, ctx, ("--genome-len", "4600000", "--seed", hex(0x4841534C + 1), "--model", "pacbio", "--cov", "25", "--variant-per-mb", "1.5"), 300)


def _drop_sim_files(pre):
    """the multi-GB inputs of the full-size tests do not stay on the box's disk for the rest of the session"""
    for suffix in (".contigs.fa", ".reads.fa", ".paf", ".genome.fa", ".truth.tsv"):
        try:
            os.remove(pre + suffix)
        except OSError:
            pass


CONFIGS3_ARGS = util.CONFIGS3_ARGS

huge = pytest.mark.skipif(bool(os.environ.get("HASLR_SKIP_HUGE")), reason="HASLR_SKIP_HUGE is set (developer runs: the 140 Mb / 400 Mb tests take ~10 min together)")


@huge
def test_configs3_full_size_against_oracle(sim, ctx):
    """BASELINE configs[3] at full size on ONE GPU (140 Mb genome, PacBio-like 25x, seed 0x4841534c + 3: bench.py --workload fly, the N = 4
    default): every stage array, every consensus and the assembly identical to the oracle's (all host cores; ~60 s simulate + ~2.5 min oracle)"""
    _full_size_against_oracle(sim, ctx, CONFIGS3_ARGS, 10000)   # (the files stay for tests/test_group_sharded.py's --gpus 8 run over the same data set, which removes them)


@huge
def test_configs4_share_full_size_properties(sim, ctx, tmp_path):
    """One GPU's share of BASELINE configs[4] (3.1 Gb / 8 GPUs = a 400 Mb genome, PacBio-like 25x, seed 0x4841534c + 4) on one MI355X. Too
    big for the oracle inside a test (405 s on 256 threads), so the size-independent properties: twin symmetry of the edge multiset,
    sortedness, non-overlapping chains, idempotence of a second pass, identity of the assembly against the truth genome."""
    # (round 6: the genome as four chromosomes of 100 Mb simulated side by side - the simulator took 2 of the test's 5 minutes on one thread)
    args = ("--genome-len", "400000000", "--seed", hex(0x4841534C + 4), "--model", "pacbio", "--cov", "25", "--no-variants", "--chromosomes", "4")
    pre = sim(*args)
    try:
        ds = host.Dataset(pre + ".contigs.fa", pre + ".reads.fa", pre + ".paf", threads=min(32, os.cpu_count() or 1))
        ctx.upload(ds)
        prm = ds.params()
        out = str(tmp_path / "g")
        run = host.Run(ds, prm, ctx.backend(), out)
        run.all()
        assert run.n_edges >= 30000
        e = run.edges_out(sides=False)
        assert np.all(e["key"][1:] >= e["key"][:-1])
        ek = e["edge_key"]
        twin = ((ek & np.uint64(0xffffffff)) ^ np.uint64(1)) << np.uint64(32) | ((ek >> np.uint64(32)) ^ np.uint64(1))
        cnt = np.diff(e["edge_off"])
        pos = np.searchsorted(ek, twin)                      # edge keys are sorted and unique
        assert np.all(pos < ek.size) and np.array_equal(ek[pos], twin) and np.array_equal(cnt[pos], cnt)   # every edge has a twin with the same support
        c = run.chain_out()
        a = c["cmp_aln"]
        inner = np.ones(a.size, dtype=bool)
        starts = c["cmp_off"][:-1]
        inner[starts[starts < a.size].astype(np.int64)] = False                                # first element of every compact read
        assert np.all(c["q_end"][a[:-1]][inner[1:]] <= c["q_start"][a[1:]][inner[1:]])        # chained hits never overlap on the read
        fasta1, cns1 = run.assembly_fasta(), run.cns_out()
        ws_free = ctx.poa_memory_stats()["last_call_workspace"]   # what this call took with the device (nearly) to itself
        run.close()
        # A rank of configs[4] holds the WHOLE replicated input beside its POA workspace: at CHM1 scale 82 GB of packed reads + CIGAR words (DESIGN.md 3,
        # 7.75 x this data set). Second pass at that shape for real: the workspace is released, a device BALLAST brings what is resident beside it to
        # 82 GB, the budget is taken again from what hipMemGetInfo reports free (no option caps it) - same consensus, same assembly. Third pass under
        # real shortage: more ballast until less is free than the workspace wanted, so the slot counts of the launch classes are scaled down until the
        # pools fit (hx_poa_plan.hip plan_batches / slots_wanted): the path a rank of a 288 GB device takes when its input share grows.
        resident = {"packed_read_bytes": int(ds.reads.off[ds.reads.n]), "cigar_word_bytes": 4 * int(ds.hits.cg_off[ds.hits.n]), "paf_records": int(ds.hits.n),
                    "read_bases": int(ds.total_read_bases), "poa_workspace_bytes_unconstrained": int(ws_free)}
        ballast = util.DeviceBallast(0)
        try:
            ctx.poa_release_workspace()
            free0 = ballast.free_bytes()
            ballast.hold(max(0, int(82e9) - resident["packed_read_bytes"] - resident["cigar_word_bytes"]))
            run2 = host.Run(ds, prm, ctx.backend(), None)
            run2.all()
            m2 = ctx.poa_memory_stats()
            print("configs4 share beside 82 GB of resident input: free before the ballast %.1f GB, ballast %.1f GB, free at the consensus call %.1f GB, budget %.1f GB, workspace settled on %.1f GB" %
                  (free0 / 1e9, ballast.bytes / 1e9, m2["free_at_first_call"] / 1e9, m2["budget"] / 1e9, m2["last_call_workspace"] / 1e9))
            assert run2.cns_out() == cns1 and run2.assembly_fasta() == fasta1
            assert m2["last_call_workspace"] <= m2["budget"] <= 0.9 * m2["free_at_first_call"] + 1
            run2.close()
            ctx.poa_release_workspace()
            want_free = int(0.55 * ws_free)                       # what the third pass finds free: about half of what the workspace took when it had the device
            extra = ballast.free_bytes() - want_free
            assert extra > 0, "the device has less free memory than the shortage this test wants to create"
            ballast.hold(extra)
            run3 = host.Run(ds, prm, ctx.backend(), None)
            run3.all()
            m3 = ctx.poa_memory_stats()
            print("configs4 share under real shortage: ballast %.1f GB, free at the consensus call %.1f GB, budget %.1f GB, workspace settled on %.1f GB (unconstrained: %.1f GB)" %
                  (ballast.bytes / 1e9, m3["free_at_first_call"] / 1e9, m3["budget"] / 1e9, m3["last_call_workspace"] / 1e9, ws_free / 1e9))
            assert run3.cns_out() == cns1 and run3.assembly_fasta() == fasta1
            assert m3["last_call_workspace"] <= m3["budget"] < ws_free          # the budget path ran short, for real, and held
            run3.close()
        finally:
            ballast.release()
            ctx.poa_release_workspace()
        print("configs4 share, resident inputs per GPU:", resident)
        assert resident["packed_read_bytes"] + resident["cigar_word_bytes"] < 40e9          # (400 Mb: ~2.6 + ~2.2 GB; x 7.75 for CHM1 = the replication cost per rank)
        o = subprocess.check_output([os.path.join(ROOT, "tools", "hxident"), pre + ".genome.fa", os.path.join(out, "asm.final.fa")], text=True)
        ident = float(o.strip().split("\n")[-1].split()[1])
        # identity against the SYNTHETIC TRUTH (not against the reference's output, which cannot be produced here: SPOA 1.1.3 is not in the image)
        assert ident >= 0.997, o[-500:]
        ds.close()
    finally:
        _drop_sim_files(pre)


def test_hairpin_reads_through_hip(sim, ctx, tmp_path):
    """missed-adapter reads (the palindrome rule of Longread.cpp:182-232 fires on every one of them): all stages identical to the oracle's"""
    pre = sim("--genome-len", "200000", "--seed", "8", "--variant-per-mb", "30", "--cov", "14", "--hairpin-frac", "0.1")
    ds = host.Dataset(pre + ".contigs.fa", pre + ".reads.fa", pre + ".paf")
    ro, rg, ob = both(ds, ctx, str(tmp_path / "o"), str(tmp_path / "g"))
    assert_same_arrays(ro.chain_out(), rg.chain_out(), "chain")
    assert_same_arrays(ro.edges_out(), rg.edges_out(), "edges")
    assert ro.cns_out() == rg.cns_out() and ro.assembly_fasta() == rg.assembly_fasta()
    assert util.compare_dirs(str(tmp_path / "o"), str(tmp_path / "g")) == []


def _read_text(ds, rid, strand=0):
    n = ds.reads.len[rid]
    off = ds.reads.off[rid]
    s = "".join("ACGT"[(ds.reads.packed[off + (i >> 2)] >> ((i & 3) * 2)) & 3] for i in range(n))
    return s if strand == 0 else s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def test_poa_supports_edge_cases_through_hip(sim, ctx):
    """the sub-sequence rule of Assemble.cpp:530-551 on the device: epos + 1 < spos wraps in 32 bits and takes the rest of the read,
    epos + 1 == spos is an empty sequence and is skipped, an edge whose sequences are all empty has an empty consensus, spos beyond
    the read is an error; every consensus equals the oracle's on the same substrings"""
    pre = sim("--genome-len", "60000", "--seed", "26", "--variant-per-mb", "40", "--cov", "14")
    ds = host.Dataset(pre + ".contigs.fa", pre + ".reads.fa", pre + ".paf")
    ctx.upload(ds)
    lens = [ds.reads.len[i] for i in range(8)]
    r0 = _read_text(ds, 0)
    a, b = 100, 700
    edges = [
        [(0, 0, a, b - 1), (0, 0, a + 3, b + 5), (0, 0, a, b - 1)],                       # plain
        [(0, 0, lens[0] - 400, lens[0] - 402), (0, 0, lens[0] - 400, lens[0] - 1)],       # wrap: epos + 1 < spos -> tail of the read from spos
        [(0, 0, 50, 49), (1, 1, 10, 9)],                                                  # every sequence empty -> ""
        [(0, 0, 50, 49), (0, 0, a, b - 1), (0, 1, 20, 19)],                               # empty ones skipped
        [(0, 0, lens[0], 5)],                                                             # spos == length: empty after the clamp
        [(0, 1, 30, 629), (0, 1, 30, 629)],                                               # reverse strand
    ]
    got = ctx.poa_supports(edges)
    rc0 = _read_text(ds, 0, 1)
    want = [orclib.poa_consensus([r0[a:b], r0[a + 3:b + 6], r0[a:b]]), orclib.poa_consensus([r0[lens[0] - 400:], r0[lens[0] - 400:]]), "",
            orclib.poa_consensus([r0[a:b]]), "", orclib.poa_consensus([rc0[30:630]] * 2)]
    assert got == want
    assert got[1] == r0[lens[0] - 400:] and got[3] == r0[a:b]
    with pytest.raises(hip.HipError):
        ctx.poa_supports([[(0, 0, lens[0] + 1, lens[0] + 10)]])                           # the reference would throw std::out_of_range


def test_poa_known_answers_through_hip(ctx):
    """the known-answer sets of tests/test_poa_known_answers.py through the HIP kernel (hx_poa_sequences), and random noisy sets against the oracle"""
    import random
    s = "ACGTTGCAAGGCTTAACCGGTACGATCGATTAGC"
    a = "ACGTACGTACGTTTGACCAGTACGGATCAAGGCT"
    sub = a[:10] + ("A" if a[10] != "A" else "C") + a[11:]
    dele, ins = a[:12] + a[15:], a[:12] + "GGG" + a[12:]
    sets = [[s] * 5, [s], [], ["", ""], ["A"], ["", "ACGT", ""], [a, sub, a], [sub, a, a], [sub, sub, a], [a, dele, a, a], [dele, dele, a, dele],
            [ins, a, a, a, ins], [ins, ins, a, ins]]
    rnd = random.Random(9)
    for _ in range(24):
        L = rnd.choice([1, 2, 3, 30, 63, 64, 65, 300, 700, 1500])
        t = "".join(rnd.choice("ACGT") for _ in range(L))

        def noisy():
            out = []
            for ch in t:
                r = rnd.random()
                if r < 0.05:
                    continue
                out.append(rnd.choice("ACGT") if r < 0.09 else ch)
                if rnd.random() < 0.04:
                    out.append(rnd.choice("ACGT"))
            return "".join(out)
        sets.append([noisy() for _ in range(rnd.choice([1, 2, 3, 9, 25]))])
    got = ctx.poa_sequences(sets)
    want = [orclib.poa_consensus(st) for st in sets]
    assert got == want
    assert got[0] == s and got[2] == "" and got[6] == a and got[8] == sub and got[10] == dele and got[12] == ins


def test_shared_edge_that_stalls_is_redone_unshared(sim, ctx):
    """a wave of a shared edge that gives up waiting for another workgroup's carry (forced here: HX_POA_POLL_LIMIT=0 makes every first poll a
    time-out) flags its edge; the host redoes exactly those edges with one workgroup each and the call succeeds with the oracle's consensus"""
    pre = sim("--genome-len", "150000", "--seed", "31", "--variant-per-mb", "15")
    ds = host.Dataset(pre + ".contigs.fa", pre + ".reads.fa", pre + ".paf")
    knobs = {"HX_POA_CLUSTER_MIN": "300", "HX_POA_MEMBER_LANES": "64", "HX_POA_CLUSTER_COLS": "4", "HX_POA_CLUSTER_MAX": "8", "HX_POA_POLL_LIMIT": "0"}
    with ctx.options(**knobs):
        ro, rg, ob = both(ds, ctx, None, None)
    assert ro.cns_out() == rg.cns_out() and ro.assembly_fasta() == rg.assembly_fasta()


def test_gap_longer_than_65535_columns(ctx):
    """a 70 000-base gap (shared by 16 workgroups, 32 columns per lane): three copies of one random sequence, two of them with sparse private
    substitutions - the consensus is the sequence itself (majority in every column)"""
    import random
    rnd = random.Random(70)
    L = 70000
    a = [rnd.choice("ACGT") for _ in range(L)]
    b, c = list(a), list(a)
    for k in range(0, L, 997):
        b[k] = "ACGT"[("ACGT".index(a[k]) + 1) % 4]
    for k in range(500, L, 1009):
        c[k] = "ACGT"[("ACGT".index(a[k]) + 2) % 4]
    a = "".join(a)
    got = ctx.poa_sequences([[a, "".join(b), "".join(c)], [a[:300]] * 2])
    assert got[0] == a and got[1] == a[:300]
    assert ctx.poa_sequences([["A" * 140000, "A" * 140000]]) == ["A" * 140000]   # (above 131 071 columns: 1024-lane members - until round 5 this failed the call)


@pytest.mark.parametrize("length,force_cm", [(3000, "32"), (17000, None)])
def test_one_workgroup_with_32_columns_per_lane(ctx, length, force_cm):
    """the 1024-lane, 32-columns-per-lane kernel on a BRANCHED graph (noisy copies: kept rows that leave the ring are read back from HBM):
    gaps of 16 384 to 32 767 columns in one workgroup reach it (forced here with the block size; HX_POA_FORCE_CM reaches it at any length).
    Its row loop spills registers; a cross-lane read of a row record inside a divergent block once picked up a lane the reload had skipped
    (round 3: wrong far-row slot -> wrong consensus or a memory fault) - found by tools/dev_fuzz.py, kept here."""
    import random
    rnd = random.Random(7 + length)

    def noisy(t, ins=0.06, dele=0.04, sub=0.03):
        out = []
        for ch in t:
            r = rnd.random()
            if r < dele:
                continue
            out.append(rnd.choice("ACGT") if r < dele + sub else ch)
            while rnd.random() < ins:
                out.append(rnd.choice("ACGT"))
        return "".join(out)

    tmpl = "".join(rnd.choice("ACGT") for _ in range(length))
    groups = [[noisy(tmpl) for _ in range(n)] for n in (3, 5)]
    want = [orclib.poa_consensus(g) for g in groups]
    try:
        with ctx.options(poa_force_cm=force_cm or 0):
            for dirb in (1, 0):
                ctx.set_poa_block(1024)
                hip.lib().hx_set_poa_traceback(ctx._h, dirb)
                assert ctx.poa_sequences(groups) == want, "traceback flavour %d" % dirb
    finally:
        ctx.set_poa_block(0)
        hip.lib().hx_set_poa_traceback(ctx._h, 1)


def test_gap_longer_than_the_default_members_hold(ctx):
    """a 150 000-base sub-sequence (what the u32 wrap of Assemble.cpp:530-532 makes of `epos + 1 < spos` on an ultra-long read: the whole tail) does
    not fail the call any more: above 131 071 columns the edge gets 1024-lane members (16 x 1024 lanes x 32 columns = 524 287). Too long for the
    oracle's full int32 matrix inside a test (90 GB), so known answers: three copies of one random sequence, two of them with sparse private
    substitutions, give the sequence back; the same shape at 3 000 bases with forced 1024-lane members is compared with the oracle bit for bit."""
    import random
    rnd = random.Random(1505)
    for length, knobs in ((3000, {"poa_member_lanes": 1024, "poa_cluster_min": 1000, "poa_cluster_max": 2, "poa_cluster_cols": 4}), (150000, {})):
        s = "".join(rnd.choice("ACGT") for _ in range(length))

        def mutated(step, off):
            t = list(s)
            for i in range(off, length, step):
                t[i] = "ACGT"[("ACGT".index(t[i]) + 1) % 4]
            return "".join(t)
        sets = [[s, mutated(997, 11), mutated(1009, 500)], [s[:length // 2], s[:length // 2]]]
        with ctx.options(**knobs):
            got = ctx.poa_sequences(sets)
        assert got[0] == s and got[1] == s[:length // 2], length
        if length <= 5000:
            assert got == [orclib.poa_consensus(st) for st in sets]
    # beyond what the score keys hold (2^20 columns) the call fails loudly, naming the limit
    with pytest.raises(hip.HipError, match="longer than the POA kernel"):
        ctx.poa_sequences([["A" * (1 << 20), "A" * 10]])


@huge
def test_read_arena_above_4_gib(sim, ctx, tmp_path):
    """five unreferenced filler reads of 3.6 Gbases ahead of the real ones: the packed 2-bit arena is 4.5 GB, EVERY read a hit or a consensus support names
    sits at a byte offset above 2^32 (the shape of a CHM1 rank: 20 GB of packed reads). Every stage array, every consensus and the
    assembly equal the oracle's on the same data set - K1's hit gathers, K5, K6's decode and the packed edge records with 64-bit offsets for real."""
    args = ("--genome-len", "2000000", "--seed", "4242", "--cov", "20", "--variant-per-mb", "10", "--filler-reads", "5", "--filler-len", "3600000000")
    pre = sim(*args)
    try:
        ds = host.Dataset(pre + ".contigs.fa", pre + ".reads.fa", pre + ".paf", threads=min(16, os.cpu_count() or 1))
        off = np.ctypeslib.as_array(ds.reads.off, shape=(int(ds.reads.n) + 1,))
        assert int(off[5]) > (1 << 32) and int(off[-1]) > (1 << 32), "the filler reads must push every real read beyond 4 GiB"
        ro, rg, ob = both(ds, ctx, str(tmp_path / "o"), str(tmp_path / "g"), threads=min(64, os.cpu_count() or 8))
        assert_same_arrays(ro.chain_out(), rg.chain_out(), "chain")
        assert_same_arrays(ro.edges_out(), rg.edges_out(), "edges")
        assert_same_arrays(ro.coords_out(), rg.coords_out(), "coords")
        sup = rg.coords_out()["supp_lr"]
        assert sup.size > 1000 and int((sup & 0x7fffffff).min()) >= 5          # supports name real reads only - all of them beyond the fillers
        assert ro.cns_out() == rg.cns_out() and rg.n_edges > 100
        assert util.compare_dirs(str(tmp_path / "o"), str(tmp_path / "g")) == []
        print("read arena: %.2f GB packed, first real read at byte %d, %d edges" % (int(off[-1]) / 1e9, int(off[5]), rg.n_edges))
        rg.close(); ro.close(); ob.close(); ds.close()
    finally:
        _drop_sim_files(pre)
