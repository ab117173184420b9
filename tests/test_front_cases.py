"""The front half on hand-built PAF edge cases (tests/frontcases.py): the oracle with the host pipeline against the compiled reference
front half, byte for byte, and every family's manifest against the oracle's output, so that the planted branches are shown to be
reached: reads with more than 64 raw hits, trim walks that stop in every CIGAR letter on both strands, filters at exact equality, the
palindrome rule at group positions past a wavefront, ties, and edges with more than 384 supports."""
import collections
import os
import subprocess

import numpy as np
import pytest

import frontcases as fc
import orclib
import util
from haslr_amd import host


@pytest.fixture(scope="module")
def cases(built, tmp_path_factory):
    made = {}

    def get(name):
        if name not in made:
            made[name] = fc.build(str(tmp_path_factory.mktemp(name)), [name])
        return made[name]
    return get


def oracle(pre, out_dir, stages=("chain", "graph")):
    ds = host.Dataset(pre + ".contigs.fa", pre + ".reads.fa", pre + ".paf")
    be = orclib.OracleBackend(ds, 4)
    run = host.Run(ds, ds.params(), be.table, out_dir)
    for s in stages:
        getattr(run, s)()
    return ds, be, run


def run_ref(ref_front, pre, out):
    os.makedirs(out, exist_ok=True)
    subprocess.check_call([ref_front, "-c", pre + ".contigs.fa", "-l", pre + ".reads.fa", "-m", pre + ".paf", "-d", out],
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)


@pytest.mark.parametrize("family", fc.FAMILIES + ("combined",))
def test_oracle_equals_the_reference(family, cases, ref_front, tmp_path):
    if family == "combined":
        pre, case = fc.build(str(tmp_path / "in"), fc.FAMILIES, seed=7)
    else:
        pre, case = cases(family)
    rd, od = str(tmp_path / "ref"), str(tmp_path / "orc")
    run_ref(ref_front, pre, rd)
    ds, be, run = oracle(pre, od)
    assert util.compare_dirs(rd, od) == []
    assert len([f for f in os.listdir(od) if f.endswith(".gfa")]) == 6
    chain, edges = run.chain_out(), run.edges_out(sides=False)
    n_other = fc.fixed_paf_equal(case, ds, chain, open(os.path.join(rd, "alignments.fixed.paf")).read())
    assert n_other > 0 or family in ("thresholds", "palindrome")
    assert util.edge_supp_text(edges) == open(os.path.join(rd, "edge_supp.01.txt")).read()
    keep = util.gfa_edge_keys(os.path.join(od, "backbone.06.smallbubble.gfa"))
    assert util.edge_supp_text(edges, keep) == open(os.path.join(rd, "edge_supp.06.txt")).read()
    run.close(); be.close(); ds.close()


def check_manifest(case, chain, edges, coords=None):
    """what each family planted really happened in the oracle's output; returns the trim walks of the modelled reads"""
    man = case.man
    hits_of_read = collections.defaultdict(list)
    for h in case.hits:
        hits_of_read[h.read].append(h)
    kept = set(chain["hit"].tolist())
    chained = set(chain["hit"][chain["cmp_aln"]].tolist())
    for key, inside, where in (("kept", True, kept), ("dropped", False, kept), ("chained", True, chained), ("unchained", False, chained)):
        for tag in man[key]:
            idx = case.tagged(tag)
            assert idx, f"{tag}: nothing planted"
            for i in idx:
                assert (i in where) == inside, f"{tag} (hit {i}) is not {key}"
    n_aln = np.diff(chain["read_off"])
    for r, n in man["n_aln"].items():
        assert n_aln[r] == n, f"read {r}: {n_aln[r]} alignments, planted {n}"
    for r in man["serial_reads"]:
        assert len(hits_of_read[r]) > 64
    # the trims, restated per base
    walks = {"wave": [], "serial": []}
    ro = chain["read_off"]
    for r in man["model_reads"]:
        rows, w = fc.trim_model(hits_of_read[r])
        b = int(ro[r])
        assert int(ro[r + 1]) - b == len(rows), f"read {r}"
        for k, row in enumerate(rows):
            got = tuple(int(chain[f][b + k]) for f in ("hit", "q_start", "q_end", "t_start", "t_end", "n_match", "n_block"))
            assert got == tuple(row[f] for f in ("index", "qs", "qe", "ts", "te", "nm", "nb")), f"read {r} alignment {k}"
        walks["serial" if len(hits_of_read[r]) > 64 else "wave"] += w
    # edges between contigs
    ek = edges["edge_key"].astype(np.uint64)
    pairs = {(min(a, b), max(a, b)) for a, b in zip((ek >> np.uint64(33)).tolist(), ((ek & np.uint64(0xffffffff)) >> np.uint64(1)).tolist())}
    for p in man["pairs"]:
        assert tuple(p) in pairs, f"no edge between contigs {p}"
    for p in man["no_pair"]:
        assert tuple(p) not in pairs, f"an edge between contigs {p}"
    recs = {}
    for i, key in enumerate(ek.tolist()):
        a, b = key >> 33, (key & 0xffffffff) >> 1
        recs[(min(a, b), max(a, b))] = int(edges["edge_off"][i + 1] - edges["edge_off"][i])
    for p, n in man["edge_records"]:
        assert recs.get(tuple(p)) == n, f"edge {p}: {recs.get(tuple(p))} supports, planted {n}"
    if coords is not None and man["edge_records"]:
        per_edge = np.diff(coords["supp_off"])
        assert (per_edge > 0).sum() >= len(man["edge_records"])
    return walks


@pytest.mark.parametrize("family", fc.FAMILIES + fc.GPU_ONLY)
def test_manifest_holds(family, cases):
    pre, case = cases(family)
    stages = ("chain", "graph", "coords") if family == "coords" else ("chain", "graph")
    ds, be, run = oracle(pre, None, stages)
    walks = check_manifest(case, run.chain_out(), run.edges_out(sides=False), run.coords_out() if family == "coords" else None)
    if family == "trims":
        for path in ("wave", "serial"):
            w = walks[path]
            stops = collections.Counter((s, stop) for s, _, stop, _ in w)
            for strand in "+-":
                for letter in "MID" + fc.OTHER:   # a walk stopped at every letter, on both strands
                    assert stops[(strand, letter)] > 0, (path, strand, letter, stops)
            assert sum(1 for *_, oth in w if oth > 0) >= 10, path   # OTHER bases kept behind the last M (never undone)
            assert sum(1 for _, _, stop, _ in w if stop is None) > 0, path    # the ops ran out: a target behind the start
    if family == "hit_counts":
        assert max(np.diff(run.chain_out()["read_off"])) >= 1000
    run.close(); be.close(); ds.close()


@pytest.mark.parametrize("n_reads", [1025, (1 << 20) + 1030])
def test_many_reads_manifest_holds(n_reads, tmp_path):
    """hit_counts spread over 1 025 and 2^20 + 1 030 reads (the GPU test of the scans over the reads, test_edge_records_gpu.py): the
    reads keep what the family planted, and those at the scans' edges carry alignments and pairs"""
    pre, case = fc.build(str(tmp_path / "in"), ["hit_counts"], n_reads=n_reads, reads_at=fc.many_reads_at(n_reads))
    assert fc.many_reads_edges(n_reads) == ([0, 1023, 1024] if n_reads == 1025 else [0, 1023, 1024, 1025, (1 << 20) - 1, 1 << 20, n_reads - 1])
    assert set(fc.many_reads_edges(n_reads)) <= set(fc.many_reads_at(n_reads)) and len(set(fc.many_reads_at(n_reads))) == 10
    ds, be, run = oracle(pre, None)
    assert ds.reads.n == n_reads
    check_manifest(case, run.chain_out(), run.edges_out(sides=False))
    fc.check_many_reads(case, n_reads, run.chain_out(), run.edges_out(sides=False))
    run.close(); be.close(); ds.close()
