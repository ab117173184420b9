"""bench.py's outputs: --dump-outputs writes what a caller of the timed path receives (CPU: the format and the size cap; GPU: a plain line
over a small genome, its dump equal to the CPU oracle's pass over the same files), and a plain line carries the headline without the --full extras."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import orclib
from haslr_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def _oracle_pass(pre):
    """(dataset, oracle backend, run) after the timed path's stages over the files of `pre`, on the CPU oracle"""
    ds = host.Dataset(pre + ".contigs.fa", pre + ".reads.fa", pre + ".paf")
    ob = orclib.OracleBackend(ds, 4)
    run = host.Run(ds, ds.params(), ob.table, None)
    run.chain(); run.graph(); run.coords(); run.consensus()
    return ds, ob, run


def test_dump_is_exact_and_capped(sim, tmp_path):
    pre = sim("--genome-len", "120000", "--seed", "23")
    ds, ob, run = _oracle_pass(pre)
    bench.dump_outputs(run, str(tmp_path / "a"))
    a = _load(str(tmp_path / "a"))
    assert run.n_edges > 0 and all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert a["consensus.offsets"].size == run.n_edges + 1 and a["consensus.bases"].size == a["consensus.offsets"][-1]
    assert set(np.unique(a["consensus.bases"]).astype(np.uint8).tobytes()) <= set(b"ACGT")
    e = run.edges_out()
    assert np.array_equal(a["edges.edge_key_from"].astype(np.uint64) << np.uint64(32) | a["edges.edge_key_to"].astype(np.uint64), e["edge_key"])
    assert np.array_equal(a["chain.q_start"], run.chain_out()["q_start"].astype(np.float64))
    # above the cap: every array cut to the same fraction, by the same positions from run to run
    total = sum(v.nbytes for v in a.values())
    cap = total // 3
    r1 = bench.dump_outputs(run, str(tmp_path / "b"), limit=cap)
    r2 = bench.dump_outputs(run, str(tmp_path / "c"), limit=cap)
    run.close(); ob.close(); ds.close()
    b, c = _load(str(tmp_path / "b")), _load(str(tmp_path / "c"))
    assert 0 < r1["sampled_fraction"] < 1 and r1 == {**r2, "dir": r1["dir"]}
    assert sum(os.path.getsize(os.path.join(tmp_path, "b", f)) for f in os.listdir(tmp_path / "b")) <= cap
    assert b.keys() == a.keys() and all(np.array_equal(b[k], c[k]) for k in b)
    assert all(np.isin(b[k], a[k]).all() for k in b)


@pytest.mark.gpu
def test_plain_line_and_its_dump(built, tmp_path, monkeypatch):
    """`bench.py --gpus 1 --steps 3 --warmup 1 --dump-outputs DIR` over a 200 kb genome: `steps` timed passes, `ms_per_step` = one of them, none of
    the --full extras, and the dump equals the CPU oracle's pass over the same input files, array for array."""
    env = dict(os.environ, HASLR_BENCH_DIR=str(tmp_path / "data"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--genome-len", "200000",
                        "--dump-outputs", str(tmp_path / "gpu")], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().split("\n")[-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["higher_is_better"] is True
    assert abs(line["value"] - line["config"]["long_read_bases"] / (line["ms_per_step"] / 1e3)) <= 1e-6 * line["value"]
    assert sum(" step " in x for x in r.stderr.splitlines()) == 3
    assert not {"cpu_baseline", "configs1", "configs3", "one_shot", "assembly", "gfa"} & line.keys()
    monkeypatch.setenv("HASLR_BENCH_DIR", env["HASLR_BENCH_DIR"])
    pre = bench.make_dataset(bench.WORKLOADS["yeast"], 200000, "gpu")   # the files the line read (made by it, found by name)
    ds, ob, run = _oracle_pass(pre)
    bench.dump_outputs(run, str(tmp_path / "orc"))
    run.close(); ob.close(); ds.close()
    g, o = _load(str(tmp_path / "gpu")), _load(str(tmp_path / "orc"))
    assert g.keys() == o.keys() and len(g) > 40
    for k in o:
        assert g[k].dtype == o[k].dtype and np.array_equal(g[k], o[k]), k
