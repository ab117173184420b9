"""The diagnostic words of the tuned POA kernel (kernels/poa_phase_words.h) from the kernel to the report, on the smallest call that writes every word
of the default build: 3 sets of 3 noisy copies of a 300-base sequence, one-wave workgroups. The text of the report for given words is held in
test_poa_phase_report.py; here the words are the kernel's own."""
import importlib.util
import os
import random
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def noisy_sets():
    rng = random.Random(20240607)
    sets = []
    for _ in range(3):
        base = [rng.choice("ACGT") for _ in range(300)]
        copies = []
        for _ in range(3):
            s = []
            for ch in base:
                r = rng.random()
                if r < 0.03:
                    continue                                 # deletion
                s.append(rng.choice("ACGT") if r < 0.06 else ch)   # substitution
                if r > 0.97:
                    s.append(rng.choice("ACGT"))             # insertion
            copies.append("".join(s))
        sets.append(copies)
    return sets


@pytest.fixture(scope="module")
def ctx(built):
    from haslr_amd import hip
    c = hip.HipContext(0, use_env=False)   # raises without a device: these tests never run on a fallback
    yield c
    c.close()


def check_counters(ctx):
    ph, pr = ctx.poa_phase_cycles(), ctx.poa_prune_stats()
    assert ph["edges"] == 3
    for k, v in ph["slowest_edge"].items():
        assert v <= ph["sum"][k], k
    assert ph["sum"]["dp"] > 0
    assert pr["wave_rows_skipped"] <= pr["wave_rows"]
    return pr


def test_counters_default_and_unpruned(ctx):
    sets = noisy_sets()
    cns = ctx.poa_sequences(sets)
    assert len(cns) == 3 and all(250 < len(c) < 350 for c in cns)
    check_counters(ctx)
    with ctx.options(poa_prune=0):
        assert ctx.poa_sequences(sets) == cns
        assert check_counters(ctx) == {"wave_rows": 0, "wave_rows_skipped": 0, "attempts_repeated": 0, "alignments_with_threshold": 0}


CHILD = """
import sys
sys.path[:0] = [%r, %r]
from haslr_amd import hip
from test_poa_phase_words_gpu import noisy_sets
c = hip.HipContext(0, use_env=False)
c.set_option("debug", 2)
c.poa_sequences(noisy_sets())
print(c.poa_phase_cycles()["edges"])
c.close()
"""


def test_edge_lines_of_debug_2(built, tmp_path):
    """debug = 2 prints one [hx-edge] line per edge on stderr (a child process: the text comes from C stdio), and tools/dev_edge_timeline.py reads them"""
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"))], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split()[-1] == "3"
    lines = [ln for ln in r.stderr.splitlines() if ln.startswith("[hx-edge]")]
    assert len(lines) == 3, r.stderr[-2000:]
    spec = importlib.util.spec_from_file_location("dev_edge_timeline", os.path.join(ROOT, "tools", "dev_edge_timeline.py"))
    tl = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tl)
    err = tmp_path / "edges.err"
    err.write_text(r.stderr)
    E = tl.parse(str(err))
    assert sorted(d["e"] for d in E) == [0, 1, 2]
    for d in E:
        assert d["lanes"] == 64 and d["members"] == 1 and d["nseq"] == 3 and 250 < d["lmax"] < 350
        assert 0 <= d["begin_us"] <= d["end_us"] and d["dp"] > 0 and d["rows"] > 0
