"""spoa::hx::strand_batch of include/spoa_hx.hpp through a small caller (tests/spoa_strand_caller.cpp): without a device it fails loudly;
on the MI355X it prints the restatement's consensus, flags, scores and rows for sets of mixed types and gap models."""
import os
import subprocess

import pytest

import strlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def strand_caller(built, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("spoa_strand") / "spoa_strand_caller")
    lib = os.path.join(ROOT, "haslr_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "spoa_strand_caller.cpp"), "-o", exe,
                           "-L", lib, "-lhaslr_hip", "-pthread", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def text_of(edges):
    return "\n".join(f"{mode} {' '.join(str(v) for v in sc)}{' +c' if c else ''}\n" + "".join((q or "-") + "\n" for q in st) for mode, sc, c, st in edges)


def test_strand_batch_without_a_device_fails_loudly(strand_caller):
    import torch
    r = subprocess.run([strand_caller], input=text_of([("nw", strlib.LINEAR, False, [strlib.S1, strlib.rc(strlib.S1)])]), capture_output=True, text=True)
    if torch.cuda.is_available():   # (a device is present: the same call works; the test below checks what it prints)
        assert r.returncode == 0 and r.stdout.endswith("=\n"), (r.returncode, r.stderr)
    else:
        assert r.returncode == 1 and "no HIP device" in r.stderr and r.stdout == "", (r.returncode, r.stderr)


@pytest.mark.gpu
def test_strand_batch_prints_the_restatements_answers(strand_caller, tmp_path):
    ref = strlib.StrandRef(str(tmp_path))
    sets = strlib.edge_sets(321)[:8] + strlib.tie_sets(322, 8) + [strlib.FOUR, ["", "ACGT", strlib.rc("ACGA")], []]
    kinds = [("nw", strlib.LINEAR, False), ("sw", strlib.AFFINE, True), ("ov", strlib.CONVEX, True), ("nw", strlib.CONVEX, False)]
    edges = [kinds[k % 4] + (st,) for k, st in enumerate(sets)]
    r = subprocess.run([strand_caller], input=text_of(edges), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [blk.split("\n")[:-1] for blk in r.stdout.split("=\n")[:-1]]
    want = []
    for mode, sc, c, st in edges:
        rec = ref.strand(st, mode, sc, include_consensus=c)
        want.append([rec.consensus, "".join("1" if f else "0" for f in rec.reversed), " ".join(f"{f}:{v}" for f, v in rec.scores)] + rec.rows)
    assert got == want
