"""The layout of a POA batch (PoaPlanner::layout_slots, ::layout_order and ::layout_launches, haslr_amd/csrc/hx_poa_plan.hip) is what the launch of a batch computed before it was a host step of
its own. tests/poa_layout_driver.cpp links the planner ALONE, compiled host-only (no HIP runtime in the link, no GPU), plans synthetic calls and prints the
layout of every batch. The golden text under tests/golden/poa_layout/ is not the output of the code under test: it was printed by the previous launch_batch,
compiled unchanged and linked to a fake runtime that recorded what it uploaded and launched ("The batch layout is a pure host step"), on the same
inputs (tests/poa_layout_text.h). Lines of the driver that begin with "+ " show what no upload carries (totals, classes, needs): the invariants read them."""
import gzip
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, ".."))
CSRC = os.path.join(ROOT, "haslr_amd", "csrc")
DRIVER = os.path.join(ROOT, "haslr_amd", "bin", "poa_layout_driver")
GOLDEN = os.path.join(HERE, "golden", "poa_layout")

# a: few edges (gaps of 40 .. 20000 bases x 3 and 6 sequences); b: with the score-matrix traceback forced; c_block / c_ring: with a block size of 256 / option
# poa_ring_zero; d: 3 300 small edges and 36 gaps; e: d under a budget of 0.4 GB; f: many edges, no column passes, a persistent 1024-lane class, option
# poa_resident_first = 3; g: a, then a second round of six edges that came back with one status each
CASES = ["a", "b", "c_block", "c_ring", "d", "e", "f", "g"]


def expected(case):
    p = os.path.join(GOLDEN, case + ".txt")
    if os.path.exists(p):
        with open(p) as f:
            return f.read()
    with gzip.open(p + ".gz", "rt") as f:
        return f.read()


@pytest.fixture(scope="module")
def driver():
    subprocess.check_call(["make", "-s", "-C", CSRC, DRIVER])   # (nothing to do when it is newer than the planner's sources)
    return DRIVER


_out = {}


def layout(driver, case):
    if case not in _out:
        r = subprocess.run([driver, case], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, check=True)
        assert r.stderr == ""
        _out[case] = r.stdout
    return _out[case]


def test_driver_links_no_hip_runtime(driver):
    libs = subprocess.run(["ldd", driver], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "amdhip" not in libs and "hsa" not in libs


@pytest.mark.parametrize("case", CASES)
def test_layout_is_what_the_launch_computed(driver, case):
    got = [ln for ln in layout(driver, case).splitlines() if not ln.startswith("+ ")]
    want = expected(case).splitlines()
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"case {case}, line {i + 1}"
    assert len(got) == len(want)


def fields(line):
    """'launch 0 stream 1 code 2 ...' -> {'launch': '0', 'stream': '1', ...}"""
    t = line.split()
    if len(t) % 2:   # (a first word without a value: batch, totals)
        t = t[1:]
    return dict(zip(t[0::2], t[1::2]))


def test_cases_reach_every_branch():
    """what the cases rest on, read off the golden text itself"""
    text = {c: expected(c).splitlines() for c in CASES}
    every = [ln for c in CASES for ln in text[c]]
    launches = [fields(ln) for ln in every if ln.startswith("launch ")]
    batches = [fields(ln) for ln in every if ln.startswith("batch ")]
    assert any(ln.endswith(" hole") for ln in text["a"] if ln.startswith("order "))     # member counts that differ inside a group of 8
    assert any(int(q["dp_lanes"]) != 0 for q in launches)                                  # wide members
    assert any(q["code"] == "0" and q["cm"] == "2" for q in launches)                      # a 2-column member class
    assert any(int(q["code"]) >= 5 for q in launches) and any(int(q["code"]) >= 6 for q in launches)   # (6 and above: the score-matrix flavour)
    assert {q["wait"] for q in launches} == {"none", "started", "delay"}
    assert any(q["wait"] == "started" and q["counter_at"] != "-1" and int(q["block_threads"]) >= 512 for q in launches)   # a persistent wide class with the head start
    assert any(q["wait"] == "none" and q["counter_at"] == "-1" and q["block_threads"] == "512" for q in map(fields, (ln for ln in text["f"] if ln.startswith("launch "))))   # ... and one workgroup per edge: none
    assert any(int(b["shrink"]) < 1000 for b in batches) and any(b["by_work"] == "1" for b in batches)
    assert any(q["R"] == "0" for q in launches)
    assert any(int(q["prune_pct"], 16) != 0 and q["counter_at"] == "-1" and int(q["block_threads"]) in (256, 512) for q in launches)   # pruned unshared classes
    assert len([b for b in text["e"] if b.startswith("batch ")]) > 1 and len([b for b in text["g"] if b.startswith("batch ")]) == 2
    # a launch group of more than one class (need buckets of one instance): the first word of its table counts them
    for c in ("d",):
        btab = {int(ln.split()[1]): int(ln.split()[2]) for ln in text[c] if ln.startswith("btab ")}
        assert any((btab[int(fields(ln)["btab_at"])] & 0xffff) == 3 for ln in text[c] if ln.startswith("launch ") and fields(ln)["btab_at"] != "-1")
    assert len([ln for ln in text["d"] if ln.startswith("edge ")]) > 3000                   # many_edges


def batches_of(text):
    out = []
    for ln in text.splitlines():
        if ln.startswith("batch "):
            out.append([])
        out[-1].append(ln)
    return out


@pytest.mark.parametrize("case", CASES)
def test_layout_invariants(driver, case):
    for lines in batches_of(layout(driver, case)):
        head = fields(lines[0])
        plus = [ln[2:] for ln in lines if ln.startswith("+ ")]
        # the budget counts what the layout takes
        tb = fields(next(ln for ln in plus if ln.startswith("total_bytes ")))
        assert int(tb["total_bytes"]) == int(head["bytes"]) <= int(tb["budget"])
        # the pools: 256-aligned, one after the other, to the end of the arena
        off = [(ln.split()[1], int(ln.split()[2])) for ln in lines if ln.startswith("pool ")]
        size = {ln.split()[1]: int(ln.split()[2]) for ln in plus if ln.startswith("pool_size ")}
        assert len(off) == 41 and off[0][1] == 0
        ends = [o for _, o in off[1:]] + [int(head["arena"])]
        for (name, o), end in zip(off, ends):
            assert o % 256 == 0 and end == o + max(256, (size[name] + 255) // 256 * 256), name
        # every slot inside its pools' totals
        tot = fields(next(ln for ln in plus if ln.startswith("totals ")))
        need = {int(ln.split()[1]): fields(ln) for ln in plus if ln.startswith("need ")}
        slots = [fields(ln) for ln in lines if ln.startswith("slot ")]
        assert len(need) == len(slots)
        pairs = [("node", "nn", "no"), ("edge", "ec", "eo"), ("h", "hc", "ho"), ("d", "dc", "dro"), ("w", "wc", "wo"), ("seq", "lm", "so"), ("stack", "st", "sto"), ("aln", "al", "ao"), ("mbox", "mb", "clo")]
        for s in slots:
            for at, n, total in pairs:
                assert int(s[at]) + int(need[int(s["slot"])][n]) <= int(tot[total])
        assert int(tot["clo"]) == int(head["mailbox_words"])
        # the order list: every edge of an unshared class once, every (edge, member) of a shared class once, holes apart
        members = {int(fields(ln)["edge"]): int(fields(ln)["members"]) for ln in lines if ln.startswith("edge ")}
        order = []
        for ln in lines:
            if ln.startswith("order "):
                t = ln.split()
                order.append(None if t[2] == "hole" else (int(t[3]), int(t[5])))
        at = 0
        for ln in plus:
            if not ln.startswith("class "):
                continue
            t = ln.split()
            q = dict(zip(t[0:t.index("edges"):2], t[1:t.index("edges"):2]))
            edges = [int(e) for e in t[t.index("edges") + 1:]]
            assert int(q["order_at"]) == at
            n = int(q["blocks"]) if q["shared"] == "1" else len(edges)
            seen = [x for x in order[at:at + n] if x is not None]
            want = [(e, m) for e in edges for m in range(members[e])] if q["shared"] == "1" else [(e, 0) for e in edges]
            assert sorted(seen) == sorted(want) and len(set(seen)) == len(seen)
            assert q["shared"] == "1" or len(seen) == n
            at += n
        assert at == len(order) and sorted(members) == sorted({x[0] for x in order if x is not None})
