"""The phase's part of the general POA path's plan (describe, plan_round, plan_coverage, plan_msa; haslr_amd/csrc/kernels/poa_modes_plan.hip),
through tests/poa_phase_plan_driver.cpp, which links the plan ALONE, compiled host-only: the size of the phase pool, that a phased call
plans the consensus places, the coverage blocks and the rows of a labelled call with two labels, that only its slots are larger, by the
phase pool, and that a call without `phase` plans what it planned before."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "haslr_amd", "bin", "poa_phase_plan_driver")
# three sets: the hand-sized one, one with an empty and an unassigned sequence, one whose second haplotype is empty (unphased)
SETS = ["5:0,5:0,5:1,5:1", "40:0,0:255,38:1,41:255,3:1,1:0", "70:0,64:0,65:0"]


def run(*args):
    return subprocess.check_output([DRIVER, *[str(a) for a in args]], text=True).splitlines()


def al256(x):
    return (x + 255) // 256 * 256


def pool_bytes(t, nseq):
    """carve_phase (kernels/poa_modes_pools.inl), restated: per column (at most one per base, + 1) four letter counts, the depth, the site
    prefix and the base's word; per site (at most one per column, + 1) six words; per sequence (+ 1) two; eight words of
    block-wide scalars; every array on 256 bytes"""
    cc = t + 1
    return al256(16 * cc) + 9 * al256(4 * cc) + 2 * al256(4 * (nseq + 1)) + 256


@pytest.mark.parametrize("t,nseq", [(1, 1), (2, 2), (64, 1), (64, 64), (65, 3), (65, 65), (1, 1000), (1 << 21, 7)])
def test_the_phase_pool(built, t, nseq):
    assert int(run("pool", t, nseq)[0]) == pool_bytes(t, nseq)


def test_the_pool_at_the_smallest_shapes(built):
    # a set of one-base sequences: every array still holds its + 1 (the mark behind the last column, the prefix behind the last site,
    # the total behind the last sequence), each on its own 256 bytes
    assert int(run("pool", 1, 1)[0]) == 13 * 256 and int(run("pool", 2, 2)[0]) == 13 * 256
    assert int(run("pool", 64, 64)[0]) == al256(16 * 65) + 9 * 512 + 2 * 512 + 256 == 1280 + 11 * 512 + 256
    assert int(run("pool", 63, 63)[0]) == 1024 + 12 * 256


def split(lines):
    slots = [ln for ln in lines if ln.startswith("slot ")]
    pools = [ln for ln in lines if ln.startswith("set ")]
    rest = [ln for ln in lines if not ln.startswith(("slot ", "set "))]
    return slots, pools, rest


def test_a_phased_call_plans_a_two_label_call(built):
    ph, lb = run("phase", 2, 25, *SETS), run("label", 2, 25, *SETS)
    ps, pp, prest = split(ph)
    ls, lp, lrest = split(lb)
    assert prest == lrest and prest[0] == "call labels 1 nl 2 cols 1 cov 1"
    # two consensus places per set, a counter block per (set, haplotype), two consensus rows behind the sequences' rows
    assert prest[1] == "cns_off 0 20 40 163 286 485 684"
    assert [ln for ln in prest if ln.startswith("cov stride")] == [f"cov stride 4 hist {4 * 2 * (5 + 41 + 70)} nc {5 + 5 + 41 + 41 + 70}"]
    assert sum(ln.startswith("cov_cns") for ln in prest) == 5 and [ln for ln in prest if ln.startswith("msa_rows")] == ["msa_rows 6 8 5"]
    # the sequence without a haplotype and the one of one base count nowhere
    assert sum(ln.startswith("cov_seq") for ln in prest) == 4 + 3 + 3
    # the slots: larger by the phase pool, set by set
    sizes = [(20, 4), (123, 6), (199, 3)]
    for a, b in zip(sorted(pp), sorted(lp)):
        i = int(a.split()[1])
        assert int(a.split()[3]) - int(b.split()[3]) == pool_bytes(*sizes[i]) and b.split()[:2] == a.split()[:2]
    assert len(ps) == len(ls) and all(int(a.split()[3]) > int(b.split()[3]) and a.split()[4:] == b.split()[4:] for a, b in zip(ps, ls))


def test_a_call_without_phase_plans_what_it_planned_before(built):
    # the same sets as a weighted call: one place per set, and the slots hold the graph pools alone (what the labelled call's hold)
    wt, lb = run("weighted", 0, 0, *SETS), run("label", 2, 25, *SETS)
    ws, wp, wrest = split(wt)
    ls, lp, _ = split(lb)
    assert wrest[0] == "call labels 0 nl 1 cols 1 cov 1" and wrest[1] == "cns_off 0 20 143 342"
    assert (ws, wp) == (ls, lp)
    # (this holds a call without `phase` to the graph pools alone; that those are what they were is held by the golden plans of
    # tests/test_poa_modes_plan.py, which pass untouched: its driver links the same plan)


def test_the_plan_refuses_what_a_phased_call_cannot_be(built):
    assert run("phase", 0, 25, "5:0")[0] == "error hx_poa_phased: min_count must be 1..255, not 0"
    assert run("phase", 256, 25, "5:0")[0] == "error hx_poa_phased: min_count must be 1..255, not 256"
    assert run("phase", 2, 0, "5:0")[0] == "error hx_poa_phased: min_pct must be 1..50, not 0"
    assert run("phase", 2, 51, "5:0")[0] == "error hx_poa_phased: min_pct must be 1..50, not 51"
