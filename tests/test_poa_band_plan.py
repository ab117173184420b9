"""The band's part of the general POA path's plan (describe, slot_of, plan_round, after_round; haslr_amd/csrc/kernels/poa_modes_plan.hip),
through tests/poa_band_plan_driver.cpp, which links the plan ALONE, compiled host-only: the size of a banded slot for the three gap models,
the escalation w, 2 w, ... and then the full matrix, both kinds of rerun in one call, a call without a band planned as before, and the two
refusals the plan makes."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, ".."))
CSRC = os.path.join(ROOT, "haslr_amd", "csrc")
DRIVER = os.path.join(ROOT, "haslr_amd", "bin", "poa_band_plan_driver")
CELL = {0: 4, 1: 8, 2: 12}
BAND_SLOT = 4   # behind the four full-matrix instances
COLUMNS = {0: [64 * 16, 256 * 16, 256 * 32, 1024 * 32], 1: [64 * 16, 256 * 16, 512 * 16, 1024 * 16], 2: [64 * 16, 128 * 16, 256 * 16, 512 * 16]}


@pytest.fixture(scope="module")
def driver():
    subprocess.check_call(["make", "-s", "-C", CSRC, DRIVER])   # (nothing to do when it is newer than the plan's sources)
    return DRIVER


def plan(driver, gm, band, slot_kb, misses, sets, score=8):
    r = subprocess.run([driver, str(gm), str(band), str(slot_kb), str(misses), str(score)] + [",".join(str(v) for v in s) for s in sets], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, check=True)
    assert r.stderr == ""
    out = dict(sets=[], slots=[], done={}, reruns=None, error=None)
    for ln in r.stdout.splitlines():
        f = ln.split()
        if f[0] == "set":
            out["sets"].append({f[k]: int(f[k + 1]) for k in range(0, len(f), 2)})
        elif f[0] == "slot":
            out["slots"].append({f[k]: int(f[k + 1]) for k in range(0, len(f), 2)})
        elif f[0] == "done":
            out["done"][int(f[1])] = int(f[3])
        elif f[0] == "reruns":
            out["reruns"] = (int(f[2]), int(f[4]))
        else:
            out["error"] = ln[len("error "):]
    return out


def al256(v):
    return (v + 255) // 256 * 256


def test_driver_links_no_hip_runtime(driver):
    libs = subprocess.run(["ldd", driver], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "amdhip" not in libs and "hsa" not in libs


@pytest.mark.parametrize("gm", [0, 1, 2])
def test_a_banded_slot_holds_the_windows_and_the_three_row_arrays(driver, gm):
    sets = [[3000, 2900, 3100], [1500, 1500]]
    for w in (8, 64, 511):
        p = plan(driver, gm, w, 0, 0, sets)
        assert p["error"] is None and p["reruns"] == (0, 0) and p["done"] == {0: w, 1: w}
        B = 2 * w + 1
        for s in p["sets"]:
            lens = sets[s["set"]]
            assert s["vest"] == min(sum(lens), max(lens) + sum(lens) // 8 + 64)   # (the estimate is the unbanded one)
            assert s["slot"] == BAND_SLOT and s["band"] == w
            assert s["need"] == s["pools"] + al256((s["vest"] + 1) * B * CELL[gm] + 12 * (s["vest"] + 1))
        assert [sl["slot"] for sl in p["slots"]] == [BAND_SLOT] and p["slots"][0]["bytes"] == max(s["need"] for s in p["sets"])
        # against the full matrix of the same call: H shrinks by (L + 1) / B, but for the row arrays
        q = plan(driver, gm, 0, 0, 0, sets)
        for s, f in zip(sorted(p["sets"], key=lambda d: d["set"]), sorted(q["sets"], key=lambda d: d["set"])):
            L = max(sets[s["set"]])
            assert f["need"] - f["pools"] == al256((f["vest"] + 1) * (L + 1) * CELL[gm]) and f["pools"] == s["pools"] and f["vest"] == s["vest"]
            assert (s["need"] - s["pools"]) * (L + 1) <= (f["need"] - f["pools"] + 256) * (B + 3) + 256 * (L + 1)


def test_a_set_that_fits_the_window_runs_on_the_full_matrix(driver):
    p = plan(driver, 0, 100, 0, 0, [[200, 150], [201, 10], [0, 0]])
    assert p["done"] == {0: 0, 1: 100, 2: 0} and p["reruns"] == (0, 0)
    assert {s["set"]: (s["slot"], s["band"]) for s in p["sets"]} == {0: (0, 0), 1: (BAND_SLOT, 100)}   # (a set without a base is in no round)


@pytest.mark.parametrize("gm", [0, 1, 2])
def test_the_escalation_doubles_the_band_and_ends_on_the_full_matrix(driver, gm):
    sets = [[2000, 2400]]
    for misses, rungs in ((0, [8]), (1, [8, 16]), (3, [8, 16, 32, 64]), (5, [8, 16, 32, 64, 128, 256]), (6, [8, 16, 32, 64, 128, 256, 0]), (9, [8, 16, 32, 64, 128, 256, 0])):
        p = plan(driver, gm, 8, 0, misses, sets)
        assert [s["band"] for s in p["sets"]] == rungs and p["done"] == {0: rungs[-1]} and p["reruns"] == (0, len(rungs) - 1)
        assert [s["round"] for s in p["sets"]] == list(range(len(rungs)))
        full = 0 in rungs
        assert [s["slot"] for s in p["sets"]] == [BAND_SLOT] * (len(rungs) - full) + [next(k for k, c in enumerate(COLUMNS[gm]) if c >= 2401)] * full
    # the ladder stops where twice the band would pass 1023 columns, or would hold the longest sequence
    assert [s["band"] for s in plan(driver, gm, 300, 0, 9, sets)["sets"]] == [300, 0]
    assert [s["band"] for s in plan(driver, gm, 200, 0, 9, [[700, 600]])["sets"]] == [200, 0]   # (2 x 400 + 1 columns hold 701)
    assert [s["band"] for s in plan(driver, gm, 511, 0, 9, sets)["sets"]] == [511, 0]


def test_both_reruns_in_one_call_and_each_stays_bounded(driver):
    p = plan(driver, 1, 8, 1, 2, [[200, 240], [300, 300, 300]])
    assert p["error"] is None and p["done"] == {0: 32, 1: 32}
    assert p["reruns"][0] >= 1 and p["reruns"][1] == 4   # (the capped slot is the largest pools: it holds no row of that set)
    assert max(s["round"] for s in p["sets"]) <= 2 + 2 + 2   # (a slot rerun at most doubles the rows up to the set's bases; a band rerun climbs one rung)


@pytest.mark.parametrize("gm", [0, 1, 2])
def test_a_call_without_a_band_is_planned_as_before(driver, gm):
    sets = [[900, 1000], [1023, 5], [1024, 1024], [4000, 3000, 10]]
    p = plan(driver, gm, 0, 0, 5, sets)
    assert p["error"] is None and p["done"] == {i: 0 for i in range(4)} and p["reruns"][1] == 0
    for s in p["sets"]:
        L = max(sets[s["set"]])
        assert s["band"] == 0 and s["slot"] == next(k for k, c in enumerate(COLUMNS[gm]) if c >= L + 1)
        assert s["need"] == s["pools"] + al256((s["vest"] + 1) * (L + 1) * CELL[gm])
    assert all(sl["slot"] < BAND_SLOT for sl in p["slots"])


def test_the_plans_refusals(driver):
    assert plan(driver, 0, 512, 0, 0, [[10]])["error"] == "hx_poa_banded: the band half-width must be 1..511, not 512"
    assert plan(driver, 0, 8, 0, 0, [[10], [30000, 30000]], score=3000)["error"] == ("hx_poa_banded: set 1 holds 60000 bases, its longest sequence 30000: with scores of up to 3000 their product 270000000 "
                                                                                  "reaches 2^28 = 268435456 (a banded set's scores must stay below it)")
    assert plan(driver, 0, 8, 0, 0, [[10], [30000, 30000]], score=2982)["error"] is None   # (90 000 x 2 982 = 268 380 000, just below)
    assert plan(driver, 2, 8, 0, 0, [[8192]])["error"].startswith("hx_poa_banded: set 0 holds a sequence of 8192 bases, longer than 8191")
    assert plan(driver, 0, 0, 0, 0, [[10], [30000, 30000]], score=3000)["error"] is None   # (without a band only the full matrix's bound holds: (60 000 + 32 768 columns) x 3 000 stays below 2^29)
