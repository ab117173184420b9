"""The plan of the general POA path (describe, plan_round, after_round, plan_msa, plan_coverage and plan_graph_out, haslr_amd/csrc/kernels/poa_modes_plan.hip) is what
poa_modes_run computed between its HIP calls before those were host steps of their own. tests/poa_modes_plan_driver.cpp links the plan ALONE, compiled host-only (no
HIP runtime in the link, no GPU), runs synthetic calls through it and prints what would be uploaded and launched. The golden text under tests/golden/poa_modes_plan/ is
not the output of the code under test: it was printed by the previous poa_modes_run, compiled unchanged and linked to a fake runtime that recorded what it allocated,
uploaded and launched and answered every launch by the rule of tests/poa_modes_plan_text.h ("The general path's round plan and retry rule are pure host
steps"), on the same inputs. Lines of the driver that begin with "+ " show what no upload carries (needs, residents, the budget): the invariants read them."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, ".."))
CSRC = os.path.join(ROOT, "haslr_amd", "csrc")
DRIVER = os.path.join(ROOT, "haslr_amd", "bin", "poa_modes_plan_driver")
GOLDEN = os.path.join(HERE, "golden", "poa_modes_plan")

# edge_*: lmax + 1 at and one past the columns of every instance, per gap model; long_*, big_set: the limits; cap, cap_fail: option poa_modes_slot_kb = 1; status2,
# status3_plain: a set that leaves MS_GRAPH_OVERFLOW, and MS_ALN_OVERFLOW in a call without a graph; graph_*: a
# graph call under poa_graph_aln_cap = 1 (graph_both: and poa_modes_slot_kb = 1; aln2, ff, lie: the three errors of the alignment pool); budget, budget_over: a
# workspace of 9.5 MB and of 4 MB; msa, msa_nocns; cov, cov_prof; strand, strand_w: the output stages
CASES = ["edge_lin", "edge_aff", "edge_cvx", "long_lin", "long_aff", "long_cvx", "big_set", "cap", "cap_fail", "status2", "status3_plain", "graph_aln", "graph_both", "graph_aln2", "graph_ff", "graph_lie",
         "budget", "budget_over", "msa", "msa_nocns", "cov", "cov_prof", "strand", "strand_w"]
# lanes x columns per lane of the instances by gap model, and the longest sequence
COLUMNS = {"lin": [64 * 16, 256 * 16, 256 * 32, 1024 * 32], "aff": [64 * 16, 256 * 16, 512 * 16, 1024 * 16], "cvx": [64 * 16, 128 * 16, 256 * 16, 512 * 16]}
BLOCK = {"lin": [64, 256, 256, 1024], "aff": [64, 256, 512, 1024], "cvx": [64, 128, 256, 512]}


def expected(case):
    with open(os.path.join(GOLDEN, case + ".txt")) as f:
        return f.read()


@pytest.fixture(scope="module")
def driver():
    subprocess.check_call(["make", "-s", "-C", CSRC, DRIVER])   # (nothing to do when it is newer than the plan's sources)
    return DRIVER


_out = {}


def plan(driver, case):
    if case not in _out:
        r = subprocess.run([driver, case], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, check=True)
        assert r.stderr == ""
        _out[case] = r.stdout
    return _out[case]


def test_driver_links_no_hip_runtime(driver):
    libs = subprocess.run(["ldd", driver], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "amdhip" not in libs and "hsa" not in libs


@pytest.mark.parametrize("case", CASES)
def test_plan_is_what_the_run_computed(driver, case):
    got = [ln for ln in plan(driver, case).splitlines() if not ln.startswith("+ ")]
    want = expected(case).splitlines()
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"case {case}, line {i + 1}"
    assert len(got) == len(want)


def fields(line):
    """'launch variant 0 grid 3 ...' -> {'launch': 'variant', ...} is no use: the first word names the line, the rest are (name, value) pairs"""
    t = line.split()
    if len(t) % 2:
        t = t[1:]
    return dict(zip(t[0::2], t[1::2]))


def rounds_of(text):
    """per round: its launches [(fields, [sets])], the results {set: fields}, the shares {set: fields}, the workspace it grew to, the pool's bytes"""
    out = []
    grew = None
    for ln in text.splitlines():
        if ln.startswith("workspace grows to "):
            grew = int(ln.split()[-1])
        elif ln.startswith("round "):
            out.append({"launches": [], "results": {}, "shares": {}, "grew": grew, "pool": None})
            grew = None
        elif ln.startswith("pool alloc_bytes "):
            out[-1]["pool"] = int(ln.split()[-1])
        elif ln.startswith("launch variant "):
            out[-1]["launches"].append((fields(ln), []))
        elif ln.startswith("order") and out:
            out[-1]["launches"][-1][1].extend(int(x) for x in ln.split()[1:])
        elif ln.startswith("result set "):
            q = fields(ln)
            out[-1]["results"][int(q["set"])] = q
        elif ln.startswith("share set "):
            q = fields(ln)
            out[-1]["shares"][int(q["set"])] = q
    return out


def sets_of(text):
    return {int(fields(ln)["set"]): {k: int(v) for k, v in fields(ln).items()} for ln in text.splitlines() if ln.startswith("set ")}


def first_estimate(s):
    return min(s["sum_len"], s["lmax"] + s["sum_len"] // 8 + 64)


def statuses(text, i):
    return [int(r["results"][i]["status"]) for r in rounds_of(text) if i in r["results"]]


def chunks_of(text, kernel):
    """{row: [first element of every chunk]}"""
    out = {}
    for ln in text.splitlines():
        if ln.startswith("chunk " + kernel + " "):
            out.setdefault(int(ln.split()[3]), []).append(int(ln.split()[5]))
    return out


def rows_of(text, kernel):
    return [{k: int(v) for k, v in fields(" ".join(ln.split()[3:])).items()} for ln in text.splitlines() if ln.startswith("row " + kernel + " ")]


def test_cases_reach_every_branch():
    """what the cases rest on, read off the golden text itself"""
    text = {c: expected(c) for c in CASES}
    # instance edges: a longest sequence + 1 of exactly an instance's columns runs there, one more runs in the next; no set of no bases runs; a lone base does
    for gm in ("lin", "aff", "cvx"):
        t = text["edge_" + gm]
        sets, (rnd,) = sets_of(t), rounds_of(t)
        where = {i: k for k, (q, order) in enumerate(rnd["launches"]) for i in order}
        assert [int(q["block"]) for q, _ in rnd["launches"]] == BLOCK[gm] and [int(q["counter_at"]) for q, _ in rnd["launches"]] == [0, 1, 2, 3]
        for k, cols in enumerate(COLUMNS[gm][:3]):
            at, past = [i for i, s in sets.items() if s["lmax"] + 1 == cols], [i for i, s in sets.items() if s["lmax"] == cols]
            assert len(at) == 1 and len(past) == 1 and where[at[0]] == k and where[past[0]] == k + 1
        assert any(s["lmax"] + 1 == COLUMNS[gm][3] for s in sets.values())
        assert sorted(where) == sorted(i for i, s in sets.items() if s["sum_len"])
        assert any(s["nseq"] == 0 for s in sets.values()) and any(s["nseq"] == 2 and s["sum_len"] == 0 for s in sets.values()) and any(s["sum_len"] == 1 for s in sets.values())
    # the limits
    assert text["long_lin"] == "error hx_test: set 1 holds a sequence of 32768 bases, longer than 32767 (the longest the general POA path takes)\n"
    assert text["long_aff"] == "error hx_test: set 1 holds a sequence of 16384 bases, longer than 16383 (the longest the general POA path takes with affine gaps)\n"
    assert text["long_cvx"] == "error hx_test: set 1 holds a sequence of 8192 bases, longer than 8191 (the longest the general POA path takes with convex gaps)\n"
    assert text["big_set"] == "error hx_test: set 1 holds 2129855 bases in all, more than the 2097150 nodes a graph can have\n"
    # the capped first round: every set with a DP comes back; what they saw lies on both sides of their estimate; one set is let past its worst case
    t = text["cap"]
    sets, rnds = sets_of(t), rounds_of(t)
    dp = [i for i, s in sets.items() if s["nseq"] > 1]
    assert all(int(rnds[0]["results"][i]["status"]) == 1 for i in dp) and sorted(rnds[1]["results"]) == dp and len(dp) < len(sets)
    arm = {2 * int(rnds[0]["results"][i]["vseen"]) + 64 > 2 * first_estimate(sets[i]) for i in dp if first_estimate(sets[i]) < sets[i]["sum_len"]}
    assert arm == {False, True}
    past = [i for i in dp if first_estimate(sets[i]) == sets[i]["sum_len"]]
    assert past and all(statuses(t, i) == [1, 0] for i in past)
    assert any(statuses(t, i) == [1, 1, 0] for i in dp)   # ... and one goes on to the worst case
    assert "out retried 4 " in t
    assert text["cap_fail"].endswith("error hx_test: set 2 failed on the device (status 1)\n") and statuses(text["cap_fail"], 2) == [1, 1]
    # any other status: no rerun, the error carries it
    assert text["status2"].endswith("error hx_test: set 1 failed on the device (status 2)\n") and statuses(text["status2"], 1) == [2]
    assert all(first_estimate(sets_of(text[c])[1]) < sets_of(text[c])[1]["sum_len"] for c in ("status2", "status3_plain"))   # (as an H overflow it would be rerun)
    assert text["status3_plain"].endswith("error hx_test: set 1 failed on the device (status 3)\n") and statuses(text["status3_plain"], 1) == [3]
    # graph calls: back for the alignments and then for the slot, and in the other order; shares in more than one round's pool; the three errors
    assert any(statuses(text["graph_aln"], i) == [3, 1, 0] for i in sets_of(text["graph_aln"]))
    assert any(statuses(text["graph_both"], i) == [1, 3, 0] for i in sets_of(text["graph_both"]))
    assert {r["pool"] for r in rows_of(text["graph_aln"], "graph_gather") if r["kind"] == 3} == {1, 2}
    assert "out retried 1 aln_retried 2 " in text["graph_aln"] and "out retried 2 aln_retried 2 " in text["graph_both"]
    assert text["graph_aln2"].endswith("error hx_test: set 2 failed on the device (its alignments hold 77 pairs, its share of the pool 75)\n")
    assert text["graph_ff"].endswith("error hx_test: set 2 failed on the device (its alignments hold 4294967295 pairs, its share of the pool 1)\n")
    assert text["graph_lie"].endswith("error hx_test: internal error (the alignments of set 5 outgrew their share of the pool)\n")
    # the budget: the slots of an instance bound by it; two instances share the workspace; the error names the set that is too large
    (rnd,) = rounds_of(text["budget"])
    (q0, o0), (q1, o1) = rnd["launches"]
    assert int(q0["grid"]) == 9500000 // int(q0["slot_bytes"]) < len(o0) and int(q1["grid"]) == 9500000 // int(q1["slot_bytes"]) < len(o1)
    need = [int(q["grid"]) * int(q["slot_bytes"]) for q in (q0, q1)]
    assert rnd["grew"] == max(need) < sum(need) and min(need) > 0
    assert text["budget_over"].endswith("error hx_test: set 43 needs 17474816 bytes of workspace, more than the budget of 4000000 (option poa_workspace_gb)\n")
    # the MSA: with and without the consensus row, a set without a column, an empty row with its one chunk; rows of 64 and of 65 elements
    for c, n_cns in (("msa", 3), ("msa_nocns", 0)):
        rows, ch = rows_of(text[c], "msa_rows"), chunks_of(text[c], "msa_rows")
        assert sum(r["kind"] for r in rows) == n_cns                                    # (kind: is_cns)
        assert any(r["len"] == 0 and ch[k] == [0] for k, r in enumerate(rows))
        assert any(r["len"] == 64 and ch[k] == [0] for k, r in enumerate(rows)) and any(r["len"] == 65 and ch[k] == [0, 64] for k, r in enumerate(rows))
        cols = [int(x) for x in next(ln for ln in text[c].splitlines() if ln.startswith("msa_cols")).split()[1:]]
        assert cols.count(0) == 2 and len(cols) == 5
    # coverage: with and without the profile; sequences of one base are not counted
    for c, stride in (("cov", 1), ("cov_prof", 4)):
        assert f"launch cov_hist grid 2 n_chunks 6 stride {stride}\n" in text[c] and f" stride {stride}\n" in text[c].split("launch cov_gather")[1]
        rows = rows_of(text[c], "cov_hist")
        assert len(rows) == 5 and min(r["len"] for r in rows) == 2 and sum(s["nseq"] for s in sets_of(text[c]).values()) == 8
    assert " prof 0 " in text["cov"] and " prof 0 " not in text["cov_prof"]
    # strand calls: the reverse complements, and the weights turned round with them
    assert "\ncodes_rc n 33 " in text["strand"] and "\nwts_rc " not in text["strand"] and "\nwts_rc n 33 " in text["strand_w"]
    assert all(" variant 4 " in ln for c in ("strand", "strand_w") for ln in text[c].splitlines() if ln.startswith("launch variant"))


SCORE_BOUND = 1 << 29   # kernels/poa_modes_plan.h; DESIGN.md section 11, "Score range of the full matrix"
MAX_SET_BASES = (1 << 21) - 2
MAX_LEN = {"lin": 32767, "aff": 16383, "cvx": 8191}


def refusal(set_, bases, columns, mag):
    """the text of describe()'s refusal of a set whose (bases + columns of its instance) x the largest score magnitude reaches 2^29"""
    return (f"error hx_test: set {set_} holds {bases} bases, its instance {columns} columns: with scores of up to {mag} their product {(bases + columns) * mag} "
            f"reaches 2^29 = {SCORE_BOUND} (a set's scores must stay below it)\n")


@pytest.mark.parametrize("gm", ["lin", "aff", "cvx"])
def test_scores_just_under_the_bound_are_accepted_and_at_the_bound_refused(driver, gm):
    # set 1: 1 024 bases in the instance of 1 024 columns; 2 048 x (2^18 - 1) = 2^29 - 2 048, 2 048 x 2^18 = 2^29
    assert COLUMNS[gm][0] == 1024 and (1024 + 1024) * (1 << 18) == SCORE_BOUND
    assert plan(driver, "bound_under_" + gm) == "accepted set 0 sum_len 70 lmax 40 columns 1024\naccepted set 1 sum_len 1024 lmax 600 columns 1024\n"
    assert plan(driver, "bound_at_" + gm) == refusal(1, 1024, 1024, 1 << 18)
    # the columns are those of the instance the set runs in, which computes every one of them: a longest sequence of 1 024 bases takes the second
    cols = COLUMNS[gm][1]
    mag = {4096: 87382, 2048: 1 << 17}[cols]
    assert (2048 + cols) * (mag - 1) < SCORE_BOUND <= (2048 + cols) * mag
    assert plan(driver, "bound_wide_" + gm) == refusal(0, 2048, cols, mag)


@pytest.mark.parametrize("gm", ["lin", "aff", "cvx"])
def test_every_int8_score_is_accepted_on_the_largest_set_with_the_longest_sequence(driver, gm):
    assert plan(driver, "bound_int8_" + gm) == f"accepted set 0 sum_len {MAX_SET_BASES} lmax {MAX_LEN[gm]} columns {MAX_LEN[gm] + 1}\n"
    assert (MAX_SET_BASES + MAX_LEN[gm] + 1) * 128 < SCORE_BOUND


@pytest.mark.parametrize("case", CASES)
def test_plan_invariants(driver, case):
    text = plan(driver, case)
    gm = case[-3:] if case[-3:] in COLUMNS else "lin"
    sets = sets_of(text)
    plus = [ln[2:] for ln in text.splitlines() if ln.startswith("+ ")]
    heads = [fields(ln.split(" todo")[0]) for ln in plus if ln.startswith("round ")]
    rnds = rounds_of(text)
    assert len(heads) == len(rnds) or text.rstrip().splitlines()[-1].startswith("error ")   # (a round whose plan fails prints no head)
    needs, insts, k = [], [], -1
    for ln in plus:
        if ln.startswith("round "):
            k += 1
            needs.append({}); insts.append({})
        elif ln.startswith("need set "):
            q = {a: int(b) for a, b in fields(ln).items()}
            needs[k][q["set"]] = q
        elif ln.startswith("inst "):
            q = {a: int(b) for a, b in fields(ln).items()}
            insts[k][q["inst"]] = q
    for k, rnd in enumerate(rnds):
        todo = [int(x) for x in plus[[i for i, ln in enumerate(plus) if ln.startswith("round ")][k]].split(" todo")[1].split()]
        budget, total = int(heads[k]["budget"]), int(heads[k]["total"])
        # every set of the round once in the order lists, the lists one after the other
        order = [i for _, o in rnd["launches"] for i in o]
        assert sorted(order) == sorted(todo) and len(set(order)) == len(order)
        at = 0
        for q, o in rnd["launches"]:
            assert int(q["order_at"]) == at and int(q["n_items"]) == len(o)
            at += len(o)
        live = sorted(insts[k])
        assert [int(q["counter_at"]) for q, _ in rnd["launches"]] == live
        for (q, o), ki in zip(rnd["launches"], live):
            I = insts[k][ki]
            slot, grid = int(q["slot_bytes"]), int(q["grid"])
            assert slot == I["slot"] and grid == I["nslots"] and int(q["block"]) == BLOCK[gm][ki]
            for i in o:
                n = needs[k][i]
                # the instance is the first that fits
                assert n["inst"] == ki and COLUMNS[gm][ki] >= sets[i]["lmax"] + 1 and (ki == 0 or COLUMNS[gm][ki - 1] < sets[i]["lmax"] + 1)
                # the slot holds the need of every set of its instance; a capped one at least the largest pools
                need = n["pools"] + (n["cells"] * n["cell_bytes"] + 255) // 256 * 256
                assert slot >= n["pools"] and slot % 256 == 0 and (I["capped"] or slot >= need)
            # costliest first, ties in the order they came in
            cost = [(-needs[k][i]["cost"], todo.index(i)) for i in o]
            assert cost == sorted(cost)
            assert grid * slot <= budget and grid == min(len(o), I["resident"], budget // slot) and grid * slot <= total
        assert total == max(int(q["grid"]) * int(q["slot_bytes"]) for q, _ in rnd["launches"])
        # the shares of the round's pool: side by side, none over another, their sum the pool
        if rnd["shares"]:
            sh = sorted((int(q["at"]), int(q["room"])) for q in rnd["shares"].values())
            end = 0
            for a, room in sh:
                assert a == end
                end = a + room
            assert end == int(heads[k]["pool_pairs"]) and rnd["pool"] == max(1, end) * 4 and sorted(rnd["shares"]) == sorted(todo)
    # the chunks cover every row exactly, in steps of 64 (a row without elements: its one chunk)
    for kernel in ("msa_rows", "cov_hist", "cov_gather", "graph_gather"):
        rows, ch = rows_of(text, kernel), chunks_of(text, kernel)
        assert sorted(ch) == list(range(len(rows)))
        for r, row in enumerate(rows):
            assert ch[r] == (list(range(0, row["len"], 64)) or [0])
        launches = [fields(ln) for ln in text.splitlines() if ln.startswith("launch " + kernel + " ")]
        if rows:
            (q,) = launches
            n = sum(len(v) for v in ch.values())
            assert int(q["n_chunks"]) == n and int(q["grid"]) == (n + 3) // 4
