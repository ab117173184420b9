"""The chain, edge-support and coordinate operators of haslr_amd/csrc/hx_api.hip behind a fake runtime, without a GPU. tests/hx_api_trace_driver.cpp
calls the public C-ABI on small synthetic data sets; tests/hx_api_fake_runtime.cpp stands where the HIP runtime and the kernels' launchers stand (no HIP
runtime in the link), records every allocation, copy, launch and synchronisation and fills every output column with a pattern that names the column. The
golden text under tests/golden/hx_api_trace/ is not the output of the code under test: it was printed by the hx_api.hip and hx_internal.h of the commit
before the columns were listed once (haslr_amd/csrc/hx_columns.h), compiled unchanged with this driver and this fake ("The front half's columns
are listed once"). The failure cases have no such text - that code could not fail there: they are asserted on."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, ".."))
CSRC = os.path.join(ROOT, "haslr_amd", "csrc")
DRIVER = os.path.join(ROOT, "haslr_amd", "bin", "hx_api_trace_driver")
GOLDEN = os.path.join(HERE, "golden", "hx_api_trace")

# a: eight reads of a few hits each; b: the read shard [2, 6); c: the empty shard [3, 3); d: one hit per read, so no pair, no record and no edge;
# e: a with no edge selected; f: a with the two hairpin edges (their capacity doubles) and one other selected; g: one context, eleven reads and then the
# eight of a (the buffers are reused); h: records emitted and exported by one context, imported by a second
CASES = ["a", "b", "c", "d", "e", "f", "g", "h"]
# the K-th synchronous copy of an operator, counted from its start: chain 1 is the error word, 2-15 the download; edges 1-2 the edge arrays, 3-24 the
# records; coords 1-4 the supports, 5-6 the two per-edge columns
FAILURES = [("chain", 2), ("chain", 9), ("chain", 15), ("edges", 1), ("edges", 3), ("edges", 12), ("edges", 24), ("coords", 1), ("coords", 3), ("coords", 5), ("coords", 6)]
OPERATOR = {"chain": "hx_chain_reads", "edges": "hx_edge_support", "coords": "hx_edge_coords"}


def expected(case):
    with open(os.path.join(GOLDEN, case + ".txt")) as f:
        return f.read()


@pytest.fixture(scope="module")
def driver():
    subprocess.check_call(["make", "-s", "-C", CSRC, DRIVER])   # (nothing to do when it is newer than its sources)
    return DRIVER


def run(driver, *args):
    r = subprocess.run([driver, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, check=True)
    assert r.stderr == ""
    return r.stdout


def test_driver_links_no_hip_runtime(driver):
    libs = subprocess.run(["ldd", driver], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "amdhip" not in libs and "hsa" not in libs


@pytest.mark.parametrize("case", CASES)
def test_trace_and_results_are_what_the_operators_did(driver, case):
    got = run(driver, case).splitlines()
    want = expected(case).splitlines()
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"case {case}, line {i + 1}"
    assert len(got) == len(want)


def sections(text):
    """[(title, lines)] of a driver's output: a line that begins with '== ' opens a section"""
    out = []
    for ln in text.splitlines():
        if ln.startswith("== "):
            out.append((ln[3:], []))
        else:
            out[-1][1].append(ln)
    return out


def test_cases_reach_what_they_are_for():
    """read off the golden text itself"""
    text = {c: expected(c) for c in CASES}
    res = {c: [ln for ln in text[c].splitlines() if ln.startswith("r ")] for c in CASES}
    assert "r chain n_aln 15 n_reads 8 n_cmp 15" in res["a"] and "r chain n_aln 9 n_reads 4 n_cmp 9" in res["b"]
    assert "r chain n_aln 0 n_reads 0 n_cmp 0" in res["c"] and "r edges n_rec 0 n_edge 0" in res["c"] and "r coords n_edge 0 supports 0" in res["c"]
    assert "r chain n_aln 4 n_reads 4 n_cmp 4" in res["d"] and "r edges n_rec 0 n_edge 0" in res["d"]
    assert "r   hit non-null, empty" in res["c"] and "r   key non-null, empty" in res["d"] and "r   supp_lr non-null, empty" in res["e"]   # empty results keep their pointers
    assert not any(" null" in ln for c in CASES for ln in res[c])
    assert "r edges n_rec 14 n_edge 10" in res["e"] and "r coords n_edge 0 supports 0" in res["e"]
    # f: an edge of one record and two hairpins of two, in a scratch of 1 + 4 + 4 records (the byte column shows it)
    assert "r coords n_edge 3 supports 6" in res["f"] and "t   alloc 9" in text["f"].splitlines()
    # g: the second pass allocates nothing
    first, second = (part.split("== hx_ctx_destroy")[0] for part in text["g"].split("== hx_upload")[1:])
    assert "t   alloc " in first and "t   alloc " not in second and "t   free " not in second
    assert "r chain n_aln 21 n_reads 11 n_cmp 21" in res["g"] and "r chain n_aln 15 n_reads 8 n_cmp 15" in res["g"]
    assert "r emitted 14 records of 44 bytes" in res["h"] and any(ln.startswith("t edge_unpack") for ln in text["h"].splitlines())


@pytest.mark.parametrize("which,k", FAILURES)
def test_a_failed_download_is_reported_and_leaves_nothing_behind(driver, which, k):
    name = OPERATOR[which]
    sec = sections(run(driver, "fail", which, str(k)))
    at = [i for i, (title, _) in enumerate(sec) if title == f"{name}, copy {k} fails"]
    assert len(at) == 1
    failed, again = sec[at[0]], sec[at[0] + 1]
    assert any(ln.endswith(" FAILS") for ln in failed[1])                       # the copy that failed is one of the operator's own
    verdict = [ln for ln in failed[1] if ln.startswith("r ")]
    assert verdict == [f"r failed ret -1 out_all_zero 1 error: {verdict[0].split('error: ')[1]}"] and verdict[0].split("error: ")[1].startswith(name + ":")
    # the same call again, on the same context: the results of case a, and of every operator after it
    assert again[0] == name
    good = {title: [ln for ln in lines if ln.startswith("r ")] for title, lines in sections(expected("a"))}
    for title, lines in sec[at[0] + 1:]:
        if title in good and title.startswith("hx_") and title != "hx_ctx_create":
            assert [ln for ln in lines if ln.startswith("r ")] == good[title], title
    assert [title for title, _ in sec[at[0] + 1:]] == [title for title, _ in sections(expected("a"))][at[0]:]
