"""The back half (edge coordinates, sub-sequence rule, path extraction and stitching) of the oracle and the host pipeline against a live
run of the compiled reference's whole program (oracle/_ref/ref_back, tests/backlib.py): on the hand-built `back` family of
tests/backcases.py, on the front-case families that keep an edge, on four simulated data sets and on the inputs of the
nanopore_rich_300k_s5 fixture. The consensus strings are the oracle's on both sides: SPOA parity (row a9) is not tested here.

The manifest test shows from the REFERENCE's logs that every branch the `back` family plants was reached in the planted variant."""
import json
import os

import pytest

import backcases as bc
import backlib
import frontcases as fc
import orclib
from haslr_amd import host

SIMS = [("--genome-len", "150000", "--seed", "21", "--variant-per-mb", "30"),
        ("--genome-len", "300000", "--seed", "5", "--model", "nanopore", "--variant-per-mb", "40"),
        ("--genome-len", "200000", "--seed", "8", "--variant-per-mb", "30", "--cov", "14", "--hairpin-frac", "0.1"),
        ("--genome-len", "150000", "--seed", "34", "--cov", "40", "--gap-median", "2500")]
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def against_ref(pre, tmp):
    """ref_back and the oracle-backed pipeline on the inputs pre.*; -> the census of the reference's logs"""
    rd, od = backlib.run_ref(pre, os.path.join(str(tmp), "ref")), os.path.join(str(tmp), "orc")
    ds = host.Dataset(pre + ".contigs.fa", pre + ".reads.fa", pre + ".paf")
    be = orclib.OracleBackend(ds, 4)
    run = host.Run(ds, ds.params(), be.table, od)
    run.all()
    c = backlib.check_against_ref(run, ds, rd, od, pre)
    run.close(); be.close(); ds.close()
    return c


@pytest.fixture(scope="module")
def back(built, tmp_path_factory):
    """the `back` family, and the reference's run on it, made once: (prefix, Case, the reference's output directory)"""
    d = tmp_path_factory.mktemp("back")
    pre, case = bc.build(str(d / "in"))
    return pre, case, backlib.run_ref(pre, str(d / "ref"))


def test_back_family_equals_the_reference(back, tmp_path):
    pre, case, rd = back
    od = str(tmp_path / "orc")
    ds = host.Dataset(pre + ".contigs.fa", pre + ".reads.fa", pre + ".paf")
    be = orclib.OracleBackend(ds, 4)
    run = host.Run(ds, ds.params(), be.table, od)
    run.all()
    backlib.check_against_ref(run, ds, rd, od, pre)
    run.close(); be.close(); ds.close()


def test_back_manifest_fired_in_the_reference(back):
    """every planted branch, counted in the reference's own logs: the count is the planted one"""
    pre, case, rd = back
    man = case.man["back"]
    got = backlib.census(rd)
    for k, v in man["census"].items():
        if not k.startswith("case"):      # (the builder counts the cases of the modelled edges only; they are checked per read below)
            assert got[k] == v, f"{k}: the reference's logs show {got[k]}, planted {v}"
    assert got["supporting_0"] == 4 and got["breaking"] == 4 and got["all_empty_edge"] == 2 and got["hairpin"] == 2 and got["singleton_paths"] == 1
    assert got["could_not_extract"] == 0 and got["wrapped_subseq"] == 0     # argued unreachable in tests/backcases.py
    coord = backlib.parse_coordinate_log(backlib.read_text(rd, "log_coordinate.txt"))
    cns = backlib.parse_consensus_log(backlib.read_text(rd, "log_consensus.txt"))
    assert set(coord) == set(man["edges"]), "the reference handed out other edges, or in another direction, than were planted"
    seen = set()
    for key, e in man["edges"].items():
        rec = coord[key]
        assert rec["n_supp"] == e["n_supp"], key
        for k in ("supporting", "best1", "best2", "contig1_pos", "contig2_pos"):
            if k in e:
                assert rec[k] == e[k], f"{key} {e.get('name', '')}: {k} is {rec[k]} in the reference's log, planted {e[k]}"
        if e["reads"]:
            assert {r["rid"]: (tuple(r["cases"]), r["lr_start"], r["lr_end"]) for r in rec["reads"]} == e["reads"], key
        for rid, (pos, trimmed) in e["what"].items():
            for k in e["reads"][rid][0]:
                seen.add((k, pos, trimmed))
    # the five walk positions for all eight cases, on alignments the front half trimmed and on untrimmed ones
    assert seen == {(k, pos, t) for k in range(1, 9) for pos in bc.WALK_POSITIONS for t in (False, True)}
    # an alignment trimmed on both sides, walked from a trimmed end, in all eight cases
    assert {k for key in man["trimmed_both"] for r in coord[key]["reads"] for k in r["cases"]} == set(range(1, 9))
    asm = backlib.read_text(rd, "log_asmfinal.txt")
    ann = backlib.read_text(rd, "asm.final.ann").split("\n")
    for key, e in man["edges"].items():
        if e.get("supporting") == 0:      # defaulted to the contigs' ends, and the path broken there
            L = {c: case.contigs[c][0] for c in (key[0], key[2])}
            want = (L[key[0]] - 1 if key[1] == 0 else 0, 0 if key[3] == 0 else L[key[2]] - 1)
            assert (cns[key]["head_end"], cns[key]["tail_beg"]) == want and cns[key]["supp"] == [] and cns[key]["cns"] == "", key
            assert "[breaking] contig1_len:%d " % L[key[0]] in asm
            assert any(row.split("\t")[3:6] == ["ctg", "+-"[key[1]], str(key[0])] for row in ann if row), key
    for key, rec in cns.items():          # the all-empty edges: an empty consensus between two stitched contigs
        if rec["supp"] and all((e + 1) & 0xffffffff == s for _, _, s, e, _ in rec["supp"]):
            assert rec["cns"] == "" and any(row.endswith("\tcns\t0\t%d" % len(rec["supp"])) for row in ann), key
    for c in man["cycle"]:                # a cycle of plain links is never extracted: its contigs appear in no record
        assert f"from:{c}:" not in asm and f"to:{c}:" not in asm
    assert any(line.split("\t")[4] == "-" and line.split("\t")[1] == "0" for line in ann if "\tctg\t" in line), "no record starts on a reverse-strand source contig"


@pytest.mark.parametrize("family", ["coords", "combined"])
def test_front_families_equal_the_reference(family, built, tmp_path):
    """the front-case families that keep an edge after cleaning (400 and 384 supports per edge)"""
    pre, case = fc.build(str(tmp_path / "in"), fc.FAMILIES if family == "combined" else [family], seed=7 if family == "combined" else 1)
    c = against_ref(pre, tmp_path)
    assert c["edges"] == 2 and c["stitching"] == 2


@pytest.mark.parametrize("args", SIMS, ids=lambda a: "_".join(a[1:4:2]))
def test_simulated_sets_equal_the_reference(args, sim, tmp_path):
    c = against_ref(sim(*args), tmp_path)
    assert c["edges"] >= 6 and all(c[f"case{k}"] > 0 for k in range(1, 9))


def test_fixture_inputs_equal_the_reference(sim, tmp_path):
    man = json.load(open(os.path.join(GOLD, "nanopore_rich_300k_s5", "manifest.json")))
    c = against_ref(sim(*man["hxsim_args"]), tmp_path)
    assert c["edges"] > 0
