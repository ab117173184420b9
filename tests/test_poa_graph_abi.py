"""The C-ABI, Python and header side of the graph and alignment output, without a GPU: the ctypes mirror of hx_graph_out has the C sizes and
offsets, the two entry points are exported and the option that caps the alignment pool is registered, a caller compiled against
include/spoa_hx.hpp that asks a graph for print_dot fails loudly without a device while a graph without sequences needs none, and the GFA
and DOT writers, fed the CPU restatement's record of the hand-derived cases, write text that parses back to that graph."""
import ctypes as C
import os
import subprocess

import pytest

import grflib
from haslr_amd import ctypes_defs as T
from haslr_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT_FIELDS = ["n_set", "n_seq", "node_off", "node_base", "node_rank", "node_col", "edge_off", "edge_from", "edge_to", "edge_w", "base_node", "cns_off", "cns", "cns_node",
              "aln_off", "aln_node", "aln_pos", "aln_score", "dp_cells", "seq_bases", "n_aligned", "gather_kernel_ms", "gather_kernel_bytes", "slot_reruns", "aln_reruns"]
KNOWN = [(["ACGT", "AGT"], "nw"), (["ACGT", "ACAGT"], "nw"), (["ACGT", "ACCT"], "nw"), (["ACGTACGGTCA", "CGGTCATTGAC"], "ov"), (["TTACGTAA", "GGACGTCC"], "sw"),
         (["ACGT", "", "ACCT", "AGCT", "G"], "nw")]


@pytest.fixture(scope="module")
def graph_caller(built, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("spoa_graph") / "spoa_graph_caller")
    lib = os.path.join(ROOT, "haslr_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "spoa_graph_caller.cpp"), "-o", exe,
                           "-L", lib, "-lhaslr_hip", "-pthread", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


@pytest.fixture(scope="module")
def ref(built, tmp_path_factory):
    return grflib.GraphRef(str(tmp_path_factory.mktemp("grf_abi")))


def test_struct_sizes_and_offsets_match_c(built, tmp_path):
    src = tmp_path / "sz.c"
    items = ["sizeof(hx_graph_out)"] + [f"offsetof(hx_graph_out,{f})" for f in OUT_FIELDS] + ["sizeof(hx_poa_convex_params)", "sizeof(hx_msa_out)", "sizeof(hx_wcns_out)"]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "haslr_types.h"\nint main(){' +
                   "".join(f'printf("%zu\\n",(size_t){it});' for it in items) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    want = [C.sizeof(T.GraphOut)] + [getattr(T.GraphOut, f).offset for f in OUT_FIELDS] + [C.sizeof(T.PoaConvexParams), C.sizeof(T.MsaOut), C.sizeof(T.WcnsOut)]
    assert got == want
    assert [n for n, _ in T.GraphOut._fields_] == OUT_FIELDS and got[0] == 192
    assert got[-3:] == [28, 96, 80]   # the structs beside it are as they were


def test_entry_points_and_the_option_are_there(built):
    assert hasattr(hip.lib(), "hx_poa_graph") and hasattr(hip.lib(), "hx_free_graph")
    assert "hx_poa_graph" in hip.SYMBOLS and "hx_free_graph" in hip.SYMBOLS
    assert "poa_graph_aln_cap" in hip.option_names() and "poa_modes_slot_kb" in hip.option_names()


def test_print_dot_without_a_device_fails_loudly(graph_caller, tmp_path):
    import torch
    for args in ([], ["--batch"], ["--threads", "4"]):
        for head in ("nw", "sw 5 -4 -8 -6", "ov 5 -4 -8 -6 -10 -4"):
            r = subprocess.run([graph_caller, "--out", str(tmp_path)] + args, input=f"{head}\nACGTACGT\nACGTTCGT\n", capture_output=True, text=True)
            if torch.cuda.is_available():   # (a device is present: the same call works; tests/test_poa_graph_gpu.py checks what it writes)
                assert r.returncode == 0 and r.stdout.endswith("=\n"), (args, head, r.returncode, r.stderr)
            else:
                assert r.returncode == 1 and "no HIP device" in r.stderr and r.stdout == "", (args, head, r.returncode, r.stderr)


def test_a_graph_without_sequences_needs_no_device(graph_caller, tmp_path):
    r = subprocess.run([graph_caller, "--out", str(tmp_path)], input="nw\n-\n", capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "=\n", (r.returncode, r.stderr)
    assert (tmp_path / "0.dot").read_text() == "digraph 0 {\n    graph [rankdir = LR]\n}\n"
    assert (tmp_path / "0.gfa").read_text() == "H\tVN:Z:1.0\n"


@pytest.mark.parametrize("case", range(len(KNOWN)))
def test_the_writers_on_the_known_answers(ref, case):
    seqs, mode = KNOWN[case]
    rec = ref.graph(seqs, mode)
    gfa, dot = hip.graph_to_gfa(rec), hip.graph_to_dot(rec)
    assert grflib.parse_gfa(gfa) == grflib.gfa_of(rec)
    assert grflib.parse_dot(dot) == grflib.dot_of(rec)
    names = [f"read/{k}" for k in range(len(seqs))]
    assert grflib.parse_gfa(hip.graph_to_gfa(rec, names)) == grflib.gfa_of(rec, names)


def test_the_text_of_the_first_known_answer(ref):
    rec = ref.graph(["ACGT", "AGT"])
    assert hip.graph_to_gfa(rec) == ("H\tVN:Z:1.0\nS\t1\tA\trk:i:0\tcl:i:0\nS\t2\tC\trk:i:1\tcl:i:1\nS\t3\tG\trk:i:2\tcl:i:2\nS\t4\tT\trk:i:3\tcl:i:3\n"
                                     "L\t1\t+\t2\t+\t0M\tew:i:2\nL\t2\t+\t3\t+\t0M\tew:i:2\nL\t3\t+\t4\t+\t0M\tew:i:4\nL\t1\t+\t3\t+\t0M\tew:i:2\n"
                                     "P\ts0\t1+,2+,3+,4+\t0M,0M,0M\nP\ts1\t1+,3+,4+\t0M,0M\nP\tconsensus\t1+,2+,3+,4+\t0M,0M,0M\n")
    assert hip.graph_to_dot(rec).split("\n")[:5] == ["digraph 2 {", "    graph [rankdir = LR]", '    0 [label = "0 - A", style = filled, fillcolor = goldenrod1]',
                                                      '    0 -> 1 [label = "2"]', '    0 -> 2 [label = "2"]']
    rec = ref.graph(["ACGT", "ACCT"])
    assert '    2 -> 4 [style = dotted, arrowhead = none]' in hip.graph_to_dot(rec).split("\n")
