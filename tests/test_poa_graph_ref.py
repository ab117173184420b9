"""The CPU restatement of the graph and alignment output (tests/poa_graph_ref.cpp, DESIGN.md "General POA path", "Graph and alignment
output"), without a GPU: on the CPU tests' sets and the structured corpus, in three modes under linear, affine and convex gaps, what it
records satisfies by itself what a partial-order graph with paths and alignments must satisfy (tests/grflib.py: checks, rescore), the
rows rebuilt from paths and columns are the MSA restatement's, replaying the alignments through a fresh graph rebuilds the graph, and the
hand-derived cases of the issue come out as stated."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import cvxlib
import grflib
import msalib
import poasets
import wgtlib
from test_poa_modes_ref import SETS

MODES = ["sw", "nw", "ov"]
MODELS = {"linear": grflib.LINEAR, "affine": grflib.AFFINE, "convex": grflib.CONVEX}


@pytest.fixture(scope="module")
def ref(built, tmp_path_factory):
    return grflib.GraphRef(str(tmp_path_factory.mktemp("grf")))


@pytest.fixture(scope="module")
def msa(built, tmp_path_factory):
    return msalib.MsaRef(str(tmp_path_factory.mktemp("grf_msa")))


@pytest.fixture(scope="module")
def cvx(built, tmp_path_factory):
    return cvxlib.ConvexRef(str(tmp_path_factory.mktemp("grf_cvx")))


def pmap(fn, items, threads=16):
    with ThreadPoolExecutor(threads) as ex:   # (the restatements release the GIL: ctypes)
        return list(ex.map(fn, items))


def want_rows(msa, cvx, st, mode, scores):
    if grflib.model_of(scores) == 2:
        return cvx.msa(st, mode, scores).rows
    return msa.rows(st, mode, scores[0], scores[1], scores[2], scores[3])


def failing(ref, msa, cvx, sets, mode, scores, weights=None):
    """per set that fails: (index, what does not hold)"""
    res = pmap(lambda k: ref.graph_cells(sets[k], mode, scores, None if weights is None else weights[k]), range(len(sets)))
    rows = pmap(lambda st: want_rows(msa, cvx, st, mode, scores), sets)
    out = []
    for k, (st, (rec, _, before)) in enumerate(zip(sets, res)):
        bad = grflib.checks(rec, st, None if weights is None else weights[k]) + grflib.rescore(rec, st, scores, mode, before) + grflib.rescore(rec, st, scores, mode) + grflib.ends(rec, st, mode)
        if grflib.rows_of(rec, st) != rows[k]:
            bad.append("the rows rebuilt from paths and columns are not the MSA restatement's")
        letters, ef, et, ew = ref.replay(st, rec)
        if letters != rec.node_base or not np.array_equal(ef, rec.edge_from) or not np.array_equal(et, rec.edge_to) or (weights is None and not np.array_equal(ew, rec.edge_w)):
            bad.append("replaying the alignments does not rebuild the graph")
        if bad:
            out.append((k, bad[:3]))
    return out


@pytest.mark.parametrize("model", list(MODELS))
@pytest.mark.parametrize("mode", MODES)
def test_the_record_holds_its_invariants_on_the_cpu_sets(ref, msa, cvx, mode, model):
    assert failing(ref, msa, cvx, SETS, mode, MODELS[model]) == []


@pytest.mark.parametrize("model", list(MODELS))
@pytest.mark.parametrize("mode", MODES)
def test_the_record_holds_its_invariants_on_the_structured_corpus(ref, msa, cvx, mode, model):
    sets = [st for _, _, st in poasets.CORPUS]
    bad = failing(ref, msa, cvx, sets, mode, MODELS[model])
    assert [(poasets.CORPUS[k][0], poasets.CORPUS[k][1], why) for k, why in bad] == []


@pytest.mark.parametrize("mode", MODES)
def test_edge_weights_are_the_sums_of_the_given_weights(ref, msa, cvx, mode):
    sets = SETS[:120]
    assert failing(ref, msa, cvx, sets, mode, grflib.AFFINE, wgtlib.quality_weights(sets, 41)) == []
    assert failing(ref, msa, cvx, sets[:60], mode, grflib.CONVEX, wgtlib.uniform_weights(sets[:60], 42)) == []


def test_small_scores_and_a_dear_second_piece(ref, msa, cvx):
    for scores in ((1, -1, -3, -3, -3, -3), (1, -1, -3, -2, -3, -2), (5, -4, -8, -6, -24, -1), (2, -7, -2, -2, -9, 0)):
        for mode in MODES:
            assert failing(ref, msa, cvx, SETS[:80], mode, scores) == [], (scores, mode)


def test_an_alignment_without_a_position_stays_as_the_walk_left_it(ref):
    # overlap, a mismatch dearer than a gap: the only cell of "C" against the node A is reached from above
    rec = ref.graph(["A", "C"], "ov", (5, -20, -8, -8, -8, -8))
    assert rec.sequences[1].alignment == [(0, -1)] and rec.sequences[1].score == -8
    assert rec.node_base == "AC" and len(rec.edge_from) == 0 and [int(c) for c in rec.node_col] == [0, 1]


# ---- the known answers of the issue (global, 5 / -4 / -8), authored by hand
def test_known_answer_a_deleted_base(ref):
    rec = ref.graph(["ACGT", "AGT"])
    assert rec.sequences[0].alignment == [] and rec.sequences[0].score == 0
    assert rec.sequences[1].alignment == [(0, 0), (1, -1), (2, 1), (3, 2)] and rec.sequences[1].score == 7
    assert rec.node_base == "ACGT"
    assert rec.edge_from.tolist() == [0, 1, 2, 0] and rec.edge_to.tolist() == [1, 2, 3, 2] and rec.edge_w.tolist() == [2, 2, 4, 2]
    assert [sq.path.tolist() for sq in rec.sequences] == [[0, 1, 2, 3], [0, 2, 3]]


def test_known_answer_an_inserted_base(ref):
    assert ref.graph(["ACGT", "ACAGT"]).sequences[1].alignment == [(0, 0), (1, 1), (-1, 2), (2, 3), (3, 4)]


def test_known_answer_a_mismatch_opens_an_aligned_node(ref):
    rec = ref.graph(["ACGT", "ACCT"])
    assert rec.sequences[1].alignment == [(0, 0), (1, 1), (2, 2), (3, 3)] and rec.sequences[1].score == 11
    assert rec.node_base == "ACGTC" and rec.node_col[4] == rec.node_col[2]
    assert rec.sequences[1].path.tolist() == [0, 1, 4, 3] and rec.node_rank.tolist() == [0, 1, 2, 4, 3] and rec.n_cols == 4


def test_known_answer_overlap(ref):
    rec = ref.graph(["ACGTACGGTCA", "CGGTCATTGAC"], "ov")
    assert rec.sequences[1].alignment == [(5 + i, i) for i in range(6)]
    assert len(rec.node_base) == 16 and rec.sequences[1].path.tolist() == [5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15]


def test_known_answer_local(ref):
    assert ref.graph(["TTACGTAA", "GGACGTCC"], "sw").sequences[1].alignment == [(2, 2), (3, 3), (4, 4), (5, 5)]


def test_empty_members_and_sets(ref):
    rec = ref.graph(["", "ACGT", "", "ACGA"])
    assert [len(sq.path) for sq in rec.sequences] == [0, 4, 0, 4] and [sq.alignment for sq in rec.sequences[:3]] == [[], [], []]
    assert grflib.checks(rec, ["", "ACGT", "", "ACGA"]) == []
    rec = ref.graph([])
    assert rec.node_base == "" and rec.consensus == "" and rec.n_cols == 0 and rec.sequences == []
    rec = ref.graph(["G"])
    assert rec.node_base == "G" and len(rec.edge_from) == 0 and rec.consensus == "G" and rec.consensus_nodes.tolist() == [0]
