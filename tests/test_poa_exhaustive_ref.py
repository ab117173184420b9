"""The end scores of the general POA path's CPU restatements (tests/poa_graph_ref.cpp, tests/poa_strand_ref.cpp) held to an exhaustive
optimum, without a GPU: the score of a sequence against the graph it was aligned to is the maximum, over the graph's source-to-sink paths,
of a plain pairwise DP against the path's letters (tests/exhlib.py, tests/pairwise_ref.cpp). That reference loops over no predecessors
and knows no sinks, so it does not share a misreading of the recurrences with the restatements, as the kernels do: F or O taken from one
predecessor only, a global alignment that ends outside a sink, an overlap that forgets the sinks' rows all lower or raise a score here.
The inputs (tests/exhsets.py) branch: no add is over the cap of 2 048 paths, and more than half of the compared alignments face more than
one path, which the tests assert. Beside the scores: the pairwise DP is pinned to the recurrences in Python integers, the alignments
start and end where their type allows (grflib.ends), and every fan-in set reaches 7 predecessors."""
import time

import pytest

import exhlib
import exhsets as xs
import grflib
import strlib
from test_poa_convex_ref import gotoh2, short_pairs

PAIRS = short_pairs(137, 300)[::10]   # (every type and score set runs them all through the Python DP)


@pytest.fixture(scope="module")
def refs(built, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("exh_ref"))
    return exhlib.Reference(grflib.GraphRef(d), strlib.StrandRef(d), exhlib.Pairwise(d))


def differing(inputs, recs, optima, score_of):
    """(family, index, sequence, recorded, optimum) wherever a compared score is not the optimum or an excluded one not zero"""
    out = []
    for (f, n, st), rec, per in zip(inputs, recs, optima):
        for k, o in enumerate(per):
            got = score_of(rec, k)
            want = (0, 0) if o is None and isinstance(got, tuple) else 0 if o is None else o[0]
            if got != want:
                out.append((f, n, k, got, want))
    return out


@pytest.mark.parametrize("mode", xs.MODES)
def test_the_pairwise_dp_is_the_recurrences_in_python_integers(refs, mode):
    assert len(PAIRS) == 30
    for scores in xs.SCORES:
        six = exhlib.gap_scores(scores)
        assert [k for k, (a, b) in enumerate(PAIRS) if refs.pw.score(a, b, mode, six) != gotoh2(a, b, mode, *six)] == [], (mode, scores)
    # a set of paths scores as its best member
    a, b = PAIRS[0]
    six = exhlib.gap_scores(grflib.CONVEX)
    assert refs.pw.best([p[0] for p in PAIRS], b, mode, six) == max(gotoh2(p[0], b, mode, *six) for p in PAIRS)


def test_paths_are_listed_and_counted_on_a_hand_graph(refs):
    # ACGT, AGT (C deleted), ACTT (G -> T): nodes 0 A, 1 C, 2 G, 3 T, 4 T beside G; edges 0-1 1-2 2-3 0-2 1-4 4-3
    rec = refs.ref.graph(["ACGT", "AGT", "ACTT", "ACGT"])
    g = exhlib.graph_before(rec, 3)
    assert exhlib.count_paths(g) == 3 and exhlib.path_strings(g) == ["ACGT", "ACTT", "AGT"] and exhlib.fan_in(g) == 2
    assert exhlib.count_paths(exhlib.graph_before(rec, 1)) == 1 and exhlib.path_strings(exhlib.graph_before(rec, 2)) == ["ACGT", "AGT"]
    rows = grflib.rows_of(rec, ["ACGT", "AGT", "ACTT", "ACGT"])
    assert exhlib.path_strings(exhlib.graph_from_rows(rows, 3)) == ["ACGT", "ACTT", "AGT"]
    # two sources and two sinks (local: only ACG is joined, the flanks GG and TT of the second member become chains of their own)
    rec = refs.ref.graph(["TTACGCC", "GGACGTT", "ACG"], "sw")
    assert exhlib.path_strings(exhlib.graph_before(rec, 2)) == ["GGACGCC", "GGACGTT", "TTACGCC", "TTACGTT"]
    # global, 5 / -4 / -8: ACG against any of the four is three matches between two gaps of two nodes, 15 - 16 - 16
    assert exhlib.optimum(refs.pw, exhlib.graph_before(rec, 2), "ACG", "nw", grflib.LINEAR) == (-17, 4)
    assert exhlib.optimum(refs.pw, exhlib.graph_before(rec, 2), "ACG", "sw", grflib.LINEAR) == (15, 4)
    assert exhlib.optimum(refs.pw, exhlib.graph_before(rec, 2), "ACG", "nw", grflib.LINEAR, cap=3) == (None, 4)   # over the cap: reported, not scored


def test_the_fan_in_sets_reach_seven_predecessors(refs):
    for mode in xs.MODES:
        for scores in (grflib.LINEAR, grflib.AFFINE, grflib.CONVEX):
            fans = [exhlib.fan_in(exhlib.graph_before(refs.ref.graph(st, mode, scores), len(st))) for st in xs.FAN_IN]
            print(f"{mode} {scores}: the largest fan-in of the fan-in sets: {fans}")
            assert min(fans) >= 7, (mode, scores, fans)


@pytest.mark.parametrize("mode", xs.MODES)
def test_every_recorded_score_is_the_optimum_over_the_paths(refs, mode):
    t0, total, total_branched = time.time(), 0, 0
    for scores in xs.SCORES:
        recs, optima = refs.graph(xs.INPUTS + xs.EXCLUDED, mode, scores)
        n, branched, most, over = exhlib.tally_graph(optima)
        print(f"{mode} {scores}: {n} alignments compared, {branched} faced more than one path, at most {most} paths, {len(over)} over the cap")
        assert over == [], (mode, scores)   # the cap is an assertion: no add is left out
        assert differing(xs.INPUTS + xs.EXCLUDED, recs, optima, lambda rec, k: rec.sequences[k].score) == [], (mode, scores)
        total, total_branched = total + n, total_branched + branched
    print(f"{mode}: {total} alignments compared, {total_branched} branched, {time.time() - t0:.1f} s")
    # (without a positive score an overlap joins a pair at a corner and the graph becomes one long chain: that score set alone stays below half)
    assert total >= 12000 and 2 * total_branched >= total, (mode, total, total_branched)


def test_the_long_gap_sets_make_the_second_piece_win_across_a_bubble(refs):
    """the premise of LONG_GAPS under (5, -4, -8, -6, -24, -1): on at least 8 alignments per type (one per set) the optimum is above the
    optimum under the first piece alone, and at least 8 recorded alignments hold a run of 5 or more nodes without a position that
    passes a node with several predecessors"""
    scores = (5, -4, -8, -6, -24, -1)
    inputs = [c for c in xs.INPUTS if c[0] == "long_gaps"]
    for mode in xs.MODES:
        wins = runs = 0
        for (_, _, st), rec in zip(inputs, refs.graph(inputs, mode, scores)[0]):
            for k in exhlib.compared(st):
                g = exhlib.graph_before(rec, k)
                several = {t for t in g.letter if sum(1 for ss in g.succ.values() if t in ss) > 1}
                wins += exhlib.optimum(refs.pw, g, st[k], mode, scores)[0] > exhlib.optimum(refs.pw, g, st[k], mode, (5, -4, -8, -6, -8, -6))[0]
                aln, i, hit = rec.sequences[k].alignment, 0, False
                while i < len(aln):
                    j = i
                    while j < len(aln) and aln[j][1] == -1:
                        j += 1
                    hit = hit or (j - i >= 5 and any(nd in several for nd, _ in aln[i:j]))
                    i = max(j, i + 1)
                runs += hit
        print(f"{mode}: the second piece raises the optimum of {wins} alignments, {runs} hold a long vertical gap through a node with several predecessors")
        assert wins >= 8 and runs >= 8, (mode, wins, runs)


@pytest.mark.parametrize("lanes,model,lmax,mode,st", xs.WIDTHS, ids=[f"{w[0]}-{w[1]}-{w[2]}-{w[3]}" for w in xs.WIDTHS])
def test_one_set_per_workgroup_width(refs, lanes, model, lmax, mode, st):
    scores = {"linear": grflib.LINEAR, "affine": grflib.AFFINE, "convex": grflib.CONVEX}[model]
    inputs = [("width", lanes, st)]
    recs, optima = refs.graph(inputs, mode, scores)
    n, branched, most, over = exhlib.tally_graph(optima)
    print(f"{lanes} lanes, {lmax} bases: {n} alignments, at most {most} paths")
    assert over == [] and n == 2 and branched >= 1 and most <= 27
    assert differing(inputs, recs, optima, lambda rec, k: rec.sequences[k].score) == []


@pytest.mark.parametrize("mode", xs.MODES)
def test_both_orientation_scores_are_optima_over_the_paths_of_the_rows(refs, mode):
    total = total_branched = 0
    for scores in xs.SCORES:
        recs, optima = refs.strand(xs.STRAND_INPUTS, xs.rc, mode, scores)
        n, branched, most, over = exhlib.tally_strand(optima)
        print(f"{mode} {scores}: {n} sequences in two orientations, {branched} faced more than one path, at most {most} paths, {len(over)} over the cap")
        assert over == [], (mode, scores)
        assert differing(xs.STRAND_INPUTS, recs, optima, lambda rec, k: rec.scores[k]) == [], (mode, scores)
        # the rule itself, and that both branches run
        assert all(rec.reversed[k] == (f < r) for rec in recs for k, (f, r) in enumerate(rec.scores))
        if max(scores) > 0:   # (without a positive score the two orientations mostly tie at nothing)
            assert 4 * sum(f for rec in recs for f in rec.reversed) >= n, (mode, scores)
        total, total_branched = total + n, total_branched + branched
    assert total >= 8000 and 2 * total_branched >= total, (mode, total, total_branched)


def test_every_corpus_set_on_the_list_stays_under_the_cap(refs):
    """every set of CORPUS_UNDER_CAP, those left out for their cost included, stays under the cap under every type and score set
    (counted, not enumerated). That the list leaves out no other set of poasets.CORPUS was counted once over the whole corpus: ten
    minutes, too long for a test."""
    named = [c for c in xs.poasets.CORPUS if (c[0], c[1]) in set(xs.CORPUS_UNDER_CAP)]
    assert len(named) == len(xs.CORPUS_UNDER_CAP) == 113 and len(xs.CORPUS) == 105
    # (the 105 that are compared: test_every_recorded_score_is_the_optimum_over_the_paths asserts it under every type and score set. Here the
    # eight left out for their cost, under kNW and the affine defaults)
    slow = [c for c in named if (c[0], c[1]) in xs.CORPUS_TOO_SLOW]
    combos = [("nw", grflib.AFFINE)]
    counts = refs._pmap(lambda c: max(exhlib.count_paths(exhlib.graph_before(refs.ref.graph(c[2], mode, scores), q)) for mode, scores in combos for q in exhlib.compared(c[2])), slow)
    print(f"{len(named)} of the {len(xs.poasets.CORPUS)} sets of poasets.CORPUS stay under {exhlib.CAP} paths per add, {len(slow)} of them left out for their cost (paths: {counts})")
    assert len(slow) == 8 and [(c[0], c[1], n) for c, n in zip(slow, counts) if n > exhlib.CAP] == []


@pytest.mark.parametrize("mode", xs.MODES)
def test_alignments_start_and_end_where_their_type_allows(refs, mode):
    for scores in xs.SCORES:
        recs, _ = refs.graph(xs.INPUTS + xs.EXCLUDED, mode, scores)
        bad = [(f, k, why) for (f, k, st), rec in zip(xs.INPUTS + xs.EXCLUDED, recs) for why in grflib.ends(rec, st, mode) + grflib.rescore(rec, st, scores, mode)]
        assert bad[:5] == [], (mode, scores)


def test_the_ends_check_refuses_what_the_rules_forbid(refs):
    st = ["ACGTACGT", "ACGTACGT"]
    rec = refs.ref.graph(st, "nw")
    assert grflib.ends(rec, st, "nw") == []
    cut = rec._replace(sequences=[rec.sequences[0], rec.sequences[1]._replace(alignment=rec.sequences[1].alignment[1:-1])])
    assert len(grflib.ends(cut, st, "nw")) == 2   # (starts at node 1, no source; ends at node 6, no sink)
    assert len(grflib.ends(cut, st, "ov")) == 2 and grflib.ends(cut, st, "sw") == []
    # an overlap that ends inside the chain is fine where it holds the last position, one that starts inside where it holds position 0
    ov = refs.ref.graph(["ACGTACGGTCA", "CGGTCATTGAC", "TTACGTAC"], "ov")
    assert grflib.ends(ov, ["ACGTACGGTCA", "CGGTCATTGAC", "TTACGTAC"], "ov") == []
    # the hand case: "C" against the node A under a dear mismatch, one vertical move and no position; node 0 is source and sink
    rec = refs.ref.graph(["A", "C"], "ov", (5, -20, -8, -8, -8, -8))
    assert rec.sequences[1].alignment == [(0, -1)] and grflib.ends(rec, ["A", "C"], "ov") == []
