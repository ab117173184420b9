"""The sets of tests/walksets.py, judged by the CPU side alone: the last alignment of every built set does what the set's name says (the
restatement's last_alignment(), kNW, 5 / -4 / -8), the corpus picks have rows with a third or fourth predecessor and rows with more than 4
(the restatement's statistics), and the restatement's consensus of every set is the oracle's. tests/test_poa_walk_tiles_gpu.py runs the
same sets through the kernel's tile walk."""
from concurrent.futures import ThreadPoolExecutor

import pytest

import orclib
import pmrlib
import walksets


@pytest.fixture(scope="module")
def lin(built, tmp_path_factory):
    return pmrlib.ModesRef(str(tmp_path_factory.mktemp("walk_pmr")))


def test_the_sets_are_seeded_and_small():
    assert walksets._build() == walksets.BUILT
    assert sorted({f for f, _, _, _ in walksets.BUILT}) == ["branch", "deletion", "insertion", "row0", "short"]
    assert [len(st[0]) for f, _, st, _ in walksets.BUILT if f == "short"] == list(walksets.SHORT_LENGTHS)
    assert all(3 <= len(st) <= 5 and all(q and set(q) <= set("ACGT") for q in st) for _, _, st, _ in walksets.BUILT)


@pytest.mark.parametrize("family", ["short", "deletion", "insertion", "branch", "row0"])
def test_the_last_alignment_does_what_the_set_is_for(lin, family):
    sets = [b for b in walksets.BUILT if b[0] == family]
    assert sets
    for _, name, st, premise in sets:
        cns = lin.consensus(st, "nw")
        aln = lin.last_alignment()
        assert walksets.premise_holds(premise, aln), (family, name, premise, aln[:8], len(aln))
        assert cns == orclib.poa_consensus(st), (family, name)


def test_corpus_picks_have_later_predecessors_and_wide_rows(lin):
    with ThreadPoolExecutor(16) as ex:   # (the restatement releases the GIL: ctypes; its statistics are per calling thread)
        res = list(ex.map(lambda c: lin.consensus_stats(c[2], "nw"), walksets.CANDIDATES))
    later, wide = walksets.corpus_picks([r[2] for r in res])
    print("later predecessors:", [(f, k) for f, k, _ in later], "wide rows:", [(f, k) for f, k, _ in wide])
    assert len(later) >= 2 and len(wide) >= 2          # each kind occurs
    by_key = {(f, k): r for (f, k, _), r in zip(walksets.CANDIDATES, res)}
    for f, k, st in later:
        assert by_key[f, k][2]["max_in_degree"] in (3, 4) and by_key[f, k][2]["wide_rows"] == 0
    for f, k, st in wide:
        assert by_key[f, k][2]["wide_rows"] >= 1 and 5 <= by_key[f, k][2]["max_in_degree"] <= 16
    for f, k, st in later + wide:
        assert by_key[f, k][0] == orclib.poa_consensus(st), (f, k)
