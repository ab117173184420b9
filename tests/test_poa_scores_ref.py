"""The CPU side of tests/test_poa_scores_gpu.py (tests/scorelib.py): for every score triple the oracle and the linear restatement give
the same kNW consensus on that triple's sets, the sets tell the triple from 5 / -4 / -8 (a kernel that ignored a score would fail on
them), and the triple is listed in the group that the planner's gate puts it in."""
import pytest

import pmrlib
import scorelib
from scorelib import DEFAULT, EXTREME, TRIPLES, UNUSUAL, USUAL, corpus_of


@pytest.fixture(scope="module")
def refs(built, tmp_path_factory):
    return scorelib.References(pmrlib.ModesRef(str(tmp_path_factory.mktemp("scores_pmr"))))


def test_the_lists():
    assert len(set(TRIPLES)) == len(TRIPLES) == 13 and DEFAULT not in TRIPLES
    assert all(-128 <= v <= 127 for t in TRIPLES for v in t)
    assert scorelib.NEGATIVE in USUAL and max(scorelib.NEGATIVE) <= 0
    lens = sorted(max(len(q) for q in st) for st in scorelib.LONG_SETS)
    assert lens[0] < 128 and lens[-1] > 2 * 2047 and sum(1 for n in lens if n > 2047) >= 3   # (wave_max 2 047: the multi-wave classes unforced)
    assert {f for f, _, _ in corpus_of(TRIPLES[1])} == set(scorelib.poasets.FAMILIES) | {"long"}


@pytest.mark.parametrize("triple", TRIPLES, ids=str)
def test_gate_grouping(triple):
    """the group a triple is listed in is the one the four inequalities of the planner's gate give it"""
    assert scorelib.gate_keeps_pruning(*triple) == (triple in USUAL + EXTREME)
    assert (not scorelib.gate_keeps_pruning(*triple)) == (triple in UNUSUAL)
    assert scorelib.group_of(triple) in scorelib.GROUPS and sum(triple in g for g in scorelib.GROUPS.values()) == 1


def test_gate_of_the_default():
    assert scorelib.gate_keeps_pruning(*DEFAULT)


@pytest.mark.parametrize("triple", [DEFAULT] + TRIPLES, ids=str)
def test_oracle_and_restatement_agree(refs, triple):
    corpus = corpus_of(triple)
    refs.agree(triple, corpus)
    cns, cells = refs.want(triple, corpus)
    assert len(cns) == len(corpus) and cells > 0


@pytest.mark.parametrize("triple", TRIPLES, ids=str)
def test_sets_tell_the_triple_from_the_default(refs, triple):
    """a condition on the inputs: at least a quarter of the sets have another consensus than under 5 / -4 / -8"""
    corpus = corpus_of(triple)
    other = scorelib.failing(corpus, refs.want(triple, corpus)[0], refs.want(DEFAULT, corpus)[0])
    print(triple, "sets whose consensus differs from the default triple's:", len(other), "of", len(corpus))
    assert 4 * len(other) >= len(corpus)
