"""The sets of tests/carrysets.py, judged by the CPU side alone: the premise of every set from the restatement (pmrlib: the cell counts give
the graph rows under the last read) and plain arithmetic - the rows of its last alignment, the waves and members that own real columns
under each cluster shape, how often the mailbox of 64 entries wraps - and the restatement's consensus of every set is the oracle's.
tests/test_poa_carry_batches_gpu.py runs the same sets through the kernel."""
from concurrent.futures import ThreadPoolExecutor

import pytest

import carrysets
import orclib
import pmrlib
from carrysets import CARRY_BATCH, CARRY_MIN, MAX_LEN, MIN_LEN, RECORD_BATCH, WAVE_MBOX


@pytest.fixture(scope="module")
def rows(built, tmp_path_factory):
    """{name: graph rows under the set's last read}; on the way the restatement's consensus of every set is compared with the oracle's"""
    lin = pmrlib.ModesRef(str(tmp_path_factory.mktemp("carry_pmr")))
    with ThreadPoolExecutor(16) as ex:   # (the restatement and the oracle release the GIL: ctypes)
        full = list(ex.map(lambda b: lin.consensus_cells(b[2], "nw"), carrysets.BUILT))
        head = list(ex.map(lambda b: lin.consensus_cells(b[2][:-1], "nw"), carrysets.BUILT))
        cns = list(ex.map(lambda b: orclib.poa_consensus(b[2]), carrysets.BUILT))
    assert [n for (_, n, _, _), f, c in zip(carrysets.BUILT, full, cns) if f[0] != c] == []
    return {n: carrysets.rows_of_last_alignment(f[1], h[1], len(st[-1])) for (_, n, st, _), f, h in zip(carrysets.BUILT, full, head)}


def test_the_sets_are_seeded_and_small():
    assert carrysets._build() == carrysets.BUILT
    assert sorted({f for f, _, _, _ in carrysets.BUILT}) == ["first_longest", "sit_out", "small", "wrap"]
    assert len({n for _, n, _, _ in carrysets.BUILT}) == len(carrysets.BUILT)
    assert all(3 <= len(st) <= 6 and all(q and set(q) <= set("ACGT") for q in st) for _, _, st, _ in carrysets.BUILT)
    # the row counts sit around the batch's least and most rows and the record batch, one below, at and one above each
    assert set(carrysets.SMALL_ROWS) >= {CARRY_MIN - 1, CARRY_MIN, CARRY_MIN + 1, CARRY_BATCH - 1, CARRY_BATCH, CARRY_BATCH + 1,
                                         RECORD_BATCH - 1, RECORD_BATCH, RECORD_BATCH + 1, 2 * RECORD_BATCH - 1, 2 * RECORD_BATCH, 2 * RECORD_BATCH + 1, 1}


def test_rows_of_the_last_alignment(rows):
    print(rows)
    for _, name, _, premise in carrysets.BUILT:
        if premise[0] == "rows":
            assert rows[name] == premise[1], name
        elif premise[0] == "rows_between":
            assert premise[1] <= rows[name] <= premise[2], (name, rows[name])
    assert sorted(rows[n] for f, n, _, _ in carrysets.BUILT if f == "small") == sorted(carrysets.SMALL_ROWS)


def test_mailbox_wraps(rows):
    wraps = {n: carrysets.mailbox_wraps(rows[n]) for f, n, _, _ in carrysets.BUILT if f == "wrap"}
    print(wraps)
    assert len(wraps) == 2 and min(wraps.values()) >= 10 and max(wraps.values()) >= 20
    # every other family's last graph is past one wrap too, except the small ones that are meant to stay below it
    assert all(carrysets.mailbox_wraps(rows[n]) >= 10 for f, n, _, _ in carrysets.BUILT if f in ("sit_out", "first_longest"))
    assert [n for f, n, _, _ in carrysets.BUILT if f == "small" and carrysets.mailbox_wraps(rows[n]) > 2] == []


@pytest.mark.parametrize("shape", sorted(carrysets.CLUSTER_SHAPES))
def test_waves_and_members_with_real_columns(shape):
    per_wave, per_member, most = carrysets.CLUSTER_SHAPES[shape]
    for family, name, st, _ in carrysets.BUILT:
        waves, members = carrysets.pipeline_of(len(st[-1]), shape)
        assert MIN_LEN <= len(st[-1]) <= MAX_LEN, name
        assert 2 <= members <= most and waves >= 2, (shape, name, waves, members)
        assert waves >= members and waves * per_wave >= len(st[-1]) + 1 > (waves - 1) * per_wave
        # the pipeline is sized by the set's longest read and holds it
        assert -(-(max(len(q) for q in st) + 1) // per_member) <= most, (shape, name)


def test_waves_sit_a_short_read_out_and_the_first_read_is_the_longest():
    (_, _, st, _), = [b for b in carrysets.BUILT if b[0] == "sit_out"]
    lengths = [len(q) for q in st]
    assert [n >= 900 for n in lengths] == [True, False, True, False, True] and all(n <= 128 for n in lengths[1::2])
    for shape in carrysets.CLUSTER_SHAPES:   # the short reads leave every wave but the first without a real column, the long ones bring them back
        assert all(carrysets.pipeline_of(n, shape)[0] == 1 for n in lengths[1::2]) and all(carrysets.pipeline_of(n, shape)[1] >= 2 for n in lengths[0::2])
    (_, _, st, _), = [b for b in carrysets.BUILT if b[0] == "first_longest"]
    assert len(st[0]) == MAX_LEN == max(len(q) for q in st) and all(len(q) < len(st[0]) - 100 for q in st[1:])
