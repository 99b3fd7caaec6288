"""CPU tests of the long-key lookup inputs (tests/long_key_cases.py): the coverage conditions the
GPU parity tests rely on, the Table::get and Table::range models against brute force at these
key lengths, and proof that the cases tell a wrong key compare from a right one: a linear-scan
model of point read and of both seeks, run with the true comparator (it must reproduce the
oracle) and with five wrong ones (each must change at least 50 answers of either kind)."""
import functools

import numpy as np
import pytest

import long_key_cases as K
import pyoracle
from table_get_model import GET_FILTERED, GET_HIT, TableModel
from table_range_model import RANGE_EMPTY, RANGE_NO_BLOCK, RANGE_ROWS, RangeModel, brute_force as range_brute_force
from test_table_get_model import brute_force as get_brute_force


def test_coverage_conditions():
    for name, count in K.coverage().items():
        print(name, "=", count)


def test_u16_block_shape():
    """The hand-built block at the u16 limit: shared lengths 65,534 and 65,535 and a zero-byte
    suffix at restart interval 2, and the oracle reads its own encoding back."""
    buf, off = K.u16_blocks()
    parsed, item_start, status = pyoracle.decode_blocks(buf, off)
    assert (status == 0).all() and list(item_start) == [0, 4, 8]
    assert list(parsed["prefix_len"]) == [0, 0, 0, 0, 0, 65534, 0, 65535]
    assert list(parsed["key_len"]) == [65534, 65535, 65535, 65535, 65534, 1, 65535, 0]
    rows = K.u16_rows()
    for b, ri in ((0, 1), (1, 2)):
        pl = K.payload(buf, off, b)
        n, p = pyoracle.data_block_decode(pl)
        assert pyoracle.materialize(pl, p, ri) == [(k, v, s, t) for k, v, s, t in rows]
        assert [pyoracle.point_read(pl, k, s + 1) for k, _, s, _ in rows] == [0, 1, 2, 3]
        assert pyoracle.point_read(pl, K.huge_needle(K.U16_STEM), K.SNAP_ALL - 1) == -1
        assert pyoracle.seek(pl, K.huge_needle(K.U16_STEM))[:2] == (4, 4)


# ---- the models at these key lengths
@functools.lru_cache(maxsize=None)
def _get_brute_force():
    keys, seqnos = [r[0] for r in K.rows()], [r[2] for r in K.rows()]
    return [get_brute_force(keys, seqnos, k, s) for k, s in K.get_queries()]


@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("two_level", [False, True])
def test_get_model_matches_brute_force(two_level, filtered):
    _, t, _ = K.table(two_level, filtered)
    starts, off = t["starts"], t["block_off"]
    rows = K.rows()
    hits = filtered_out = 0
    for (key, snap), want, (st, ans) in zip(K.get_queries(), _get_brute_force(), K.get_expected(two_level, filtered)):
        outcome, block_off, block_size, item, seqno, _, val_len, vtype = ans
        assert st == 0
        if outcome == GET_FILTERED:  # (the Bloom filter has no false negatives)
            assert filtered and want is None, (key, snap)
            filtered_out += 1
        elif want is None:
            assert outcome != GET_HIT and item == -1, (key, snap, outcome)
        else:
            b = int(np.searchsorted(starts, want, side="right")) - 1
            assert outcome == GET_HIT, (key, snap, outcome)
            assert (block_off, block_size) == (int(off[b]), int(off[b + 1] - off[b])), (key, snap)
            assert int(starts[b]) + item == want, (key, snap)
            assert (seqno, vtype, val_len) == (rows[want][2], rows[want][3], len(rows[want][1])), (key, snap)
            hits += 1
    print("queries / hits / filtered:", len(K.get_queries()), hits, filtered_out)
    assert hits >= 2000 and (filtered_out >= 1000) == filtered, (hits, filtered_out)


@pytest.mark.parametrize("two_level", [False, True])
def test_range_model_matches_brute_force(two_level):
    """The first and the last row of every bound pair against the window of the item list.  The
    window comes from bisection over the sorted keys; brute_force, which visits every key, is
    run on every eighth pair (the crossed and the unbounded ones among them) and must give the
    same window."""
    _, t, _ = K.table(two_level, False)
    keys = [r[0] for r in K.rows()]
    row0 = {int(t["block_off"][b]): int(t["starts"][b]) for b in range(t["block_count"])}
    count = {RANGE_ROWS: 0, RANGE_EMPTY: 0, RANGE_NO_BLOCK: 0}
    for i, (q, (st, ans)) in enumerate(zip(K.range_queries(), K.range_expected(two_level))):
        a, b = K.window(keys, *q)
        if i % 8 == 0:
            assert range_brute_force(keys, *q) == list(range(a, b)), q
        assert st == 0
        count[ans[0]] += 1
        if a < b:
            assert ans[0] == RANGE_ROWS and row0[ans[1]] + ans[3] == a and row0[ans[4]] + ans[6] == b - 1, (q, ans)
        else:
            assert ans[0] in (RANGE_EMPTY, RANGE_NO_BLOCK), (q, ans)
    print("ROWS / EMPTY / NO_BLOCK:", count[RANGE_ROWS], count[RANGE_EMPTY], count[RANGE_NO_BLOCK])
    # (each key as both bounds, inclusive, is a range with rows; its exclusive forms are empty)
    assert count[RANGE_ROWS] >= 2000 and count[RANGE_EMPTY] >= 1000 and count[RANGE_NO_BLOCK] >= 4, count


def test_u16_table_models():
    file, t = K.u16_table()
    assert t["block_count"] == 4
    rows = K.u16_rows()
    model = TableModel(file, t["tli_off"], t["tli_size"], True)
    assert len(model.index_entries(*model.tli)) == 4  # one handle per partition
    keys, seqnos = [r[0] for r in rows], [r[2] for r in rows]
    for key, snap in K.u16_get_queries():
        want = get_brute_force(keys, seqnos, key, snap)
        st, ans = model.lookup(key, snap)
        assert st == 0 and (ans[0] == GET_HIT) == (want is not None), (len(key), snap)
        if want is not None:  # (one row per block)
            assert ans[1] == int(t["block_off"][want]) and ans[3] == 0 and ans[4] == seqnos[want]
    rmodel = RangeModel(file, t["tli_off"], t["tli_size"], True)
    row0 = {int(t["block_off"][b]): b for b in range(4)}
    for q in K.u16_range_queries():
        want = range_brute_force(keys, *q)
        st, ans = rmodel.answer(*q)
        assert st == 0 and (ans[0] == RANGE_ROWS) == bool(want), [x if x is None else len(x) for x in q[:2]]
        if want:
            assert (row0[ans[1]] + ans[3], row0[ans[4]] + ans[6]) == (want[0], want[-1])


# ---- mutants: a wrong key compare changes answers
SIGNED = bytes(i ^ 0x80 for i in range(256))


def _order(a, b):
    return (a > b) - (a < b)


def cmp_true(a, b):
    return _order(a, b)


def cmp_first_window(a, b):
    return _order(a[:16], b[:16])


def cmp_first_window_then_length(a, b):
    return _order(a[:16], b[:16]) or _order(len(a), len(b))


def cmp_signed_bytes(a, b):
    return _order(a.translate(SIGNED), b.translate(SIGNED))


def cmp_no_length_tie_break(a, b):
    n = min(len(a), len(b))
    return _order(a[:n], b[:n])


def cmp_tail_window_dropped(a, b):
    n = min(len(a), len(b)) & ~15
    return _order(a[:n], b[:n]) or _order(len(a), len(b))


MUTANTS = (cmp_first_window, cmp_first_window_then_length, cmp_signed_bytes, cmp_no_length_tie_break,
           cmp_tail_window_dropped)


def model_point_read(block, needle, snap, cmp):
    """block: [(key, seqno)] in block order -> the index of the first item with key == needle
    and seqno < snap, -1 once a key is above the needle or the block ends."""
    for i, (key, seqno) in enumerate(block):
        c = cmp(key, needle)
        if c > 0:
            return -1
        if c == 0 and seqno < snap:
            return i
    return -1


def model_seek(block, lo, hi, lo_excl, hi_excl, cmp):
    """(first, end, lower found, upper found) as pyoracle.seek reports them."""
    n = len(block)
    first, end, found_lo, found_hi = 0, n, False, False
    if lo is not None:
        first = next((i for i, (key, _) in enumerate(block) if cmp(key, lo) > (0 if lo_excl else -1)), n)
        found_lo = first < n if lo_excl else first < n and cmp(block[first][0], lo) == 0
    if hi is not None:
        end = next((i for i, (key, _) in enumerate(block) if cmp(key, hi) > (-1 if hi_excl else 0)), n)
        found_hi = end > 0 if hi_excl else end > 0 and cmp(block[end - 1][0], hi) == 0
    return min(first, end), end, found_lo, found_hi


@functools.lru_cache(maxsize=None)
def _mutant_inputs():
    """The blocks at restart interval 3 with a hash index as key lists, the point-read and seek
    queries (one flag value per pair) and the oracle's answers."""
    buf, off = K.blocks(3, 1.33)
    s = K.block_starts()
    pls = [K.payload(buf, off, b) for b in range(len(off) - 1)]
    lists = []
    for b, pl in enumerate(pls):
        n, p = pyoracle.data_block_decode(pl)
        got = [(k, q) for k, _, q, _ in pyoracle.materialize(pl, p, 3)]
        assert got == [(r[0], r[2]) for r in K.rows()[int(s[b]):int(s[b + 1])]]
        lists.append(got)
    points = [(b, n, min(snap, K.SNAP_ALL - 1)) for b, n, snap in K.point_queries()]
    seeks = [(b, lo if f & 1 else None, hi if f & 2 else None, bool(f & 4), bool(f & 8))
             for b, lo, hi, f in K.one_flag_per_pair(K.seek_queries())]
    return (lists, points, seeks, [pyoracle.point_read(pls[q[0]], *q[1:]) for q in points],
            [pyoracle.seek(pls[q[0]], *q[1:]) for q in seeks])


def _model_answers(cmp):
    lists, points, seeks, _, _ = _mutant_inputs()
    return ([model_point_read(lists[b], n, snap, cmp) for b, n, snap in points],
            [model_seek(lists[q[0]], *q[1:], cmp) for q in seeks])


def test_true_comparator_reproduces_the_oracle():
    _, points, seeks, want_points, want_seeks = _mutant_inputs()
    got_points, got_seeks = _model_answers(cmp_true)
    assert got_points == want_points
    assert got_seeks == want_seeks
    assert len(seeks) >= 4000 and len(points) >= 8000


@pytest.mark.parametrize("mutant", MUTANTS, ids=lambda f: f.__name__)
def test_wrong_comparator_changes_answers(mutant):
    _, points, seeks, want_points, want_seeks = _mutant_inputs()
    got_points, got_seeks = _model_answers(mutant)
    killed_points = sum(g != w for g, w in zip(got_points, want_points))
    killed_seeks = sum(g != w for g, w in zip(got_seeks, want_seeks))
    print("%s: %d of %d point reads, %d of %d seeks changed" % (mutant.__name__, killed_points, len(points),
                                                             killed_seeks, len(seeks)))
    assert killed_points >= 50 and killed_seeks >= 50, (killed_points, killed_seeks)
