"""GPU parity of the four lookup entry points (lsm_point_read_blocks, lsm_seek_blocks,
lsm_table_get, lsm_table_range) on keys and needles longer than one 16-byte compare window:
the inputs of tests/long_key_cases.py (what they cover is asserted on the CPU by
tests/test_long_key_cases.py), against the oracle (point read, seek) and the Python table
models (get, range), never against the library itself.  Bar: every output of every query
equals the reference's."""
import numpy as np
import pytest

import long_key_cases as K
import pyoracle
import test_gpu_table_get as G
import test_gpu_table_range as R
from table_get_model import GET_FILTERED, GET_HIT, TableModel
from table_range_model import RANGE_EMPTY, RANGE_ROWS
from test_gpu_point_read import _check, _run

pytestmark = pytest.mark.gpu


def _arena(parts):
    off = np.zeros(len(parts) + 1, np.int64)
    off[1:] = np.cumsum([len(p) for p in parts])
    return np.frombuffer(b"".join(parts) or b"\0", np.uint8), off


def _seek(gpu, buf, off, qs):
    """qs: [(block, lo, hi, flags)] -> (first, end, found) numpy arrays; every status must be OK."""
    import torch
    (lo, loff), (hi, hoff) = _arena([q[1] for q in qs]), _arena([q[2] for q in qs])
    res = gpu.seek(gpu.to_device_bytes(buf), torch.from_numpy(off.astype(np.int64)).cuda(), len(off) - 1,
                   torch.tensor([q[0] for q in qs], dtype=torch.int32).cuda(), gpu.to_device_bytes(lo),
                   torch.from_numpy(loff).cuda(), gpu.to_device_bytes(hi), torch.from_numpy(hoff).cuda(),
                   torch.tensor([q[3] for q in qs], dtype=torch.uint8).cuda())
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy()[:len(qs)] for k, v in res.items()}
    assert (res["status"] == 0).all()
    return res["first"].astype(np.int64), res["end"].astype(np.int64), res["found"]


def _check_seek(gpu, buf, off, qs):
    first, end, found = _seek(gpu, buf, off, qs)
    pls = [K.payload(buf, off, b) for b in range(len(off) - 1)]
    want = np.array([pyoracle.seek(pls[b], lo if fl & 1 else None, hi if fl & 2 else None, bool(fl & 4), bool(fl & 8))
                     for b, lo, hi, fl in qs], np.int64)
    got = np.stack([first, end, found & 1, (found >> 1) & 1], axis=1)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, (len(bad), [(int(q), qs[q][0], qs[q][1][-20:], qs[q][2][-20:], qs[q][3], got[q], want[q])
                                    for q in bad[:5]])
    return first, end


# ---- lsm_point_read_blocks
@pytest.mark.parametrize("ratio", K.HASH_RATIOS)
@pytest.mark.parametrize("ri", K.RESTART_INTERVALS)
def test_point_read_long_keys(gpu, ri, ratio):
    buf, off = K.blocks(ri, ratio)
    qs = K.point_queries()
    hits = _check(gpu, buf, off, qs)
    assert 10 * hits >= len(qs), (hits, len(qs))


@pytest.mark.parametrize("filler", [0, 1, 7, 15])
def test_point_read_needle_alignment(gpu, filler):
    """The same queries behind 0, 1, 7 and 15 bytes of filler at the start of the needle arena (a
    first query that owns them), so that a long needle starts at every alignment of its first
    window in one of the runs."""
    buf, off = K.blocks(3, 1.33)
    qs = [(0, b"\xa5" * filler, K.SNAP_ALL)] + K.point_queries()
    at, long_at = 0, set()
    for _, needle, _ in qs:
        if len(needle) >= 33:
            long_at.add(at % 16)
        at += len(needle)
    assert long_at == set(range(16))
    assert 10 * _check(gpu, buf, off, qs) >= len(qs)


# ---- lsm_seek_blocks
@pytest.mark.parametrize("ri", K.RESTART_INTERVALS)
def test_seek_long_keys(gpu, ri):
    buf, off = K.blocks(ri, K.HASH_RATIOS[ri % 2])
    qs = K.seek_queries()
    first, end = _check_seek(gpu, buf, off, qs)
    # the huge needle (the last pair, on the last block) as a lower bound: past every item
    n_items = int(K.block_starts()[-1] - K.block_starts()[-2])
    assert qs[-15][3] == 1 and (first[-15], end[-15]) == (n_items, n_items)
    assert int((first < end).sum()) >= len(qs) // 8  # (most bounded pairs are narrow or crossed)


# ---- lsm_table_get
@pytest.mark.parametrize("two_level,filtered,hashes", [(False, False, False), (True, False, False),
                                                        (False, True, False), (False, True, True),
                                                        (True, True, False), (True, True, True)])
def test_table_get_long_keys(gpu, two_level, filtered, hashes):
    """Every needle and every row's key on the four table variants; with a filter block, once with
    the kernel hashing the needle and once with the host's hashes."""
    file, t, flt = K.table(two_level, filtered)
    qs = K.get_queries()
    outcomes = G.compare(G.run(gpu, file, t, qs, filter=flt, hashes=hashes), qs, K.get_expected(two_level, filtered))
    assert outcomes[GET_HIT] >= 2000 and (outcomes.get(GET_FILTERED, 0) >= 1000) == filtered, outcomes


# ---- lsm_table_range
@pytest.mark.parametrize("with_scan", [False, True])
@pytest.mark.parametrize("two_level", [False, True])
def test_table_range_long_keys(gpu, two_level, with_scan):
    """Bound pairs from the needle set under all 16 flag values; with the scan offsets also the
    block ordinals and the row window, which is the window of the sorted item list."""
    file, t, _ = K.table(two_level, False)
    qs, expected = K.range_queries(), K.range_expected(two_level)
    if not with_scan:
        outcomes = R.compare(R.run(gpu, file, t, qs), qs, expected)
    else:
        d_file = gpu.to_device_bytes(file)
        scan = gpu.scan_table(d_file, len(file), t["tli_off"], t["tli_size"], two_level=two_level)
        assert scan["table_status"] == 0 and scan["n_blocks"] == t["block_count"]
        res = R.run(gpu, d_file, dict(t, file_len=len(file)), qs, scan=scan)
        outcomes = R.compare(res, qs, expected, ordinal=R.ordinals(t["block_off"]))
        keys = [r[0] for r in K.rows()]
        want = np.array([K.window(keys, *q) for q in qs], np.int64)
        want[want[:, 0] == want[:, 1]] = 0
        bad = np.nonzero((res["row_first"] != want[:, 0]) | (res["row_end"] != want[:, 1]))[0]
        assert len(bad) == 0, (len(bad), [(int(q), int(res["row_first"][q]), int(res["row_end"][q]), want[q])
                                        for q in bad[:5]])
    assert outcomes[RANGE_ROWS] >= 2000 and outcomes[RANGE_EMPTY] >= 1000, outcomes


# ---- keys at the u16 limit
def test_u16_limit_point_read(gpu):
    """Keys of 65,534 and 65,535 bytes, shared lengths of 65,534 and 65,535 (three-byte varints)
    and a zero-byte suffix; every row key above and below each seqno, the near misses, and the
    70,000-byte needle, which is a miss."""
    buf, off = K.u16_blocks()
    qs = K.u16_point_queries()
    assert _check(gpu, buf, off, qs) >= 20
    huge = [q for q, (_, needle, _) in enumerate(qs) if len(needle) == K.HUGE]
    res = _run(gpu, buf, off, [qs[q] for q in huge])
    assert len(huge) == 2 and (res["item"] == -1).all() and (res["status"] == 0).all()


def test_u16_limit_seek(gpu):
    buf, off = K.u16_blocks()
    qs = K.u16_seek_queries()
    first, end = _check_seek(gpu, buf, off, qs)
    lower = [q for q, (_, lo, _, fl) in enumerate(qs) if len(lo) == K.HUGE and fl == 1]
    assert len(lower) == 4 and all((first[q], end[q]) == (4, 4) for q in lower)


def test_u16_limit_table(gpu):
    """The four rows as a two-level table (one row per block, one handle per partition: every index
    seek compares end keys at the u16 limit) through table_get and table_range."""
    file, t = K.u16_table()
    qs = K.u16_get_queries()
    model = TableModel(file, t["tli_off"], t["tli_size"], True)
    outcomes = G.compare(G.run(gpu, file, t, qs), qs, G.expect(model, qs))
    assert outcomes[GET_HIT] >= 8, outcomes
    rq = K.u16_range_queries()
    _, outcomes = R.check(gpu, file, t, rq)
    assert outcomes[RANGE_ROWS] >= 50 and outcomes[RANGE_EMPTY] >= 10, outcomes
