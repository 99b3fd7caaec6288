"""The order of the checks that open a block, which decides the status of a block with two
faults.  lsm_point_read_blocks and lsm_seek_blocks are given a block's extent and test it
against the header's data_length (TRUNCATED) before the block type (TYPE_MISMATCH);
lsm_table_get's load_block follows the reference's load_block (src/table/util.rs:79-86) and
tests the type first.  One sound ten-item block, its damaged variants, one query each.  The
kernels do not verify header checksums, so no header is re-sealed."""
import numpy as np
import pytest

import pyoracle
from helpers import counter_items, index_items, pack
from table_get_model import GET_NONE, item_key
from test_gpu_table_get import _hand_table, run as table_get_run

pytestmark = pytest.mark.gpu

OK, BAD_MAGIC, BAD_TYPE, PARSE, TYPE_MISMATCH, TRUNCATED, BAD_ARG = 0, 1, 2, 5, 7, 8, 10


def _patched(block, type_byte=None, data_length_add=0, flip=None):
    b = bytearray(block)
    if type_byte is not None:
        b[4] = type_byte
    if data_length_add:
        b[21:25] = (int.from_bytes(b[21:25], "little") + data_length_add).to_bytes(4, "little")
    if flip is not None:
        b[flip[0]] ^= flip[1]
    return bytes(b)


def _sound():
    items = counter_items(10, seed=2)
    buf, off = pyoracle.encode_blocks(items, np.array([0, 10], np.uint32))
    return bytes(buf[:int(off[1])]), item_key(items, 0), item_key(items, 9)


@pytest.fixture(scope="module")
def answers(gpu):
    """(expected statuses, point_read result, seek result) of the eleven queries."""
    import torch
    sound, key, _ = _sound()
    ibuf, ioff = pyoracle.encode_blocks(index_items(10), np.array([0, 10], np.uint32), block_type=1)
    cases = [(sound, OK),
             (bytes(ibuf[:int(ioff[1])]), TYPE_MISMATCH),                      # an index block in a data slot
             (_patched(sound, type_byte=1, data_length_add=1), TRUNCATED),     # extent is tested before type
             (_patched(sound, data_length_add=1), TRUNCATED),
             (_patched(sound, flip=(1, 0x20)), BAD_MAGIC),
             (_patched(sound, type_byte=9), BAD_TYPE),
             (sound[:20], TRUNCATED),
             (sound[:3], TRUNCATED),
             (_patched(sound, flip=(len(sound) - 31 + 2, 0x7F)), PARSE)]       # trailer bin_len
    buf, off = pack([c[0] for c in cases])
    off = np.append(off, np.uint64(0))  # slot 9: a descending block_off pair
    n_blocks = len(off) - 1
    want = [c[1] for c in cases] + [TRUNCATED, BAD_ARG]  # the last query names block n_blocks
    n = len(want)
    d_buf, d_off = gpu.to_device_bytes(buf), torch.from_numpy(off.astype(np.int64)).cuda()
    q_block = torch.arange(n, dtype=torch.int32).cuda()
    keys = gpu.to_device_bytes(np.frombuffer(key * n, np.uint8))
    key_off = torch.arange(0, 16 * (n + 1), 16, dtype=torch.int64).cuda()
    pr = gpu.point_read(d_buf, d_off, n_blocks, q_block, keys, key_off,
                        torch.full((n,), (1 << 63) - 1, dtype=torch.int64).cuda())
    sk = gpu.seek(d_buf, d_off, n_blocks, q_block, keys, key_off, keys, key_off,
                  torch.full((n,), 3, dtype=torch.uint8).cuda())
    torch.cuda.synchronize()
    return want, {k: v.cpu().numpy()[:n] for k, v in pr.items()}, {k: v.cpu().numpy()[:n] for k, v in sk.items()}


def test_point_read_check_order(answers):
    want, pr, _ = answers
    print("point_read status", list(pr["status"]), "item", list(pr["item"]))
    assert list(pr["status"]) == want
    assert list(pr["item"]) == [0 if st == OK else -1 for st in want]


def test_seek_check_order(answers):
    want, _, sk = answers
    print("seek status", list(sk["status"]), "first", list(sk["first"]), "end", list(sk["end"]), "found", list(sk["found"]))
    assert list(sk["status"]) == want
    assert (int(sk["first"][0]), int(sk["end"][0]), int(sk["found"][0])) == (0, 1, 3)  # [key, key] in the sound block
    for q, st in enumerate(want):
        if st != OK:
            assert (int(sk["first"][q]), int(sk["end"][q]), int(sk["found"][q])) == (0, 0, 0), q


@pytest.mark.parametrize("type_byte,want", [(1, TYPE_MISMATCH), (None, TRUNCATED)])
def test_table_get_check_order(gpu, type_byte, want):
    """load_block: the type is tested before the extent."""
    sound, key, end_key = _sound()
    file, table = _hand_table([_patched(sound, type_byte=type_byte, data_length_add=1)],
                              lambda h: [(end_key, 63) + h[0]])
    res = table_get_run(gpu, file, table, [(key, 64)])
    print("table_get status", int(res["status"][0]), "outcome", int(res["outcome"][0]))
    assert (int(res["status"][0]), int(res["outcome"][0]), int(res["item"][0])) == (want, GET_NONE, -1)
