"""decode_blocks_kernel's per-group chain: the wave that runs phase A also does the group's
header fields, trailers and interval numbering (group_block_meta: all loads at once, statuses
selected afterwards) and goes on without a barrier, while the three hash waves start at the
DMA barrier from the block handles and their verdicts are applied in the status merge.

Everything here is checked against pyoracle.decode_blocks the way tests/test_gpu_parity.py
does it: statuses and item_start for every block, every field of every accepted block.  The
outputs are seeded with a canary: rows behind the last item, and rows of blocks that are
rejected before any record is described (header fields, data length, type, trailer), must
still hold it.  Each case runs through lsm_decode_blocks and lsm_decode_blocks16, with and
without LSM_DECODE_ITEM_START_VALID.

tests/golden/decode_group_chain.json holds what the library gave for the status batch BEFORE
this kernel change (generated from the parent commit's build by
tests/golden/make_decode_group_chain.py on an MI355X): its statuses with and without
LSM_DECODE_PAYLOAD_VERIFIED, and SHA-256 digests of the canary-seeded output arrays with the
rows of PARSE / OVERFLOW blocks masked (a block that fails in phase B keeps whichever of its
records were stored before the failure was seen, which depends on timing).
"""
import functools
import hashlib
import json

import numpy as np
import pytest

import pyoracle
from conftest import GOLDEN
from helpers import counter_items, index_items, pack

pytestmark = pytest.mark.gpu

CANARY = 0xA5
FIELD32 = {"seqno": np.uint64, "key_off": np.uint32, "val_off": np.uint32, "val_len": np.uint32,
           "key_len": np.uint16, "prefix_len": np.uint16, "vtype": np.uint8, "handle_off": np.uint64}
FIELD16 = {"seqno": np.uint64, "key_off": np.uint16, "val_off": np.uint16, "val_len": np.uint16,
           "key_len": np.uint16, "prefix_len": np.uint16, "vtype": np.uint8}
ITEM_START_VALID, PAYLOAD_VERIFIED = 1, 2
UNSUPPORTED, PARSE, OVERFLOW = 9, 5, 6
# (compact, item_start given)
MODES = [pytest.param(c, v, id=("blocks16" if c else "blocks") + ("-item_start" if v else ""))
         for c in (False, True) for v in (False, True)]
FIXTURE = GOLDEN / "decode_group_chain.json"


# ------------------------------------------------------------------ batches (built once, never changed)

def _blocks_of(buf, off):
    return [bytes(buf[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]


@functools.lru_cache(maxsize=None)
def data_blocks(n_blocks, items_per_block=52, ri=16, seed=31):
    """n_blocks blocks of the configs[1] record shape (16 B counter keys, 64 B values)."""
    items = counter_items(items_per_block * n_blocks, seed=seed)
    starts = np.arange(0, items_per_block * (n_blocks + 1), items_per_block, dtype=np.uint32)
    buf, off = pyoracle.encode_blocks(items, starts, restart_interval=ri, nthreads=2)
    return tuple(_blocks_of(buf, off))


def _reseal_header(blk):
    """The header checksum (low 32 bits of XXH3-128 over its first 29 bytes) recomputed."""
    b = bytearray(blk)
    b[29:33] = (pyoracle.xxh3_128(bytes(b[:29])) & 0xFFFFFFFF).to_bytes(4, "little")
    return bytes(b)


def _flip(blk, pos, bit=0x10):
    b = bytearray(blk)
    b[pos] ^= bit
    return bytes(b)


def _payload_edit(blk, fn, block_type=0):
    p = bytearray(blk[33:])
    fn(p)
    return pyoracle.block_write(bytes(p), block_type)


def _break_count(p):
    p[-4] ^= 1  # trailer item count


def _break_record(p):
    p[0] = 0x7F  # the first record's value type


# block -> (what is wrong with it, rows stay untouched: it is rejected before phase A describes a record)
STATUS_FAULTS = {
    0: ("bad magic", True),
    4: ("header checksum byte flipped", False),
    8: ("payload byte flipped", False),
    9: ("data_length off by one, header re-sealed", True),
    11: ("index block type against expect_type 0", True),
    13: ("trailer item count broken, re-sealed", False),  # 53 for 52: the same interval count, so phase A finds it
    15: ("first record broken, re-sealed", False),
    17: ("header checksum byte and payload byte flipped", False),
    19: ("payload byte flipped inside the trailer (checksum and trailer both bad)", False),
}


@functools.lru_cache(maxsize=None)
def status_batch():
    """20 blocks of the configs[1] shape (3.7 KB: eight per 32 KiB stage, nine where they run
    shorter): faults on the first block of a group (0, and 8 or 9), on the last (8 or 15, 19) and
    in the middle (4, 11, 13, 17); the other eleven blocks are valid."""
    blocks = list(data_blocks(20, seed=41))
    good = list(blocks)
    blocks[0] = _flip(good[0], 1, 0x40)
    blocks[4] = _flip(good[4], 30)
    blocks[8] = _flip(good[8], 33 + 60)  # inside the first record's value
    b = bytearray(good[9])
    b[21] ^= 1
    blocks[9] = _reseal_header(bytes(b))
    blocks[11] = pyoracle.block_write(good[11][33:], 1)
    blocks[13] = _payload_edit(good[13], _break_count)
    blocks[15] = _payload_edit(good[15], _break_record)
    blocks[17] = _flip(_flip(good[17], 7), 33 + 60)
    blocks[19] = _flip(good[19], len(good[19]) - 4, 0x01)
    assert [len(x) for x in blocks] == [len(x) for x in good]
    buf, off = pack(blocks)
    return buf, off


@functools.lru_cache(maxsize=None)
def oracle_of(key, expect_type=-1):
    buf, off = BATCHES[key]()
    return pyoracle.decode_blocks(buf, off, expect_type=expect_type, nthreads=2)


def _index_mix():
    """Index blocks between data blocks (the group kernel hands them on from inside its loop)
    and two data blocks larger than the stage (listed before the loop)."""
    idx = index_items(600)
    ibuf, ioff = pyoracle.encode_blocks(idx, np.array([0, 40, 41, 200, 330, 600], np.uint32), block_type=1, nthreads=2)
    ib = _blocks_of(ibuf, ioff)
    d = data_blocks(12, seed=43)
    big = data_blocks(2, items_per_block=600, seed=44)
    assert len(big[0]) > 40 * 1024
    order = [d[0], ib[0], d[1], d[2], big[0], ib[1], ib[2], d[3], d[4], d[5], d[6], d[7], d[8], ib[3], d[9], big[1],
             d[10], ib[4], d[11]]
    return pack(order)


BATCHES = {
    "status": status_batch,
    "index_mix": functools.lru_cache(maxsize=None)(_index_mix),
    "two_16k": lambda: pack(list(data_blocks(2, items_per_block=205, seed=35))),  # k = 2: a wave per block
    "ri1_2": lambda: pack(list(data_blocks(2, ri=1, seed=36))),    # 104 intervals: phase A on two waves
    "ri1_10": lambda: pack(list(data_blocks(10, ri=1, seed=37))),  # 468 intervals in the full group: three waves
}
for _n in (1, 2, 5, 9, 10, 13, 55):  # one group; k = 4 h + 1 (5, 9, 13); a full group + 1; two workgroups
    BATCHES[f"c1_{_n}"] = functools.partial(lambda n: pack(list(data_blocks(n))), _n)


# ------------------------------------------------------------------ the GPU call and the comparison

def decode_canary(gpu, buf, off, compact, item_start=None, expect_type=-1, flags=0):
    """Decode into outputs filled with CANARY; item_start given: LSM_DECODE_ITEM_START_VALID."""
    import torch
    n = len(off) - 1
    cap = len(buf) // 3 + 1
    d_blocks = gpu.to_device_bytes(buf)
    d_off = torch.from_numpy(off.astype(np.int64)).cuda()
    dec = gpu.Decoder()
    out = dec.alloc_outputs(cap, n, compact=compact)
    for t in out.values():
        t.view(torch.uint8).fill_(CANARY)
    if item_start is not None:
        out["item_start"].copy_(torch.from_numpy(item_start.view(np.int32)))
        flags |= ITEM_START_VALID
    dec.decode(d_blocks, d_off, n, out, cap, expect_type=expect_type, tuning=(0, 0, 0, flags) if flags else None,
               compact=compact, pool=False)
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res["status"] = res["status"][:n].astype(np.int32)
    return res


def compact_expected(buf, off, status):
    """lsm_decode_blocks16: index blocks and payloads over 65535 bytes the oracle would parse
    are LSM_UNSUPPORTED (tests/test_gpu_compact.py)."""
    exp = status.copy()
    for b in range(len(off) - 1):
        blk = bytes(buf[int(off[b]):int(off[b + 1])])
        _, h = pyoracle.header_decode(blk)
        if status[b] in (0, PARSE, OVERFLOW) and (h.block_type == 1 or len(blk) - 33 > 0xFFFF):
            exp[b] = UNSUPPORTED
    return exp


def check(gpu, key, compact, given, expect_type=-1, flags=0, exp_status=None, untouched=()):
    buf, off = BATCHES[key]()
    parsed, item_start, status = oracle_of(key, expect_type)
    exp = compact_expected(buf, off, status) if compact else status
    if exp_status is not None:
        exp = np.asarray(exp_status, np.int32)
    g = decode_canary(gpu, buf, off, compact, item_start if given else None, expect_type, flags)
    assert (g["status"] == exp).all(), (key, np.nonzero(g["status"] != exp)[0][:10], g["status"], exp)
    assert (g["item_start"].view(np.uint32) == item_start).all(), key
    starts = item_start.astype(np.int64)
    n = int(starts[-1])
    accepted = np.zeros(n, bool)
    for b in np.nonzero((exp == 0) & (status == 0))[0]:
        accepted[starts[b]:starts[b + 1]] = True
    keep = np.zeros(n, bool)
    for b in untouched:
        keep[starts[b]:starts[b + 1]] = True
    for f, dt in (FIELD16 if compact else FIELD32).items():
        gv = g[f].view(dt)
        o = parsed[f][:n].astype(dt)
        bad = np.nonzero((gv[:n] != o) & accepted)[0]
        assert len(bad) == 0, (key, f, bad[:10], gv[bad[:10]], o[bad[:10]])
        raw = g[f].view(np.uint8).reshape(len(gv), -1)
        assert (raw[n:] == CANARY).all(), (key, f, "rows behind the last item")
        assert (raw[:n][keep] == CANARY).all(), (key, f, "rows of a block rejected before phase A")
    return g, exp, starts


def digests(g, exp, starts, compact):
    """SHA-256 per output array, rows of PARSE / OVERFLOW blocks zeroed."""
    n = int(starts[-1])
    mask = np.zeros(n, bool)
    for b in np.nonzero((exp == PARSE) | (exp == OVERFLOW))[0]:
        mask[starts[b]:starts[b + 1]] = True
    out = {}
    for f, dt in (FIELD16 if compact else FIELD32).items():
        v = g[f].view(dt).copy()
        v[:n][mask] = 0
        out[f] = hashlib.sha256(v.tobytes()).hexdigest()
    return out


# ------------------------------------------------------------------ tests

@pytest.mark.parametrize("compact,given", MODES)
@pytest.mark.parametrize("key", [k for k in BATCHES if k.startswith("c1_")] + ["two_16k", "ri1_2", "ri1_10"])
def test_group_shapes(gpu, key, compact, given):
    _, exp, _ = check(gpu, key, compact, given)
    assert (exp == 0).all()


@pytest.mark.parametrize("compact,given", MODES)
def test_status_order(gpu, compact, given):
    """One fault per block, two in some: the oracle's order header -> header checksum ->
    payload checksum -> data length / type / trailer -> parse."""
    untouched = [b for b, (_, u) in STATUS_FAULTS.items() if u]
    g, exp, starts = check(gpu, "status", compact, given, expect_type=0, untouched=untouched)
    assert sorted(np.nonzero(exp)[0]) == sorted(STATUS_FAULTS), exp
    assert len(set(exp[list(STATUS_FAULTS)])) >= 6, exp  # the faults are told apart
    want = json.loads(FIXTURE.read_text())["plain"]["blocks16" if compact else "blocks"]
    assert list(exp) == want["status"]
    assert digests(g, exp, starts, compact) == want["sha256"]


@pytest.mark.parametrize("compact,given", MODES)
def test_payload_verified(gpu, compact, given):
    """LSM_DECODE_PAYLOAD_VERIFIED: payload corruption is not reported, every header and trailer
    fault still is, as the library reported them before the kernel change (the fixture)."""
    want = json.loads(FIXTURE.read_text())["verified"]["blocks16" if compact else "blocks"]
    untouched = [b for b, (_, u) in STATUS_FAULTS.items() if u]
    g, exp, starts = check(gpu, "status", compact, given, expect_type=0, flags=PAYLOAD_VERIFIED,
                           exp_status=want["status"], untouched=untouched)
    _, _, status = oracle_of("status", 0)
    # what the fixture itself must say: header-field, data-length, type, trailer and record faults
    # as the oracle has them; the flipped value byte unseen; the flipped trailer byte a trailer
    # fault.  (Blocks 4 and 17: the header checksum is computed by the hash waves, which the flag
    # turns off, so the fixture alone says what they give.)
    for b in (0, 9, 11, 13, 15):
        assert exp[b] == status[b] != 0, (b, STATUS_FAULTS[b][0])
    assert exp[8] == 0 and exp[19] == PARSE, exp
    assert digests(g, exp, starts, compact) == want["sha256"]


@pytest.mark.parametrize("compact,given", MODES)
def test_index_blocks_between_data_blocks(gpu, compact, given):
    _, exp, _ = check(gpu, "index_mix", compact, given)
    assert ((exp == 0).all() if not compact else sorted(set(exp)) == [0, UNSUPPORTED]), exp
