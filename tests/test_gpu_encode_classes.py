"""The encode size classes at their edges.  A block the group kernel does not take is written, by
the LDS image it needs (e2_need, csrc/encode_plan.hpp: the block, pad and read slack, and the
hash-index vote arrays), by one wave (medium, <= 20 KiB), by eight waves (big, <= 96 KiB) or straight
in HBM (huge: one workgroup per block, or across the GPU with the workspace pool).  Pinned here,
every expected byte, offset and status from the oracle:
  * fine sweeps of block sizes over the medium | big and the big | huge boundary;
  * big blocks on both sides of the binary index's 2 | 4 byte step;
  * huge blocks of 255..258 items (256: the workgroup scan | the plan's record offsets);
  * huge blocks whose hash index takes one, two and three LDS passes of 4096 buckets;
  * index blocks in the listed classes;
  * an output capacity that cuts through a block of each class;
  * in every batch, listed blocks at 16-byte aligned and at unaligned output offsets (the two arms
    of the ragged copy-out).
The size conditions are asserted from the oracle's output before anything runs on the device."""
import ctypes as C
import functools

import numpy as np
import pytest

import pyoracle
from helpers import index_items

pytestmark = pytest.mark.gpu

KIB = 1024
IMG_MEDIUM, IMG_BIG = 20 * KIB, 96 * KIB  # csrc/encode_common.hpp: kImgMedium, kImgBig
GROUP_IMG = 15872                         # kGImg: no block above it is group-class
HDR, TRAILER = 33, 31
OK, OVERFLOW = 0, 6
MARKER = 0xA5


def _items(vlens, key_len=16, seed=1):
    """Big-endian counter keys, random values of the given lengths, no tombstones."""
    vlens = np.asarray(vlens, np.uint64)
    n = len(vlens)
    rng = np.random.default_rng(seed)
    ctr = np.arange(n, dtype=np.uint64)
    keys = np.zeros((n, key_len), np.uint8)
    for b in range(8):
        keys[:, key_len - 1 - b] = ((ctr >> np.uint64(8 * b)) & np.uint64(0xFF)).astype(np.uint8)
    val_off = np.concatenate([[0], np.cumsum(vlens)]).astype(np.uint64)
    vals = rng.integers(0, 256, int(val_off[-1]), dtype=np.uint8)
    return pyoracle.Items(keys.reshape(-1), np.arange(n + 1, dtype=np.uint64) * np.uint64(key_len), vals, val_off,
                          np.full(n, 63, np.uint64), np.zeros(n, np.uint8))


def _spread(total, n):
    """n value lengths that add up to total, equal within one byte."""
    return [total // n + (1 if i < total % n else 0) for i in range(n)]


def _blocks(value_bytes, n, seed=1):
    """One block of n items per entry of value_bytes (the block's value bytes in all)."""
    vlens = [v for total in value_bytes for v in _spread(total, n)]
    return _items(vlens, seed=seed), np.arange(len(value_bytes) + 1, dtype=np.uint32) * np.uint32(n)


def _trailer(buf, off, b):
    """(step, hash-index bytes) of block b, trailer.rs:118-163."""
    t = bytes(buf[int(off[b + 1]) - TRAILER:int(off[b + 1])])
    return t[1], int.from_bytes(t[10:14], "little")


def _need(buf, off, b):
    """e2_need of block b."""
    total = int(off[b + 1]) - int(off[b])
    return ((15 + total + 15) & ~15) + 32 + 8 * ((_trailer(buf, off, b)[1] + 3) & ~3)


def _both_alignments(off, listed):
    rem = {int(off[b]) % 16 for b in listed}
    assert 0 in rem and len(rem) > 1, sorted(rem)


def _gpu_encode(gpu, items, starts, ri=16, ratio=0.0, off32=False, block_type=0, pool=False):
    import torch
    d_items = gpu.items_to_device(items, off32=off32)
    d_starts = torch.from_numpy(np.asarray(starts, np.int64).astype(np.int32)).cuda()
    nb = len(starts) - 1
    out = gpu.Encoder().encode(d_items, d_starts, nb, restart_interval=ri, hash_ratio=ratio, block_type=block_type,
                               pool=pool)
    torch.cuda.synchronize()
    off = out["block_off"].cpu().numpy().view(np.uint64)
    return out["buf"].cpu().numpy()[:int(off[-1])], off, out["status"].cpu().numpy()[:nb]


def _check(gpu, items, starts, ref, **kw):
    ref_buf, ref_off = ref
    buf, off, st = _gpu_encode(gpu, items, starts, **kw)
    assert (st == OK).all(), st
    assert (off == ref_off).all()
    bad = [b for b in range(len(starts) - 1)
           if buf[int(off[b]):int(off[b + 1])].tobytes() != ref_buf[int(off[b]):int(off[b + 1])].tobytes()]
    assert not bad, bad


# ------------------------------------------------------------------ class boundaries
# Blocks of a fixed item count whose value bytes grow by 100 per block: the sizes rise in steps of
# 100 B, and the hash index (so the vote arrays' share of e2_need) is the same for every block.
# (items per block, first block's value bytes by restart interval, blocks; restart interval 1 has the
# larger binary index)
SWEEPS = {IMG_MEDIUM: (40, {16: 18100, 1: 18100}, 30), IMG_BIG: (160, {16: 94300, 1: 91600}, 36)}


@functools.lru_cache(maxsize=None)
def _sweep(limit, ri, ratio):
    n, first, count = SWEEPS[limit]
    v0 = first[ri]
    items, starts = _blocks([v0 + 100 * k for k in range(count)], n, seed=limit // KIB + ri)
    buf, off = pyoracle.encode_blocks(items, starts, restart_interval=ri, hash_ratio=ratio)
    sizes = np.diff(off.astype(np.int64))
    need = np.array([_need(buf, off, b) for b in range(count)])
    assert sizes.min() > GROUP_IMG and (np.abs(np.diff(sizes) - 100) <= 8).all(), sizes
    assert sizes.min() <= limit - 512 and sizes.max() >= limit + 512, (sizes.min(), sizes.max())
    assert need.min() <= limit - 512 and need.max() >= limit + 512, (need.min(), need.max())  # both classes
    assert (_trailer(buf, off, 0)[1] > 0) == (ratio > 0)
    _both_alignments(off, range(count))
    return items, starts, (buf, off)


@pytest.mark.parametrize("off32", [False, True])
@pytest.mark.parametrize("ratio", [0.0, 1.33])
@pytest.mark.parametrize("ri", [16, 1])
def test_medium_big_boundary(gpu, ri, ratio, off32):
    items, starts, ref = _sweep(IMG_MEDIUM, ri, ratio)
    _check(gpu, items, starts, ref, ri=ri, ratio=ratio, off32=off32)


@pytest.mark.parametrize("pool", [True, False])
@pytest.mark.parametrize("off32", [False, True])
@pytest.mark.parametrize("ratio", [0.0, 1.33])
@pytest.mark.parametrize("ri", [16, 1])
def test_big_huge_boundary(gpu, ri, ratio, off32, pool):
    items, starts, ref = _sweep(IMG_BIG, ri, ratio)
    _check(gpu, items, starts, ref, ri=ri, ratio=ratio, off32=off32, pool=pool)


# ------------------------------------------------------------------ binary-index step
@pytest.mark.parametrize("ratio", [0.0, 1.33])
def test_big_blocks_binary_index_step(gpu, ratio):
    """Big blocks whose last restart head lies on both sides of offset 65,535: 2- and 4-byte entries."""
    n = 300
    items, starts = _blocks([60000 + 700 * k for k in range(12)], n, seed=3)
    buf, off = pyoracle.encode_blocks(items, starts, restart_interval=16, hash_ratio=ratio)
    steps = [_trailer(buf, off, b)[0] for b in range(12)]
    need = [_need(buf, off, b) for b in range(12)]
    assert set(steps) == {2, 4} and steps == sorted(steps), steps
    assert min(need) > IMG_MEDIUM and max(need) <= IMG_BIG, need
    _both_alignments(off, range(12))
    _check(gpu, items, starts, (buf, off), ri=16, ratio=ratio)


# ------------------------------------------------------------------ huge blocks around 256 items
@pytest.mark.parametrize("pool", [True, False])
@pytest.mark.parametrize("ratio", [0.0, 1.33])
def test_huge_blocks_256_items(gpu, ratio, pool):
    """Up to 256 items a huge block's record offsets come from the writer's own workgroup scan,
    above from the plan's."""
    counts = [255, 256, 257, 258, 256, 257]
    # (the first block's value bytes make its size a multiple of 16: the second starts aligned too)
    for pad in range(16):
        vlens = [500 + (pad if i == 0 else 0) for i in range(sum(counts))]
        items = _items(vlens, seed=5)
        starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
        buf, off = pyoracle.encode_blocks(items, starts, restart_interval=16, hash_ratio=ratio)
        if int(off[1]) % 16 == 0:
            break
    assert all(_need(buf, off, b) > IMG_BIG for b in range(len(counts)))
    assert (_trailer(buf, off, 0)[1] > 0) == (ratio > 0)
    _both_alignments(off, range(len(counts)))
    _check(gpu, items, starts, (buf, off), ri=16, ratio=ratio, pool=pool)


# ------------------------------------------------------------------ hash-index passes
@pytest.mark.parametrize("pool", [True, False])
def test_huge_blocks_hash_index_passes(gpu, pool):
    """Hash indexes of 4096, 4097 and more than 8192 buckets: one, two and three passes of the vote
    arrays.  Restart interval 32 keeps the restart count <= 254, so the index is kept
    (trailer.rs:100-111)."""
    counts = [3080, 3081, 6161, 3080]
    items = _items([64 + (i % 16 if i < 16 else 0) for i in range(sum(counts))], seed=7)
    starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    buf, off = pyoracle.encode_blocks(items, starts, restart_interval=32, hash_ratio=1.33)
    hw = [_trailer(buf, off, b)[1] for b in range(4)]
    assert hw[0] == 4096 and hw[1] == 4097 and hw[2] >= 8193, hw
    assert all(_need(buf, off, b) > IMG_BIG for b in range(4))
    _both_alignments(off, range(4))
    _check(gpu, items, starts, (buf, off), ri=32, ratio=1.33, pool=pool)


# ------------------------------------------------------------------ listed index blocks
def test_listed_index_blocks(gpu):
    """Index blocks (u64 handles, restart interval 1) of about 30 and about 60 KiB, between small ones."""
    for first in range(100, 164):  # (a first block whose size is a multiple of 16: the second starts aligned)
        counts = [first, 830, 1, 1650, 835, 7]
        items = index_items(sum(counts), seed=13)
        starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
        buf, off = pyoracle.encode_blocks(items, starts, block_type=1)
        if int(off[1]) % 16 == 0:
            break
    sizes = np.diff(off.astype(np.int64))
    assert 28 * KIB < sizes[1] < 32 * KIB and 56 * KIB < sizes[3] < 64 * KIB, sizes
    listed = [b for b in range(len(counts)) if sizes[b] > GROUP_IMG]
    assert listed == [1, 3, 4] and all(IMG_MEDIUM < _need(buf, off, b) <= IMG_BIG for b in listed)
    _both_alignments(off, listed)
    _check(gpu, items, starts, (buf, off), ri=1, block_type=1)


# ------------------------------------------------------------------ overflow per class
@functools.lru_cache(maxsize=None)
def _overflow_batch():
    """A group-class, a medium, a big and two huge blocks; the medium one starts 16-byte aligned."""
    counts = [40, 40, 160, 300, 300]
    for pad in range(16):
        vlens = [64 + pad if i == 0 else 64 for i in range(40)] + [400] * 40 + [400] * 160 + [450] * 600
        items = _items(vlens, seed=9)
        starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
        buf, off = pyoracle.encode_blocks(items, starts, restart_interval=16, hash_ratio=1.33)
        if int(off[1]) % 16 == 0:
            break
    sizes = np.diff(off.astype(np.int64))
    need = [_need(buf, off, b) for b in range(5)]
    assert sizes[0] + 15 <= GROUP_IMG and GROUP_IMG < sizes[1] and need[1] <= IMG_MEDIUM, (sizes, need)
    assert IMG_MEDIUM < need[2] <= IMG_BIG and need[3] > IMG_BIG and need[4] > IMG_BIG, need
    _both_alignments(off, range(1, 5))
    return items, starts, buf, off


@pytest.mark.parametrize("pool", [True, False])
@pytest.mark.parametrize("cut", [1, 2, 3, 4])
def test_overflow_per_class(gpu, cut, pool):
    """out_cap in the middle of block `cut`: the blocks that end at or before it are written, the
    others report OVERFLOW, block_off is complete, and no byte at or past out_cap is touched."""
    import torch
    items, starts, ref_buf, ref_off = _overflow_batch()
    nb = len(starts) - 1
    out_cap = (int(ref_off[cut]) + int(ref_off[cut + 1])) // 2
    d = gpu.items_to_device(items)
    d_starts = torch.from_numpy(starts.astype(np.int32)).cuda()
    it = gpu.LsmItems()
    it.keys, it.key_off, it.vals, it.val_off = (d[k].data_ptr() for k in ("keys", "key_off", "vals", "val_off"))
    it.seqno, it.vtype = d["seqno"].data_ptr(), d["vtype"].data_ptr()
    it.handle_off, it.handle_size = d["handle_off"].data_ptr(), d["handle_size"].data_ptr()
    it.n_items = items.n
    params = gpu.LsmBlockParams(16, gpu.BLOCK_DATA, 0, 0, 1.33, gpu.ENCODE_HUGE_POOL if pool else 0)
    lib = gpu.lib()
    bound = lib.lsm_encode_bound(items.n, nb, int(d["keys"].numel()), int(d["vals"].numel()), C.byref(params))
    assert bound >= int(ref_off[-1])
    need = lib.lsm_encode_workspace_size_ex(items.n, nb, bound) if pool else lib.lsm_encode_workspace_size(items.n, nb)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    buf = torch.full((bound + gpu.LSM_INPUT_PADDING,), MARKER, dtype=torch.uint8, device="cuda")
    block_off = torch.zeros(nb + 1, dtype=torch.int64, device="cuda")
    status = torch.full((nb,), -1, dtype=torch.int32, device="cuda")
    rc = lib.lsm_encode_blocks(C.byref(it), C.c_void_p(d_starts.data_ptr()), nb, C.byref(params),
                               C.c_void_p(buf.data_ptr()), out_cap, C.c_void_p(block_off.data_ptr()),
                               C.c_void_p(status.data_ptr()), C.c_void_p(ws.data_ptr()), need, None)
    torch.cuda.synchronize()
    assert rc == 0
    off = block_off.cpu().numpy().view(np.uint64)
    st = status.cpu().numpy()
    got = buf.cpu().numpy()
    assert (off == ref_off).all()
    assert list(st) == [OK] * cut + [OVERFLOW] * (nb - cut), st
    end = int(ref_off[cut])
    assert got[:end].tobytes() == ref_buf[:end].tobytes()
    assert (got[out_cap:] == MARKER).all()
