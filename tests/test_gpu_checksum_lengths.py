"""Payload-length boundaries of every payload-checksum path (csrc/xxh3.hpp and its callers).

The payload's XXH3-128 takes the short path up to 240 bytes and the long path above: KiB
blocks nbk = (plen - 1) / 1024, the tail stripes ((plen - 1) % 1024) / 64 and the last
stripe.  Which kernel hashes a block depends on its class, so every class gets blocks whose
payload length plen (encoded size - 33) sits on those edges:

  wave     the group kernel's wave-per-block loop (every block <= 4496 - 15 B, nbk <= 4):
           240 | 241, the stripe edges after one KiB block, nbk 0 -> 1 .. 3 -> 4, and
           the largest payloads of that loop.
  group    the same blocks with one block of more than 4496 B in each run of 32, which
           sends the whole run through the group loop.
  group4   the group loop's chain reads four contributions per batch: nbk 4 -> 5, 7 -> 8,
           8 -> 9 and 11 -> 12.
  listed   blocks above the group image (the listed-block writer): its chain passes take 64
           contributions each, nbk 63 -> 64 is 65536 | 65537.
  large    blocks above 96 KiB (encode_large_kernel without the workspace pool, the whole-GPU
           path with it; decode_chunked or the parse / hash units).

A block has a few items with 16 B counter keys; one value's length is stepped until the
oracle's own block_off gives the wanted plen.  The CPU test pins that the batches really
hold every listed length.  On the GPU every batch is encoded through lsm_encode_blocks32 and
lsm_encode_blocks (offsets, bytes and status 0 bit-exact against the oracle), the oracle's
bytes are decoded (status 0, equal items), and decoded again with the last payload byte of
every block flipped (every block reports the checksum status)."""
import functools

import numpy as np
import pytest

import pyoracle
from helpers import compare_decode, counter_items, gpu_decode

HDR = 33
RUN = 32                       # kGRun: blocks per workgroup of the group kernel
W_IMG, G_IMG, BIG = 4496, 15872, 96 * 1024   # kWImg (csrc/encode_group.hpp), kGImg, kImgBig (csrc/encode_common.hpp)
ST_CKSUM = 4

WAVE = (list(range(236, 261)) + list(range(1020, 1031)) + list(range(1084, 1095)) +
        [2048, 2049, 3072, 3073, 4096, 4097, 4160, 4161, 4162])
GROUP4 = [5120, 5121, 8192, 8193, 9216, 9217, 12288, 12289]
LISTED = [20480, 65535, 65536, 65537, 65600, 65601]
LARGE = [131072, 131073, 131137]
FILLER = 5000                  # a group-class block that is too large for the wave loop


def _group_targets():
    """WAVE with a FILLER block at the head of every run of RUN blocks."""
    out = []
    for t in WAVE:
        if len(out) % RUN == 0:
            out.append(FILLER)
        out.append(t)
    return out


TARGETS = {"wave": WAVE, "group": _group_targets(), "group4": GROUP4, "listed": LISTED, "large": LARGE}


def _items(vlens, seed):
    n = len(vlens)
    base = counter_items(n, val_len=0, seed=seed)
    vlens = np.asarray(vlens).astype(np.uint64)
    vals = np.random.default_rng(seed + 100).integers(0, 256, int(vlens.sum()), dtype=np.uint8)
    val_off = np.concatenate([[0], np.cumsum(vlens)]).astype(np.uint64)
    return pyoracle.Items(base.keys, base.key_off, vals, val_off, base.seqno, np.zeros(n, np.uint8))


@functools.lru_cache(maxsize=None)
def _batch(name):
    """(items, starts, oracle bytes, oracle block_off) with payload lengths TARGETS[name], in
    order.  Block b has 1 + plen / (fixed + 200) items: its first value is stepped, the others
    have `fixed` bytes (all lengths stay two-byte varints, so one value byte is one payload byte)."""
    targets = np.array(TARGETS[name], np.int64)
    fixed = 3000 if name in ("listed", "large") else 300
    per = 1 + targets // (fixed + 200)
    starts = np.concatenate([[0], np.cumsum(per)]).astype(np.uint32)
    vlens = np.full(int(starts[-1]), fixed, np.int64)
    first = starts[:-1].astype(np.int64)
    vlens[first] = targets - (per - 1) * fixed - 60 - 22 * per
    for _ in range(6):
        assert (vlens[first] >= 128).all() and (vlens < 16384).all()
        items = _items(vlens, seed=len(targets))
        buf, off = pyoracle.encode_blocks(items, starts)
        miss = targets - (np.diff(off.astype(np.int64)) - HDR)
        if not miss.any():
            return items, starts, buf, off
        vlens[first] += miss
    raise AssertionError((name, miss))


def test_batches_hold_every_length():
    """The oracle's own offsets: every listed payload length is there, and every batch's
    blocks are of the class that the batch is for."""
    for name, targets in TARGETS.items():
        items, starts, buf, off = _batch(name)
        total = np.diff(off.astype(np.int64))
        assert (total - HDR).tolist() == list(targets), name
        n = np.diff(starts.astype(np.int64))
        if name == "wave":      # wave_fits: items, key span, value span and size (spans from a 16-B boundary)
            vspan = np.diff(items.val_off.astype(np.int64)[starts])
            assert n.max() <= 64 and 16 * n.max() + 30 <= 1024 and vspan.max() + 30 <= 4096
            assert total.max() + 15 + 15 <= W_IMG
        elif name == "group":   # every run of RUN blocks holds a block that the wave loop refuses
            assert all((total[r:r + RUN] > W_IMG).any() for r in range(0, len(total), RUN))
            assert total.max() + 30 <= G_IMG
        elif name == "group4":
            assert total.min() > W_IMG and total.max() + 30 <= G_IMG
        elif name == "listed":
            assert total.min() > G_IMG and total.max() + 30 <= BIG
        else:
            assert total.min() > BIG + 30
    assert set(WAVE) >= set(range(236, 261)) | set(range(1020, 1031)) | set(range(1084, 1095)) | {
        2048, 2049, 3072, 3073, 4096, 4097, 4160, 4161, 4162}
    assert set(WAVE) <= set(TARGETS["group"]) and FILLER + HDR > W_IMG
    assert sum(int(_batch(k)[3][-1]) for k in TARGETS) < 1_300_000  # about 1 MB in all


def _gpu_encode(gpu, items, starts, off32, pool):
    import torch
    d_items = gpu.items_to_device(items, off32=off32)
    assert d_items["key_off"].element_size() == (4 if off32 else 8)
    d_starts = torch.from_numpy(np.asarray(starts, np.int64).astype(np.int32)).cuda()
    nb = len(starts) - 1
    out = gpu.Encoder().encode(d_items, d_starts, nb, pool=pool)
    torch.cuda.synchronize()
    off = out["block_off"].cpu().numpy().view(np.uint64)
    return out["buf"].cpu().numpy()[:int(off[-1])], off, out["status"].cpu().numpy()[:nb]


@pytest.mark.gpu
@pytest.mark.parametrize("name,pool", [("wave", False), ("group", False), ("group4", False), ("listed", False),
                                       ("listed", True), ("large", False), ("large", True)])
def test_checksum_lengths(gpu, name, pool):
    items, starts, ref_buf, ref_off = _batch(name)
    for off32 in (True, False):
        buf, off, st = _gpu_encode(gpu, items, starts, off32, pool)
        assert (st == 0).all(), (off32, np.flatnonzero(st)[:10], st[st != 0][:10])
        assert (off == ref_off).all(), off32
        bad = np.flatnonzero(buf != ref_buf)
        assert len(bad) == 0, (off32, bad[:10], np.searchsorted(ref_off, bad[:10], side="right") - 1)
    parsed, item_start, status = pyoracle.decode_blocks(ref_buf, ref_off)
    assert (status == 0).all() and int(item_start[-1]) == items.n
    g = gpu_decode(gpu, ref_buf, ref_off, pool=pool)
    assert (g["status"] == 0).all(), g["status"]
    compare_decode(g, parsed, item_start, status)
    flipped = ref_buf.copy()
    flipped[ref_off[1:].astype(np.int64) - 1] ^= 0x01  # the last payload byte of every block
    parsed, item_start, status = pyoracle.decode_blocks(flipped, ref_off)
    assert (status == ST_CKSUM).all(), status
    g = gpu_decode(gpu, flipped, ref_off, pool=pool)
    assert (g["status"] == ST_CKSUM).all(), g["status"]
    compare_decode(g, parsed, item_start, status)
