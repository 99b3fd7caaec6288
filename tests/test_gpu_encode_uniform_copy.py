"""The group kernel's value copy (csrc/encode_group.hpp lds_copy_uniform + lds_copy): the
interior dwords that every value-carrying lane of a wave has are copied in a loop with
a wave-uniform trip count B (the wave-wide minimum), the head bytes, each lane's surplus
dwords and the tail bytes by the general loop; under kUniformMin = 4 dwords, or with no
value in the wave, the general loop alone.  The bytes must not depend on which ran.

Every case is encoded through lsm_encode_blocks32 and lsm_encode_blocks and compared bit
for bit (block_off, bytes, status 0) with the oracle (DataBlock::encode_into +
Block::write_into, src/table/data_block/mod.rs:523-549, src/table/block/mod.rs:45-84):
equal lengths around every threshold of the loop (B = 0, B < 4, B not a multiple of the
unroll, the remainder loop) at every source and destination alignment, mixed waves
(tombstones, an odd length, an empty value, a short last block), nearly equal and widely
different lengths, the split writer (2 and 4 threads per item), the hash-index
instantiations and the fused plan."""
import random

import numpy as np
import pytest

import pyoracle
from helpers import counter_items, prefix_items, random_sorted_items

pytestmark = pytest.mark.gpu

PER = 52  # items per 4 KiB block of 16 B keys / 64 B values


def _encode(gpu, items, starts, off32, ri=16, ratio=0.0, run_plan=False):
    import torch
    d_items = gpu.items_to_device(items, off32=off32)
    assert d_items["key_off"].element_size() == (4 if off32 else 8)
    d_starts = torch.from_numpy(np.asarray(starts, np.int64).astype(np.int32)).cuda()
    kw = dict(pool=False, run_plan=True) if run_plan else {}
    out = gpu.Encoder().encode(d_items, d_starts, len(starts) - 1, restart_interval=ri, hash_ratio=ratio, **kw)
    torch.cuda.synchronize()
    off = out["block_off"].cpu().numpy().view(np.uint64)
    return out["buf"].cpu().numpy()[:int(off[-1])].tobytes(), off, out["status"].cpu().numpy()[:len(starts) - 1]


def _check(gpu, items, starts, ref=None, **kw):
    ref_buf, ref_off = ref or pyoracle.encode_blocks(items, starts, restart_interval=kw.get("ri", 16),
                                                      hash_ratio=kw.get("ratio", 0.0))
    for off32 in (True, False):
        buf, off, st = _encode(gpu, items, starts, off32, **kw)
        assert (st == 0).all(), (off32, st)
        assert (off == ref_off).all(), off32
        assert buf == ref_buf.tobytes(), off32


def _with_lengths(vlens, vtype=None, seed=1, shift=0, seqno=None):
    """Counter keys of 16 B; item i has a random value of vlens[i] bytes (tombstones: none).
    shift: the value arena starts `shift` bytes into its buffer (val_off[0] = shift);
    seqno: per-item sequence numbers (default: 63 for all, one varint byte)."""
    n = len(vlens)
    base = counter_items(n, val_len=0, seed=seed)
    vtype = np.zeros(n, np.uint8) if vtype is None else np.asarray(vtype, np.uint8)
    vlens = np.where((vtype == 1) | (vtype == 2), 0, np.asarray(vlens)).astype(np.uint64)
    rng = np.random.default_rng(seed + 100)
    vals = rng.integers(0, 256, int(vlens.sum()) + shift, dtype=np.uint8)
    val_off = (np.concatenate([[0], np.cumsum(vlens)]) + shift).astype(np.uint64)
    return pyoracle.Items(base.keys, base.key_off, vals, val_off, base.seqno if seqno is None else seqno, vtype)


def _starts(n, per):
    return np.array(list(range(0, n, per)) + [n], np.uint32)


@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 5, 7, 8, 11, 12, 13, 15, 16, 17, 19, 20, 63, 64, 65, 127, 128, 255, 256])
def test_equal_lengths(gpu, n):
    """Every value n bytes: the interior is n / 4 dwords or one fewer, by the destination
    alignment, so B runs over 0, under the threshold, one unrolled step, steps plus a
    remainder; lanes with one dword more than B finish it in the general loop."""
    items = _with_lengths(np.full(PER * 8, n), seed=n + 1)
    _check(gpu, items, _starts(items.n, PER))


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_equal_lengths_64_alignments(gpu, shift):
    """64 B values with the value arena 0..3 bytes into its buffer (every source alignment).
    With one sequence number the records are all 70 bytes and the values' places in the
    payload only even, so every third item has a two-byte sequence number: the places take
    every residue mod 4 (checked on the oracle's own decode, so the case cannot lose its
    destination alignments unnoticed)."""
    seqno = np.where(np.arange(PER * 8) % 3 == 0, 300, 63)
    items = _with_lengths(np.full(PER * 8, 64), seed=70 + shift, shift=shift, seqno=seqno)
    starts = _starts(items.n, PER)
    ref = pyoracle.encode_blocks(items, starts)
    parsed, item_start, status = pyoracle.decode_blocks(ref[0], ref[1], nthreads=2)
    assert (status == 0).all() and int(item_start[-1]) == items.n
    assert (parsed["val_len"][:items.n] == 64).all()
    assert set((parsed["val_off"][:items.n].astype(np.int64) % 4).tolist()) == {0, 1, 2, 3}
    _check(gpu, items, starts, ref=ref)


def test_mixed_waves(gpu):
    """64 B values with 5 % tombstones, one item in the middle of a wave with another length,
    one empty value of type Value, and a short last block (the last group's item count is
    no multiple of 64)."""
    n = PER * 12 + 37
    rng = np.random.default_rng(8)
    vtype = (rng.random(n) < 0.05).astype(np.uint8)
    vlens = np.full(n, 64)
    for i, v in ((30, 23), (64 + 31, 0), (PER * 6 + 20, 131)):
        vtype[i] = 0
        vlens[i] = v
    assert 0 < int(vtype.sum()) < n // 8
    items = _with_lengths(vlens, vtype, seed=21)
    _check(gpu, items, _starts(n, PER))
    # the generator of the large-batch tests, as it is
    items = counter_items(PER * 9 + 11, seed=6, tomb_frac=0.05)
    _check(gpu, items, _starts(items.n, PER))


def test_nearly_equal_lengths(gpu):
    """Lengths 60..68: B is a true minimum and lanes finish 0..2 surplus dwords."""
    n = 50 * 10
    vlens = np.random.default_rng(12).integers(60, 69, n)
    assert set(vlens.tolist()) == set(range(60, 69))
    _check(gpu, _with_lengths(vlens, seed=22), _starts(n, 50))


def test_widely_different_lengths(gpu):
    """Values of 0..120 bytes, every value type, blocks of 1..120 items: the fast path is
    mostly refused (B under the threshold)."""
    items = random_sorted_items(3000, seed=41, vmax=120)
    rng = random.Random(9)
    starts = [0]
    while starts[-1] < items.n:
        starts.append(min(items.n, starts[-1] + rng.randint(1, 120)))
    _check(gpu, items, np.array(starts, np.uint32), ri=5)


def test_split_writer(gpu):
    """Groups of few items, where 4 or 2 threads split an item's value copy: 16 KiB blocks of
    56 items (40 B prefix keys, 256 B values), and 100-item blocks of 128 B values."""
    items = prefix_items(56 * 8)
    _check(gpu, items, _starts(items.n, 56))
    items = counter_items(100 * 6, val_len=128, seed=13)
    _check(gpu, items, _starts(items.n, 100))
    # parts of unequal and of zero length (values shorter than the threads that share them)
    vlens = np.random.default_rng(3).integers(0, 300, 50 * 4)
    _check(gpu, _with_lengths(vlens, seed=23), _starts(len(vlens), 50))


@pytest.mark.parametrize("key_len", [16, 24])
def test_hash_index(gpu, key_len):
    """Hash ratio 1.33 with 64 B values: buckets from the plan pass (16 B keys) and hashed in
    the group kernel (24 B keys)."""
    items = counter_items(PER * 8, key_len=key_len, seed=17)
    _check(gpu, items, _starts(items.n, PER if key_len == 16 else 47), ratio=1.33)


def test_fused_plan(gpu):
    """The run-level plan fused into the group kernel, eight 205-item blocks of 64 B values."""
    items = counter_items(205 * 8, seed=19)
    _check(gpu, items, _starts(items.n, 205), run_plan=True)
