"""The group kernel's wave-per-block loop (csrc/encode_group.hpp, encode_group_kernel without a
hash index or the fused plan): a 32-block run whose every block is group-class, has at most
64 items, fits a wave slot (wave_fits: kWKeys / kWVals / kWImg) and ends at or before
out_cap is written one wave per block, wave w taking blocks w, w + 4, ... of the run, with
no workgroup barrier; every other run takes the group loop.  The bytes must not depend on
which loop ran.

Every case is encoded through lsm_encode_blocks32 and lsm_encode_blocks and compared bit
for bit (block_off, bytes, status 0) with the oracle (DataBlock::encode_into +
Block::write_into, src/table/data_block/mod.rs:523-549, src/table/block/mod.rs:45-84).
The diagnostic build's lsm_block_params.reserved bit 0x20 (kDiagNoWaveBlocks) makes every
run take the group loop, for the comparisons of the two loops on one input."""
import ctypes as C
import random

import numpy as np
import pytest

import pyoracle
from helpers import counter_items, prefix_items, random_sorted_items

pytestmark = pytest.mark.gpu

PER = 52   # items per 4 KiB block of 16 B keys / 64 B values
RUN = 32   # kGRun: blocks per workgroup
# csrc/encode_group.hpp, mirrored: a block takes the wave loop with n <= 64 items and
# span + 15 <= limit for its key span, value span and encoded size, each span counted
# from the 16-B boundary at or before its start (wave_fits)
W_ITEMS, W_KEYS, W_VALS, W_IMG = 64, 1024, 4096, 4496
DIAG_NO_WAVE_BLOCKS = 0x20
CANARY = 0xA5


def _encode(gpu, items, starts, off32, ri=16, reserved=0, lib=None, out_cap=None):
    """Straight through the C ABI (no flags).  The output buffer starts filled with CANARY;
    out_cap: the capacity handed to the library (default: lsm_encode_bound)."""
    import torch
    d = gpu.items_to_device(items, off32=off32)
    assert d["key_off"].element_size() == (4 if off32 else 8)
    nb = len(starts) - 1
    d_starts = torch.from_numpy(np.asarray(starts, np.int64).astype(np.int32)).cuda()
    L = lib or gpu.lib()
    it = gpu.LsmItems32() if off32 else gpu.LsmItems()
    it.keys, it.key_off = d["keys"].data_ptr(), d["key_off"].data_ptr()
    it.vals, it.val_off = d["vals"].data_ptr(), d["val_off"].data_ptr()
    it.seqno, it.vtype = d["seqno"].data_ptr(), d["vtype"].data_ptr()
    it.n_items = d["seqno"].numel()
    params = gpu.LsmBlockParams(ri, 0, 0, reserved, 0.0, 0)
    bound = L.lsm_encode_bound(it.n_items, nb, d["keys"].numel(), d["vals"].numel(), C.byref(params))
    need = L.lsm_encode_workspace_size(it.n_items, nb)
    ws = torch.zeros(max(need, 256), dtype=torch.uint8, device="cuda")
    buf = torch.full((bound + gpu.LSM_INPUT_PADDING,), CANARY, dtype=torch.uint8, device="cuda")
    off = torch.zeros(nb + 1, dtype=torch.int64, device="cuda")
    st = torch.full((max(nb, 1),), -1, dtype=torch.int32, device="cuda")
    fn = L.lsm_encode_blocks32 if off32 else L.lsm_encode_blocks
    rc = fn(C.byref(it), C.c_void_p(d_starts.data_ptr()), nb, C.byref(params), C.c_void_p(buf.data_ptr()),
            bound if out_cap is None else out_cap, C.c_void_p(off.data_ptr()), C.c_void_p(st.data_ptr()),
            C.c_void_p(ws.data_ptr()), need, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return buf.cpu().numpy(), off.cpu().numpy().view(np.uint64), st.cpu().numpy()[:nb]


def _check(gpu, items, starts, ref=None, ri=16):
    ref_buf, ref_off = ref or pyoracle.encode_blocks(items, starts, restart_interval=ri)
    for off32 in (True, False):
        buf, off, st = _encode(gpu, items, starts, off32, ri=ri)
        assert (st == 0).all(), (off32, np.flatnonzero(st)[:10], st[st != 0][:10])
        assert (off == ref_off).all(), off32
        assert buf[:int(off[-1])].tobytes() == ref_buf.tobytes(), off32
        assert (buf[int(off[-1]):] == CANARY).all(), off32


def _with_lengths(vlens, vtype=None, seed=1, shift=0, seqno=None, keys=None):
    """Counter keys of 16 B (or the key arena and offsets of `keys`); item i has a random
    value of vlens[i] bytes.  shift: the value arena starts `shift` bytes into its buffer;
    seqno: per-item sequence numbers (default: 63 for all, one varint byte).  A tombstone
    keeps its vlens[i] bytes of the arena, which no record holds."""
    n = len(vlens)
    base = counter_items(n, val_len=0, seed=seed) if keys is None else keys
    vtype = np.zeros(n, np.uint8) if vtype is None else np.asarray(vtype, np.uint8)
    vlens = np.asarray(vlens).astype(np.uint64)
    rng = np.random.default_rng(seed + 100)
    vals = rng.integers(0, 256, int(vlens.sum()) + shift, dtype=np.uint8)
    val_off = (np.concatenate([[0], np.cumsum(vlens)]) + shift).astype(np.uint64)
    return pyoracle.Items(base.keys, base.key_off, vals, val_off, base.seqno if seqno is None else seqno, vtype)


def _starts(n, per):
    return np.array(list(range(0, n, per)) + [n], np.uint32)


# ------------------------------------------------------------------ run shapes
@pytest.mark.parametrize("nb", [1, 3, 4, 5, 6, 7, 32, 33, 69])
def test_run_shapes(gpu, nb):
    """52-item blocks of 16 B keys and 64 B values: waves with unequal block counts, a run of
    one block, two and three runs, last runs that are no multiple of 4."""
    items = counter_items(PER * nb, seed=nb)
    _check(gpu, items, _starts(items.n, PER))


# ------------------------------------------------------------ eligibility edges
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_items_per_block(gpu, n):
    """Blocks of 1, 63, 64 and 65 items (20 B values): the last is past one lane per item."""
    items = counter_items(n * 9, val_len=20, seed=n)
    _check(gpu, items, _starts(items.n, n))


def _var_key_items(klens, vlens, vtype=None, seed=5):
    """Keys of klens[i] bytes: a 4-byte big-endian counter, then filler."""
    n = len(klens)
    rng = np.random.default_rng(seed)
    key_off = np.concatenate([[0], np.cumsum(klens)]).astype(np.uint64)
    keys = rng.integers(0, 256, int(key_off[-1]), dtype=np.uint8)
    for i in range(n):
        keys[int(key_off[i]):int(key_off[i]) + 4] = np.frombuffer(int(i).to_bytes(4, "big"), np.uint8)
    base = pyoracle.Items(keys, key_off, np.zeros(0, np.uint8), np.zeros(n + 1, np.uint64),
                          np.full(n, 63, np.uint64), np.zeros(n, np.uint8))
    return _with_lengths(vlens, vtype, seed=seed, keys=base)


@pytest.mark.parametrize("over", [0, 1])
def test_key_span_limit(gpu, over):
    """The batch's first block (key span from offset 0) has W_KEYS - 15 key bytes, or one
    more; the blocks after it are ordinary."""
    first = [20] * 49 + [W_KEYS - 15 - 49 * 20 + over]
    assert sum(first) + 15 == W_KEYS + over and min(first) >= 4
    klens = np.array(first + [16] * (PER * 6))
    items = _var_key_items(klens, np.full(len(klens), 8))
    _check(gpu, items, np.array([0, 50] + list(range(50 + PER, len(klens) + 1, PER)), np.uint32))


@pytest.mark.parametrize("over", [0, 1])
def test_value_span_limit(gpu, over):
    """The first block's values span W_VALS - 15 bytes of the arena, or one more.  (Most of
    them belong to a tombstone, which no record holds: with every value in a record the
    encoded size would pass its own limit first.)"""
    n0 = 50
    vlens = np.full(n0 + PER * 6, 64)
    vtype = np.zeros(len(vlens), np.uint8)
    vlens[:n0] = 24
    vtype[20] = 1
    vlens[20] = W_VALS - 15 - 24 * (n0 - 1) + over
    assert int(vlens[:n0].sum()) + 15 == W_VALS + over
    items = _with_lengths(vlens, vtype, seed=31)
    _check(gpu, items, np.array([0, n0] + list(range(n0 + PER, len(vlens) + 1, PER)), np.uint32))


@pytest.mark.parametrize("over", [0, 1])
def test_encoded_size_limit(gpu, over):
    """The first block (at output offset 0) encodes to W_IMG - 15 bytes, or one more: its
    last value's length is set from the oracle's own size."""
    n0 = 62
    vlens = np.full(n0 + PER * 6, 64)
    starts = np.array([0, n0] + list(range(n0 + PER, len(vlens) + 1, PER)), np.uint32)
    _, off = pyoracle.encode_blocks(_with_lengths(vlens, seed=32), starts)
    vlens[n0 - 1] += W_IMG - 15 + over - int(off[1])
    assert 0 < vlens[n0 - 1] < 128  # (the length's varint stays one byte)
    items = _with_lengths(vlens, seed=32)
    ref = pyoracle.encode_blocks(items, starts)
    assert int(ref[1][1]) + 15 == W_IMG + over
    _check(gpu, items, starts, ref=ref)


def test_oversize_block_in_the_middle_run(gpu):
    """Three runs; only the middle one holds an oversize block (100 items of 128 B values),
    so runs of both kinds sit side by side."""
    sizes = [PER] * 40 + [100] + [PER] * 40
    assert RUN <= 40 < 2 * RUN and len(sizes) > 2 * RUN
    vlens = np.concatenate([np.full(s, 128 if s == 100 else 64) for s in sizes])
    items = _with_lengths(vlens, seed=33)
    _check(gpu, items, np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32))


# ------------------------------------------------------------- record contents
@pytest.mark.parametrize("ri", [1, 2, 5, 16])
def test_restart_intervals(gpu, ri):
    """Restart intervals 1, 2, 5 and 16, with 5 % tombstones and a short last block."""
    items = counter_items(PER * 9 + 11, seed=6 + ri, tomb_frac=0.05)
    assert 0 < int((items.vtype == 1).sum()) < items.n // 8
    _check(gpu, items, _starts(items.n, PER), ri=ri)


def test_empty_values(gpu):
    """Every value empty (type Value): no value bytes in the stage at all."""
    _check(gpu, _with_lengths(np.zeros(PER * 6, np.int64), seed=34), _starts(PER * 6, PER))


def test_widely_different_lengths_and_every_output_alignment(gpu):
    """Values of 0..120 bytes, every value type, blocks of 1..60 items (the uniform copy is
    mostly refused).  The blocks start at every residue mod 16 of the output, which is
    checked on the oracle's own block_off."""
    items = random_sorted_items(3000, seed=41, vmax=120)
    rng = random.Random(9)
    starts = [0]
    while starts[-1] < items.n:
        starts.append(min(items.n, starts[-1] + rng.randint(1, 60)))
    starts = np.array(starts, np.uint32)
    ref = pyoracle.encode_blocks(items, starts, restart_interval=5)
    assert set((ref[1][:-1] % np.uint64(16)).tolist()) == set(range(16))
    _check(gpu, items, starts, ref=ref, ri=5)


def test_nearly_equal_lengths(gpu):
    """Values of 60..68 bytes."""
    n = 50 * 10
    vlens = np.random.default_rng(12).integers(60, 69, n)
    assert set(vlens.tolist()) == set(range(60, 69))
    _check(gpu, _with_lengths(vlens, seed=22), _starts(n, 50))


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_value_alignments(gpu, shift):
    """64 B values with the value arena 0..3 bytes into its buffer, and a two-byte sequence
    number on every third item: the values land on every destination alignment (checked on
    the oracle's own decode)."""
    seqno = np.where(np.arange(PER * 8) % 3 == 0, 300, 63)
    items = _with_lengths(np.full(PER * 8, 64), seed=70 + shift, shift=shift, seqno=seqno)
    starts = _starts(items.n, PER)
    ref = pyoracle.encode_blocks(items, starts)
    parsed, item_start, status = pyoracle.decode_blocks(ref[0], ref[1], nthreads=2)
    assert (status == 0).all() and int(item_start[-1]) == items.n
    assert set((parsed["val_off"][:items.n].astype(np.int64) % 4).tolist()) == {0, 1, 2, 3}
    _check(gpu, items, starts, ref=ref)


def test_prefix_keys(gpu):
    """40 B keys with a 32 B shared prefix, 24 items per block (960 B of keys)."""
    items = prefix_items(24 * 9, val_len=64)
    _check(gpu, items, _starts(items.n, 24))


def _tiny_batch():
    """One-item blocks with an empty value (a header, one record, the marker, a one-entry
    binary index and the trailer: the smallest block there is) among normal blocks."""
    sizes = [PER, 1, 1, PER, 1, PER, PER, 1, 1, 1, PER] * 4
    vlens = np.concatenate([np.full(s, 64 if s == PER else 0) for s in sizes])
    return _with_lengths(vlens, seed=35), np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)


def test_tiny_blocks(gpu):
    items, starts = _tiny_batch()
    ref = pyoracle.encode_blocks(items, starts)
    assert int(np.diff(ref[1].astype(np.int64)).min()) < 96  # (the short checksum path: payloads <= 240 B)
    _check(gpu, items, starts, ref=ref)


# ------------------------------------------------------- capacity, both loops
def test_capacity_cut_inside_a_run(gpu, diag_lib):
    """out_cap cuts through block 40, inside the second run: statuses and every byte below
    the cut equal those of the diagnostic build with the wave loop disabled, and nothing is
    written at or past out_cap."""
    items = counter_items(PER * 69, seed=36)
    starts = _starts(items.n, PER)
    _, ref_off = pyoracle.encode_blocks(items, starts)
    cap = int(ref_off[40]) + 100
    assert int(ref_off[RUN]) < cap < int(ref_off[41])
    for off32 in (True, False):
        buf, off, st = _encode(gpu, items, starts, off32, out_cap=cap)
        gbuf, goff, gst = _encode(gpu, items, starts, off32, out_cap=cap, lib=diag_lib, reserved=DIAG_NO_WAVE_BLOCKS)
        assert (st == gst).all() and (off == goff).all()
        assert (st[:40] == 0).all() and (st[40:] != 0).all(), st
        assert buf[:cap].tobytes() == gbuf[:cap].tobytes()
        assert (buf[cap:] == CANARY).all() and (gbuf[cap:] == CANARY).all()


def _agree_batches():
    yield counter_items(PER * 69, seed=37, tomb_frac=0.05), _starts(PER * 69, PER), 16
    items = random_sorted_items(2000, seed=43, vmax=120)
    rng = random.Random(10)
    starts = [0]
    while starts[-1] < items.n:
        starts.append(min(items.n, starts[-1] + rng.randint(1, 60)))
    yield items, np.array(starts, np.uint32), 5
    yield _tiny_batch() + (16,)


@pytest.mark.parametrize("which", [0, 1, 2])
def test_both_loops_agree(gpu, diag_lib, which):
    """The diagnostic build with the bit set (group loop), the diagnostic build without it
    and the release build give identical bytes, offsets and statuses."""
    items, starts, ri = list(_agree_batches())[which]
    for off32 in (True, False):
        a = _encode(gpu, items, starts, off32, ri=ri, lib=diag_lib, reserved=DIAG_NO_WAVE_BLOCKS)
        b = _encode(gpu, items, starts, off32, ri=ri, lib=diag_lib)
        c = _encode(gpu, items, starts, off32, ri=ri)
        for x in (b, c):
            assert (x[2] == a[2]).all() and (x[1] == a[1]).all() and x[0].tobytes() == a[0].tobytes()
        assert (a[2] == 0).all()
