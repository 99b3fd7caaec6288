"""Deferred scramble chains, checksum tails and headers in the group kernel's wave-per-block
loop (csrc/encode_group.hpp, flush_headers): a wave stores a block's payload at block time and no
header byte; it keeps the block's 40 contribution words in registers (or, in lane quad j,
the finished digest of a payload of <= 240 B), and after every kWDefer = 4 of its blocks,
or its last one of the run, quad j runs the j-th kept block's chain, merge, avalanche and
header checksum and writes the 33 header bytes straight to the output.

Every batch goes through lsm_encode_blocks32 and lsm_encode_blocks into a buffer filled
with a canary and is compared bit for bit (block_off, bytes, status 0, canary past the end)
with the oracle (DataBlock::encode_into + Block::write_into); and through the diagnostic
build with and without lsm_block_params.reserved bit 0x20 (every run takes the group
loop), for the two loops on one input.  A block's payload length is set exactly by sizing
its last value from the oracle's own offsets.  Batches are at most 3 runs of 32 blocks."""
import ctypes as C
import functools

import numpy as np
import pytest

import pyoracle
from helpers import counter_items

pytestmark = pytest.mark.gpu

PER = 52    # items per 4 KiB block of 16 B keys / 64 B values
RUN = 32    # kGRun: blocks per workgroup
WAVES = 4   # kGWaves: wave w takes blocks w, w + 4, ... of a run
HDR = 33    # block header bytes
# csrc/encode_group.hpp, mirrored (wave_fits): n <= 64 items, span + 15 <= limit for the key span,
# the value span and the encoded size, each counted from the 16-B boundary at or before its start
W_ITEMS, W_KEYS, W_VALS, W_IMG = 64, 1024, 4096, 4496
DIAG_NO_WAVE_BLOCKS = 0x20
CANARY = 0xA5


def _encode(gpu, items, starts, off32, reserved=0, lib=None, out_cap=None):
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
    params = gpu.LsmBlockParams(16, 0, 0, reserved, 0.0, 0)
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


# ------------------------------------------------------------------ batches
def _items(vlens, seed):
    """Counter keys of 16 B, sequence number 63; item i has a random value of vlens[i] bytes."""
    base = counter_items(len(vlens), val_len=0, seed=seed)
    vlens = np.asarray(vlens).astype(np.uint64)
    vals = np.random.default_rng(seed + 100).integers(0, 256, int(vlens.sum()), dtype=np.uint8)
    val_off = np.concatenate([[0], np.cumsum(vlens)]).astype(np.uint64)
    return pyoracle.Items(base.keys, base.key_off, vals, val_off, base.seqno, base.vtype)


def _plens(ref_off):
    return np.diff(ref_off.astype(np.int64)) - HDR


def _sized(blocks, seed):
    """blocks: (items, value length, payload length or None) per block.  The last value of a
    block with a payload length is sized, from the oracle's own offsets, until the block's
    payload has exactly that length.  Returns items, starts and the oracle's encoding."""
    sizes = [b[0] for b in blocks]
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    vlens = np.concatenate([np.full(n, v, np.int64) for n, v, _ in blocks])
    want = np.array([-1 if t is None else t for _, _, t in blocks], np.int64)
    for _ in range(6):  # (a length's varint can change size on the way: a few rounds)
        items = _items(vlens, seed)
        ref = pyoracle.encode_blocks(items, starts, restart_interval=16)
        delta = np.where(want >= 0, want - _plens(ref[1]), 0)
        if not delta.any():
            break
        vlens[starts[1:].astype(np.int64) - 1] += delta
        assert (vlens >= 0).all()
    got = _plens(ref[1])
    assert (got[want >= 0] == want[want >= 0]).all()
    return items, starts, ref


def _assert_wave_loop(items, starts, ref_off):
    """Every block passes wave_fits, so every run of the batch takes the wave-per-block loop."""
    s = starts.astype(np.int64)
    ko, vo, oo = (a.astype(np.int64) for a in (items.key_off, items.val_off, ref_off))
    assert (np.diff(s) >= 1).all() and (np.diff(s) <= W_ITEMS).all()
    assert (ko[s[1:]] - (ko[s[:-1]] & ~15) + 15 <= W_KEYS).all()
    assert (vo[s[1:]] - (vo[s[:-1]] & ~15) + 15 <= W_VALS).all()
    assert (oo[1:] - (oo[:-1] & ~15) + 15 <= W_IMG).all()


def _quad_slots(nb):
    items = counter_items(PER * nb, seed=100 + nb)
    starts = np.array(list(range(0, items.n, PER)) + [items.n], np.uint32)
    return items, starts, pyoracle.encode_blocks(items, starts, restart_interval=16)


def _short_and_long():
    """One run: blocks of 1 and 2 items with payloads of 240 B and below, and of 241 B,
    alternate with full 4 KiB blocks so that every wave holds both kinds in both orders."""
    tiny = [240, 241, 239, 241, 120, 240, 64, 241]
    blocks, kinds = [], []
    for p in range(RUN):
        small = (p // WAVES + p % WAVES) % 2 == 0
        kinds.append(small)
        if small:
            k = len([x for x in kinds if x]) - 1
            blocks.append((1 + k % 2, 30, tiny[k % len(tiny)]))
        else:
            blocks.append((PER, 64, None))
    items, starts, ref = _sized(blocks, seed=51)
    plen = _plens(ref[1])
    assert 240 in plen and 241 in plen and (plen[np.array(kinds)] <= 241).all() and (plen[~np.array(kinds)] > 3000).all()
    for w in range(WAVES):
        mine = [kinds[p] for p in range(w, RUN, WAVES)]
        pairs = set(zip(mine, mine[1:]))
        assert (True, False) in pairs and (False, True) in pairs, w
    return items, starts, ref


def _unit_counts():
    """One run whose payloads sit at and around 1024, 2048, 3072 and 4096 B: the lane quads of
    one flush hold blocks with different numbers of full KiB units, (plen - 1) / 1024."""
    targets = [1024, 2049, 4097, 1025, 3073, 2048, 4096, 3072, 1023, 4095, 2047, 3071]
    blocks = []
    for p in range(RUN):
        t = targets[(p // WAVES + 3 * (p % WAVES)) % len(targets)]
        blocks.append((8, (t - 230) // 8, t))
    items, starts, ref = _sized(blocks, seed=52)
    nbk = (_plens(ref[1]) - 1) // 1024
    assert set(nbk.tolist()) == {0, 1, 2, 3, 4}
    groups = [nbk[w::WAVES][g:g + 4].tolist() for w in range(WAVES) for g in (0, 4)]  # the blocks of one flush
    for w in range(WAVES):
        assert len(set(nbk[w::WAVES].tolist())) >= 4, w
    assert all(len(set(g)) >= 2 for g in groups) and any(len(set(g)) == 4 for g in groups)
    return items, starts, ref


def _alignments():
    """Two runs in which the blocks start at every residue mod 16 of the output, and blocks
    of 240 B and below follow and precede full ones: a deferred header's neighbouring bytes
    belong to another wave's block."""
    blocks, kinds = [], []
    for p in range(2 * RUN):
        small = p % 3 == 1 or p % 7 == 3
        kinds.append(small)
        blocks.append((1 + p % 2, 20 + (5 * p) % 23, None) if small else (PER, 57 + (11 * p) % 16, None))
    items, starts, ref = _sized(blocks, seed=53)
    assert set((ref[1][:-1] % np.uint64(16)).tolist()) == set(range(16))
    plen = _plens(ref[1])
    k = np.array(kinds)
    assert (plen[k] <= 240).all() and (plen[~k] > 3000).all()
    pairs = set(zip(kinds, kinds[1:]))
    assert (True, False) in pairs and (False, True) in pairs
    return items, starts, ref


QUAD_SLOTS = [8, 9, 12, 16, 29, 31, 32, 35]
NAMES = [f"quad_slots_{nb}" for nb in QUAD_SLOTS] + ["short_and_long", "unit_counts", "alignments"]


@functools.lru_cache(maxsize=None)
def _batch(name):
    """items, starts and the oracle's (bytes, block_off): built once, shared by the tests."""
    if name.startswith("quad_slots_"):
        items, starts, ref = _quad_slots(int(name.rsplit("_", 1)[1]))
    else:
        items, starts, ref = {"short_and_long": _short_and_long, "unit_counts": _unit_counts,
                              "alignments": _alignments}[name]()
    assert len(starts) - 1 <= 3 * RUN
    _assert_wave_loop(items, starts, ref[1])
    for a in ref:
        a.setflags(write=False)
    return items, starts, ref


# -------------------------------------------------------------------- tests
@pytest.mark.parametrize("name", NAMES)
def test_matches_the_oracle(gpu, name):
    """quad_slots_*: 52-item blocks; the waves of a run hold 2, 3, 7 or 8 blocks, unequal
    counts across the four waves, and in the last run some waves hold none."""
    items, starts, (ref_buf, ref_off) = _batch(name)
    for off32 in (True, False):
        buf, off, st = _encode(gpu, items, starts, off32)
        assert (st == 0).all(), (off32, np.flatnonzero(st)[:10], st[st != 0][:10])
        assert (off == ref_off).all(), off32
        assert buf[:int(off[-1])].tobytes() == ref_buf.tobytes(), off32
        assert (buf[int(off[-1]):] == CANARY).all(), off32


@pytest.mark.parametrize("name", NAMES)
def test_both_loops_agree(gpu, diag_lib, name):
    """The diagnostic build with the bit set (group loop), the diagnostic build without it
    and the release build give identical bytes, offsets and statuses."""
    items, starts, _ = _batch(name)
    for off32 in (True, False):
        a = _encode(gpu, items, starts, off32, lib=diag_lib, reserved=DIAG_NO_WAVE_BLOCKS)
        b = _encode(gpu, items, starts, off32, lib=diag_lib)
        c = _encode(gpu, items, starts, off32)
        for x in (b, c):
            assert (x[2] == a[2]).all() and (x[1] == a[1]).all() and x[0].tobytes() == a[0].tobytes()
        assert (a[2] == 0).all()


@pytest.mark.parametrize("name", ["quad_slots_35", "alignments"])
def test_capacity_exactly_the_end(gpu, name):
    """out_cap equal to the batch's end: every run still takes the wave loop (each block ends
    at or before out_cap), and nothing is written past the end."""
    items, starts, (ref_buf, ref_off) = _batch(name)
    end = int(ref_off[-1])
    for off32 in (True, False):
        buf, off, st = _encode(gpu, items, starts, off32, out_cap=end)
        assert (st == 0).all() and (off == ref_off).all()
        assert buf[:end].tobytes() == ref_buf.tobytes()
        assert (buf[end:] == CANARY).all()


def test_capacity_cut_inside_the_last_run(gpu, diag_lib):
    """out_cap cuts through block 33 of 35, in the last run (which then takes the group loop
    while the first run's headers are deferred): statuses and every byte equal those of the
    diagnostic build with the wave loop disabled, and nothing is written at or past out_cap."""
    items, starts, (ref_buf, ref_off) = _batch("quad_slots_35")
    cap = int(ref_off[33]) + 100
    assert int(ref_off[RUN]) < int(ref_off[33]) < cap < int(ref_off[34])
    for off32 in (True, False):
        buf, off, st = _encode(gpu, items, starts, off32, out_cap=cap)
        gbuf, goff, gst = _encode(gpu, items, starts, off32, out_cap=cap, lib=diag_lib, reserved=DIAG_NO_WAVE_BLOCKS)
        assert (st == gst).all() and (off == goff).all()
        assert (st[:33] == 0).all() and (st[33:] != 0).all(), st
        assert buf.tobytes() == gbuf.tobytes()
        assert buf[:int(ref_off[33])].tobytes() == ref_buf[:int(ref_off[33])].tobytes()
        assert (buf[cap:] == CANARY).all()
