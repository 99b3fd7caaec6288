"""CPU checks of the device block cut's ground: the closed-form chain of
lsm_cut_blocks_device (tests/cut_model.py) equals the writer's loop (lsm_cut_blocks and the
oracle's orc_cut_blocks) on random offsets; the new entry points exist; and their argument
errors are reported before any device work."""
import ctypes as C
import random

import numpy as np
import pytest

import cut_model as CM


@pytest.fixture(scope="module")
def L():
    import lsmgpu
    if not lsmgpu.LIB_PATH.exists():
        lsmgpu.build()
    return lsmgpu


def _offsets(rng, n, wmax, base=0, zero_share=0.0):
    w = [0 if rng.random() < zero_share else rng.randint(0, wmax) for _ in range(n)]
    return np.concatenate([[base], base + np.cumsum(w, dtype=np.uint64)]).astype(np.uint64)


CASES = [  # (n, key wmax, val wmax, block_size, key base, val base, share of zero weights)
    (0, 1, 1, 64, 0, 0, 0.0), (1, 40, 300, 64, 0, 0, 0.0), (1, 40, 300, 1 << 20, 0, 0, 0.0),
    (200, 40, 300, 0, 0, 0, 0.0), (200, 40, 300, 1, 0, 0, 0.3), (200, 0, 0, 0, 0, 0, 1.0),
    (200, 0, 0, 1, 0, 0, 1.0), (300, 40, 300, 512, 0, 0, 0.5), (300, 40, 300, 4096, 7, 0, 0.0),
    (300, 40, 300, 4096, 12345, 99, 0.1), (300, 1 << 31, 1 << 31, 0xFFFFFFFF, 1 << 40, 1 << 41, 0.0),
    (300, 1 << 20, 1 << 31, 1 << 30, (1 << 40) + 3, 1 << 50, 0.2), (257, 1, 0, 33, 0, 0, 0.0),
]


@pytest.mark.parametrize("case", CASES)
def test_chain_equals_the_host_loop(L, oracle, case):
    n, kw, vw, bs, kb, vb, zs = case
    rng = random.Random(hash(case) & 0xFFFF)
    for _ in range(5):
        ko, vo = _offsets(rng, n, kw, kb, zs), _offsets(rng, n, vw, vb, zs)
        want = [int(x) for x in L.cut_blocks(ko, vo, bs)]
        assert CM.loop_cut(ko, vo, bs) == want
        assert CM.chain_cut(ko, vo, bs) == want
        for tile in (1, 4, 64):
            assert CM.tiled_cut(ko, vo, bs, tile=tile) == want
        if kb == 0 and vb == 0 and n:  # the oracle's Items start both offset arrays at 0
            it = oracle.Items(np.zeros(int(ko[-1]) if ko[-1] < 1 << 24 else 0, np.uint8), ko,
                              np.zeros(0, np.uint8), vo, np.zeros(n, np.uint64), np.zeros(n, np.uint8))
            assert [int(x) for x in oracle.cut_blocks(it, bs)] == want


@pytest.mark.parametrize("extra,bs", [(48, 256), (48, 0), (1, 1), (7, 100), (0xFFFFFFFF, 0xFFFFFFFF)])
def test_chain_with_extra_and_no_values(extra, bs):
    rng = random.Random(extra * 31 + bs)
    for n in (0, 1, 2, 90, 333):
        ko = _offsets(rng, n, 40, rng.choice((0, 5, 1 << 40)), 0.2)
        want = CM.loop_cut(ko, None, bs, extra)
        assert CM.chain_cut(ko, None, bs, extra) == want
        assert CM.tiled_cut(ko, None, bs, extra, tile=16) == want
        vo = _offsets(rng, n, 300)
        assert CM.chain_cut(ko, vo, bs, extra) == CM.loop_cut(ko, vo, bs, extra)


def test_partition_rule_is_the_oracles():
    """extra = 48 with no values is the partition cut of pyoracle.table_write: buffered size per
    handle = end key length + 48, a partition cut once it reaches partition_size."""
    rng = random.Random(3)
    ko = _offsets(rng, 120, 40)
    starts, size = [0], 0
    for i in range(120):
        size += int(ko[i + 1] - ko[i]) + 48
        if size >= 256:
            starts.append(i + 1)
            size = 0
    if starts[-1] != 120:
        starts.append(120)
    assert CM.chain_cut(ko, None, 256, 48) == starts


def test_new_symbols_exist(L):
    lib = L.lib()
    for f in ("lsm_cut_workspace_size", "lsm_cut_blocks_device", "lsm_index_entries_workspace_size",
              "lsm_index_entries"):
        assert hasattr(lib, f) and f in L.EXPORTED_SYMBOLS
    assert L.CUT_TILE_ITEMS == 16384
    assert lib.lsm_cut_workspace_size(0) > 0
    assert lib.lsm_cut_workspace_size(1) <= lib.lsm_cut_workspace_size(3 * L.CUT_TILE_ITEMS + 5)
    assert lib.lsm_cut_workspace_size(1 << 20) >= 8 << 20
    assert lib.lsm_index_entries_workspace_size(0) > 0
    assert lib.lsm_index_entries_workspace_size(1 << 20) >= 4 << 20


def test_cut_bad_args_rejected_without_device(L):
    lib = L.lib()
    p = [C.c_void_p(0x1000 * (i + 1)) for i in range(6)]
    ws = lib.lsm_cut_workspace_size(100)

    def call(key_off=p[0], val_off=p[1], n=100, d_n=None, starts=p[2], cap=100, nb=p[3], st=p[4], w=p[5], wb=ws):
        return lib.lsm_cut_blocks_device(key_off, val_off, n, d_n, 0, 4096, starts, cap, nb, st, w, wb, None)

    assert call(key_off=None) == 10
    assert call(starts=None) == 10
    assert call(nb=None) == 10
    assert call(st=None) == 10
    assert call(w=None) == 10
    assert call(n=0xFFFFFFFF, wb=1 << 62) == 10  # more than 2^32 - 2 items
    assert call(n=1 << 40, wb=1 << 62) == 10
    assert call(cap=0) == 10                     # no room for a block, with items
    assert call(wb=ws - 1) == 10                 # short workspace
    assert call(wb=0) == 10


def test_index_entries_bad_args_rejected_without_device(L):
    lib = L.lib()
    p = [C.c_void_p(0x1000 * (i + 1)) for i in range(12)]
    it = L.LsmItems()
    it.keys, it.key_off, it.seqno, it.n_items = 0x100000, 0x200000, 0x300000, 50
    ws = lib.lsm_index_entries_workspace_size(7)
    args = [C.byref(it), p[0], p[1], 7, 0, p[2], 100, p[3], p[4], p[5], p[6], p[7], p[8], ws, None]
    for i in (0, 1, 2, 5, 7, 8, 9, 10, 11, 12):  # every pointer
        a = list(args)
        a[i] = None
        assert lib.lsm_index_entries(*a) == 10, i
    a = list(args)
    a[13] = ws - 1
    assert lib.lsm_index_entries(*a) == 10
    for f in ("keys", "key_off", "seqno"):
        bad = L.LsmItems()
        bad.keys, bad.key_off, bad.seqno, bad.n_items = 0x100000, 0x200000, 0x300000, 50
        setattr(bad, f, None)
        a = list(args)
        a[0] = C.byref(bad)
        assert lib.lsm_index_entries(*a) == 10, f
