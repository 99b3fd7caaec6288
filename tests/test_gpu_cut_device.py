"""lsm_cut_blocks_device against the host lsm_cut_blocks (the writer's loop, writer/mod.rs:284-290,374),
or against tests/cut_model.py's loop where extra_per_item is set (the partition rule,
partitioned.rs:166-179).  Only offset arrays are needed.  The sizes come from the kernel's
tile (CUT_TILE_ITEMS = T): one tile less, exactly one, one more, several, blocks that end on
tile edges and blocks longer than two tiles.  Every call shares one workspace, pre-filled
with 0xFF and never cleared between cases, whatever the previous case left in it; the start
array carries a canary behind the entries the call may write."""

import numpy as np
import pytest

import cut_model as CM
from merge_gpu import capture

pytestmark = pytest.mark.gpu

CANARY = 0x5A5A5A5A
PAD = 8  # canary entries behind the starts


class Cutter:
    def __init__(self, gpu, max_items):
        import torch
        self.gpu, self.torch = gpu, torch
        self.ws = torch.full((gpu.lib().lsm_cut_workspace_size(max_items),), 0xFF, dtype=torch.uint8, device="cuda")

    def buffers(self, ko, vo, cap_blocks, d_n=None):
        torch = self.torch
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).cuda()
        b = {"ko": dev(ko), "vo": dev(vo) if vo is not None else None,
             "d_n": torch.tensor([d_n], dtype=torch.int64, device="cuda") if d_n is not None else None,
             "starts": torch.full((cap_blocks + 1 + PAD,), CANARY, dtype=torch.int32, device="cuda"),
             "nb": torch.full((1,), -1, dtype=torch.int64, device="cuda"),
             "st": torch.full((1,), -1, dtype=torch.int32, device="cuda"),
             "n": len(ko) - 1, "cap": cap_blocks}
        return b

    def launch(self, b, bs, extra=0):
        gpu = self.gpu
        need = gpu.lib().lsm_cut_workspace_size(b["n"])
        assert need <= self.ws.numel()
        rc = gpu.lib().lsm_cut_blocks_device(gpu._ptr(b["ko"]), gpu._ptr(b["vo"]), b["n"], gpu._ptr(b["d_n"]), extra, bs,
                                             gpu._ptr(b["starts"]), b["cap"], gpu._ptr(b["nb"]), gpu._ptr(b["st"]),
                                             gpu._ptr(self.ws), need, gpu._stream(None))
        assert rc == 0

    def read(self, b):
        """-> (starts written: list, n_blocks, status); checks the canary."""
        self.torch.cuda.synchronize()
        nb, st = int(b["nb"].item()), int(b["st"].item())
        starts = b["starts"].cpu().numpy().view(np.uint32)
        written = min(nb, b["cap"]) + 1
        assert (starts[written:] == CANARY).all(), "wrote behind the last start"
        return [int(x) for x in starts[:written]], nb, st

    def cut(self, ko, vo, bs, extra=0, cap_blocks=None, d_n=None):
        n = len(ko) - 1
        b = self.buffers(ko, vo, max(n, 1) if cap_blocks is None else cap_blocks, d_n)
        self.launch(b, bs, extra)
        return self.read(b)


@pytest.fixture(scope="module")
def cutter(gpu):
    return Cutter(gpu, 3 * gpu.CUT_TILE_ITEMS + 64)


def _off(w, base=0):
    return np.concatenate([[base], base + np.cumsum(np.asarray(w, np.uint64), dtype=np.uint64)]).astype(np.uint64)


def _random_offsets(seed, n, kmax=30, vmax=380):
    rng = np.random.default_rng(seed)
    return _off(rng.integers(1, kmax + 1, n)), _off(rng.integers(0, vmax + 1, n))


def _expect(gpu, ko, vo, bs, extra=0):
    if extra == 0 and vo is not None:
        return [int(x) for x in gpu.cut_blocks(ko, vo, bs)]
    return CM.loop_cut(ko, vo, bs, extra)


def _check(cutter, ko, vo, bs, extra=0, **kw):
    want = _expect(cutter.gpu, ko, vo, bs, extra)
    got, nb, st = cutter.cut(ko, vo, bs, extra, **kw)
    assert st == 0 and nb == len(want) - 1
    assert got == want
    return want


def _sizes(T):
    return [0, 1, 2, T - 1, T, T + 1, 2 * T + 1, 3 * T + 5]


@pytest.mark.parametrize("k", range(8))
def test_sizes_around_the_tile(gpu, cutter, k):
    n = _sizes(gpu.CUT_TILE_ITEMS)[k]
    ko, vo = _random_offsets(k, n)  # mean weight 205: about 5 items per 1 KiB block
    want = _check(cutter, ko, vo, 1024)
    assert n == 0 or 4 < n / (len(want) - 1) < 7 or n < 3


@pytest.mark.parametrize("bs", [0, 1])
def test_every_item_its_own_block(gpu, cutter, bs):
    n = gpu.CUT_TILE_ITEMS + 3
    rng = np.random.default_rng(bs)
    ko = _off(rng.integers(1 if bs else 0, 3, n))  # block_size 0 cuts after zero-weight items too
    vo = _off(rng.integers(0, 3, n))
    assert _check(cutter, ko, vo, bs) == list(range(n + 1))


@pytest.mark.parametrize("per_block", [64, 16384, 16384 * 2, 4096 * 3])
def test_uniform_weights_cut_on_tile_boundaries(gpu, cutter, per_block):
    T = gpu.CUT_TILE_ITEMS
    assert T % 64 == 0 and T == 16384
    n = 3 * T
    ko, vo = _off([8] * n), _off([8] * n)
    want = _check(cutter, ko, vo, 16 * per_block)
    assert want == list(range(0, n, per_block)) + [n]


def test_block_spans_whole_tiles(gpu, cutter):
    T = gpu.CUT_TILE_ITEMS
    n = 3 * T + 7
    ko, vo = _off([1] * n), _off([0] * n)
    assert _check(cutter, ko, vo, 2 * T + 3) == [0, 2 * T + 3, n]
    assert _check(cutter, ko, vo, 0xFFFFFFFF) == [0, n]
    assert _check(cutter, ko, None, 2 * T + 3, extra=1) == [0, T + 2, 2 * T + 4, 3 * T + 6, n]


def test_zero_weight_runs_across_tile_edges(gpu, cutter):
    T = gpu.CUT_TILE_ITEMS
    n = 2 * T + 100
    rng = np.random.default_rng(9)
    kw, vw = rng.integers(1, 30, n), rng.integers(0, 380, n)
    for a, b in ((T - 10, T + 10), (2 * T - 1, 2 * T + 1), (T - 300, T), (2 * T, 2 * T + 40), (n - 5, n)):
        kw[a:b] = 0
        vw[a:b] = 0
    _check(cutter, _off(kw), _off(vw), 1024)
    kw[:] = 0  # nothing but zero weights in the keys; values decide
    _check(cutter, _off(kw), _off(vw), 1024)
    vw[:] = 0  # no weight at all: one block (the flush of the last partial one)
    assert _check(cutter, _off(kw), _off(vw), 1) == [0, n]


@pytest.mark.parametrize("bs", [1 << 31, 0xFFFFFFFF, 5])
def test_large_offsets_and_weights(gpu, cutter, bs):
    n = gpu.CUT_TILE_ITEMS + 100
    rng = np.random.default_rng(bs & 0xFFFF)
    ko = _off(rng.integers(0, 1 << 31, n), base=(1 << 40) + 5)
    vo = _off(rng.integers(0, (1 << 31) + 1, n), base=1 << 41)
    assert int(vo[-1]) > 1 << 44
    _check(cutter, ko, vo, bs)


@pytest.mark.parametrize("extra,bs", [(48, 256), (48, 0), (1, 4096)])
def test_extra_per_item_without_values(gpu, cutter, extra, bs):
    n = gpu.CUT_TILE_ITEMS + 1
    ko, _ = _random_offsets(extra + bs, n, kmax=40)
    _check(cutter, ko, None, bs, extra=extra)


@pytest.mark.parametrize("count", [0, 1, 16384 + 17])
def test_device_count_below_capacity(gpu, cutter, count):
    """Only entries 0 .. count of both arrays are defined; the rest is 0xFF."""
    T = gpu.CUT_TILE_ITEMS
    cap = 2 * T + 50
    ko, vo = _random_offsets(count, count)
    want = _expect(gpu, ko, vo, 1024)
    fill = np.full(cap - count, 0xFFFFFFFFFFFFFFFF, np.uint64)
    got, nb, st = cutter.cut(np.concatenate([ko, fill]), np.concatenate([vo, fill]), 1024, d_n=count)
    assert st == 0 and nb == len(want) - 1 and got == want
    # a count beyond the capacity is clamped to it
    ko, vo = _random_offsets(1, 500)
    got, nb, st = cutter.cut(ko, vo, 1024, d_n=1 << 40)
    assert st == 0 and got == _expect(gpu, ko, vo, 1024)


@pytest.mark.parametrize("cap", [1, 7, 3300])
def test_overflow_reports_the_real_count(gpu, cutter, cap):
    n = 2 * gpu.CUT_TILE_ITEMS + 9
    ko, vo = _random_offsets(4, n)
    want = _expect(gpu, ko, vo, 1024)
    assert len(want) - 1 > cap + 1000
    got, nb, st = cutter.cut(ko, vo, 1024, cap_blocks=cap)
    assert st == 6 and nb == len(want) - 1
    assert got == want[:cap + 1]
    # exactly enough room: no overflow
    got, nb, st = cutter.cut(ko, vo, 1024, cap_blocks=len(want) - 1)
    assert st == 0 and got == want


@pytest.mark.parametrize("which,at", [("key", 1), ("key", 16384 + 77), ("val", 2 * 16384), ("val", 5)])
def test_decreasing_offsets_are_rejected(gpu, cutter, which, at):
    n = 2 * gpu.CUT_TILE_ITEMS + 9
    ko, vo = _random_offsets(6, n)
    good = _expect(gpu, ko, vo, 1024)
    bad = (ko if which == "key" else vo).copy()
    bad[at] = bad[at - 1] - 1 if bad[at - 1] else bad[at + 1] + 1
    assert (np.diff(bad.astype(np.int64)) < 0).any()
    got, nb, st = cutter.cut(bad if which == "key" else ko, vo if which == "key" else bad, 1024)
    assert st == 10 and nb == 0 and got == [0]
    # the same workspace right after the rejection
    got, nb, st = cutter.cut(ko, vo, 1024)
    assert st == 0 and got == good


def test_workspace_of_any_content(gpu, cutter):
    """The call clears what it needs: a workspace full of 0xFF, of zeros, or of a larger batch's leftovers."""
    T = gpu.CUT_TILE_ITEMS
    big, small = _random_offsets(7, 3 * T + 5), _random_offsets(8, T + 1)
    for fill in (0xFF, 0x00, None, 0x01):
        if fill is None:
            _check(cutter, *big, 1024)
        else:
            cutter.ws.fill_(fill)
        _check(cutter, *small, 1024)
        _check(cutter, *small, 64)


def test_graph_replay_over_new_offsets(gpu, cutter):
    import torch
    T = gpu.CUT_TILE_ITEMS
    n = T + 300
    sets = [_random_offsets(s, n) for s in (20, 21)]
    dec = sets[0][0].copy()
    dec[T + 1] = dec[T] - 1
    b = cutter.buffers(*sets[0], n)
    graph = capture(lambda: cutter.launch(b, 1024))
    for ko, vo, ok in ((*sets[0], True), (*sets[1], True), (dec, sets[0][1], False), (*sets[0], True)):
        b["ko"].copy_(torch.from_numpy(ko.view(np.int64)))
        b["vo"].copy_(torch.from_numpy(vo.view(np.int64)))
        b["starts"].fill_(CANARY)
        b["nb"].fill_(-1)
        b["st"].fill_(-1)
        graph.replay()
        got, nb, st = cutter.read(b)
        if ok:
            want = _expect(gpu, ko, vo, 1024)
            assert st == 0 and nb == len(want) - 1 and got == want
        else:
            assert st == 10 and nb == 0 and got == [0]
