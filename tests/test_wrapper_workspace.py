"""Host-side checks of the ctypes mirror's workspace handling (no GPU: the
library is replaced by a recorder; the size functions are the real ones).

Since ABI 7 the huge-block pool is an explicit opt-in (LSM_DECODE_HUGE_POOL /
LSM_ENCODE_HUGE_POOL, include/lsmgpu.h): a pool=True call passes the flag and
the _ex workspace, a pool=False call neither.  A Decoder reused across calls
still hands a pool=False call exactly lsm_decode_workspace_size(n), however
large an earlier pool=True call grew its cached buffer."""
import ctypes as C

import pytest
import torch

import lsmgpu


class _Recorder:
    def __init__(self, real):
        self.real = real
        self.calls = []

    def __getattr__(self, name):
        if name.startswith("lsm_decode_workspace_size") or name.startswith("lsm_encode_workspace_size") \
                or name == "lsm_encode_bound":
            return getattr(self.real, name)

        def rec(*args):
            self.calls.append((name, args))
            return 0
        return rec


@pytest.fixture
def fake(monkeypatch):
    real = lsmgpu.lib()
    r = _Recorder(real)
    monkeypatch.setattr(lsmgpu, "lib", lambda: r)
    monkeypatch.setattr(lsmgpu, "_torch", lambda: torch)
    monkeypatch.setattr(lsmgpu, "_stream", lambda s: C.c_void_p(0))
    return r


class _Stream:
    """Stands for a caller's side stream."""

    def synchronize(self):
        pass


def test_wrappers_take_workspaces_through_the_helper(fake, monkeypatch):
    """Every wrapper that takes stream= and has a throw-away workspace gets it from _workspace with
    the stream it was given, and hands the library no other: in each recorded call the pointer in
    front of a size_t (the prototypes' workspace_bytes) is one _workspace returned.  The six that
    did not record their stream before (lz4_decompress_blocks, decode_lz4_blocks,
    materialize_keys, scan_table in both modes, xxh3_128_file) are among them.  Decoder and
    Encoder keep a cached workspace (the tests above); their calls are left out."""
    import contextlib
    L = lsmgpu
    # (from the header's text: as a ctypes type size_t is uint64_t's)
    sized = {name: [i for i, t in enumerate(params) if t.strip() == "size_t"]
             for name, (_, params) in L.PROTOTYPES.items()}
    getattr_ = _Recorder.__getattr__
    monkeypatch.setattr(_Recorder, "__getattr__", lambda self, name: (  # (the other stages' workspaces: 64 bytes)
        (lambda *a: 64) if name.endswith("_workspace_size") and not name.startswith(("lsm_decode", "lsm_encode"))
        else getattr_(self, name)))
    monkeypatch.setattr(torch, "empty", torch.zeros)  # (a recorder writes no outputs: counts read back are 0)
    monkeypatch.setattr(torch.cuda, "stream", lambda s: contextlib.nullcontext())
    taken, workspace = [], L._workspace

    def recorder(nbytes, device, stream=None):
        ws = workspace(nbytes, device, stream)
        taken.append((ws, stream))
        return ws
    monkeypatch.setattr(L, "_workspace", recorder)

    s = _Stream()
    u8 = lambda n: torch.zeros(n + 64, dtype=torch.uint8)
    i64 = lambda n: torch.zeros(n, dtype=torch.int64)
    blocks, off, n = u8(256), i64(4), 3
    items = {"keys": u8(64), "key_off": i64(5), "vals": u8(64), "val_off": i64(5), "seqno": i64(4),
             "vtype": torch.zeros(4, dtype=torch.uint8)}
    dec = L.Decoder("cpu").alloc_outputs(8, n)
    table = {"tli_off": 128, "tli_size": 64}
    pos = {f: torch.zeros(2, dtype=torch.int32) for f, _ in L.LsmRangePositions._fields_}
    wrappers = {
        "lz4_decompress_blocks": lambda: L.lz4_decompress_blocks(blocks, off, stream=s),
        "decode_lz4_blocks": lambda: L.decode_lz4_blocks(blocks, off, stream=s),
        "decode_lz4_blocks capped": lambda: L.decode_lz4_blocks(blocks, off, stream=s, frames_cap=512),
        "materialize_keys": lambda: L.materialize_keys(blocks, off, n, dec, stream=s),
        "materialize_keys capped": lambda: L.materialize_keys(blocks, off, n, dec, stream=s, key_cap=64),
        "scan_table": lambda: L.scan_table(blocks, 256, 128, 64, stream=s),
        "scan_table async": lambda: L.scan_table(blocks, 256, 128, 64, stream=s, sync=False),
        "xxh3_128_file": lambda: L.xxh3_128_file(blocks, 256, stream=s),
        "lz4_compress_blocks": lambda: L.lz4_compress_blocks(blocks, off, stream=s),
        "cut_blocks_device": lambda: L.cut_blocks_device(items, 4096, stream=s),
        "index_entries": lambda: L.index_entries(items, torch.zeros(2, dtype=torch.int32), off, 1, stream=s),
        "merge_runs": lambda: L.merge_runs(items, [0, 2, 4], stream=s),
        "merge_read": lambda: L.merge_read(items, [0, 2, 4], 1, 2, 10, stream=s),
        "table_range_rows": lambda: L.table_range_rows(blocks, table, pos, off, stream=s),
        "materialize_items": lambda: L.materialize_items(blocks, off, n, dec, stream=s),
        "tables_to_runs": lambda: L.tables_to_runs([(blocks, off, n, dec), (blocks, off, n, dec)], stream=s),
    }
    for name, call in wrappers.items():
        taken.clear()
        fake.calls.clear()
        call()
        assert taken and all(stream is s for _, stream in taken), name
        ours = {ws.data_ptr() for ws, _ in taken}
        passed = [args[i - 1].value for fn, args in fake.calls if not fn.startswith("lsm_decode_blocks")
                  for i in sized[fn]]
        assert passed and set(passed) <= ours, name
    # a Decoder's workspace_bytes (a workspace of exactly that size, for one call) is such a workspace too
    taken.clear()
    L.Decoder("cpu").decode(blocks, off, n, dec, 8, stream=s, workspace_bytes=4096)
    nbytes, ptr = _ws_arg(fake.calls[-1])
    assert [stream for _, stream in taken] == [s] and nbytes == 4096 and ptr.value == taken[0][0].data_ptr()
    # on the current stream the helper is told no stream (it records the current one itself)
    taken.clear()
    L.xxh3_128_file(blocks, 256)
    assert [stream for _, stream in taken] == [None]


def _ws_arg(call):
    name, args = call
    assert name in ("lsm_decode_blocks", "lsm_decode_blocks_tuned")
    return args[9], args[8]  # workspace_bytes, workspace pointer


def _pool_flag(call):
    name, args = call
    if name == "lsm_decode_blocks":  # (no tuning: never the pool)
        return False
    return bool(args[10]._obj.flags & lsmgpu.DECODE_HUGE_POOL)


def test_decoder_pool_then_no_pool(fake):
    n = 100
    blocks = torch.zeros(n * 300 * 1024, dtype=torch.uint8)  # 300 KiB mean: the pool would pay
    off = torch.zeros(n + 1, dtype=torch.int64)
    d = lsmgpu.Decoder("cpu")
    out = d.alloc_outputs(16, n)
    d.decode(blocks, off, n, out, 16, pool=True)
    d.decode(blocks, off, n, out, 16, pool=False)
    d.decode(blocks, off, n, out, 16)  # default: the mean block size picks the pool
    base = fake.real.lsm_decode_workspace_size(n)
    full = fake.real.lsm_decode_workspace_size_ex(n, blocks.numel())
    got = [_ws_arg(c)[0] for c in fake.calls]
    assert got == [full, base, full]
    assert [_pool_flag(c) for c in fake.calls] == [True, False, True]
    threshold = ((base + 255) & ~255) + 8704  # lsmgpu.h: the pool threshold
    assert base < threshold <= full
    # the cached buffer is reused (one allocation), only its view changes
    assert len({_ws_arg(c)[1].value for c in fake.calls}) == 1


def test_encoder_passes_exact_workspace(fake):
    n_items, n_blocks = 64, 4
    items = {"keys": torch.zeros(64 * 16 + 64, dtype=torch.uint8),
             "key_off": torch.arange(n_items + 1, dtype=torch.int64) * 16,
             "vals": torch.zeros(64 * 64 + 64, dtype=torch.uint8),
             "val_off": torch.arange(n_items + 1, dtype=torch.int64) * 64,
             "seqno": torch.zeros(n_items, dtype=torch.int64), "vtype": torch.zeros(n_items, dtype=torch.uint8)}
    starts = torch.arange(0, n_items + 1, 16, dtype=torch.int32)
    e = lsmgpu.Encoder("cpu")
    e.encode(items, starts, n_blocks, pool=True)
    e.encode(items, starts, n_blocks, pool=False)
    ws = [args[9] for name, args in fake.calls if name == "lsm_encode_blocks"]
    assert ws[1] == fake.real.lsm_encode_workspace_size(n_items, n_blocks) < ws[0]
    flags = [args[3]._obj.flags for name, args in fake.calls if name == "lsm_encode_blocks"]
    assert flags == [lsmgpu.ENCODE_HUGE_POOL, 0]


def test_encoder_run_plan_flag(fake):
    """run_plan=True asks for the run-level plan (LSM_ENCODE_RUN_PLAN), alone or with the pool."""
    n_items, n_blocks = 64, 4
    items = {"keys": torch.zeros(64 * 16 + 64, dtype=torch.uint8),
             "key_off": torch.arange(n_items + 1, dtype=torch.int32) * 16,
             "vals": torch.zeros(64 * 64 + 64, dtype=torch.uint8),
             "val_off": torch.arange(n_items + 1, dtype=torch.int32) * 64,
             "seqno": torch.zeros(n_items, dtype=torch.int64), "vtype": torch.zeros(n_items, dtype=torch.uint8)}
    starts = torch.arange(0, n_items + 1, 16, dtype=torch.int32)
    e = lsmgpu.Encoder("cpu")
    e.encode(items, starts, n_blocks, pool=False, run_plan=True)
    e.encode(items, starts, n_blocks, pool=True, run_plan=True)
    e.encode(items, starts, n_blocks, pool=False)
    calls = [(name, args) for name, args in fake.calls if name.startswith("lsm_encode_blocks")]
    assert [name for name, _ in calls] == ["lsm_encode_blocks32"] * 3  # (int32 offsets: the u32 entry)
    assert [args[3]._obj.flags for _, args in calls] == [lsmgpu.ENCODE_RUN_PLAN,
                                                         lsmgpu.ENCODE_HUGE_POOL | lsmgpu.ENCODE_RUN_PLAN, 0]
