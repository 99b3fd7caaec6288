"""The wrappers that take a temporary workspace or read a device value back give the same
answer on a caller's side stream (stream=torch.cuda.Stream(), not the current one) as on the
current stream: the workspace is recorded on that stream (lsmgpu._workspace) and every read-back
waits for it (lsmgpu._read_back).  Inputs: 30 random items in data blocks of 256 bytes, as plain
blocks, as LZ4 blocks and as one table image; one plain call per stream, outputs compared over
the rows each call defines."""
import numpy as np
import pytest

import pyoracle
from helpers import random_sorted_items

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def case(gpu):
    """Everything the calls read, prepared on the current stream and complete before any call."""
    import torch
    items = random_sorted_items(30)
    d_items = gpu.items_to_device(items)
    starts = pyoracle.cut_blocks(items, 256)
    nb = len(starts) - 1
    assert nb >= 3
    enc = gpu.Encoder().encode(d_items, torch.from_numpy(starts.astype(np.int32)).cuda(), nb)
    c = {"gpu": gpu, "items": d_items, "nb": nb, "enc": enc,
         "lz": gpu.lz4_compress_blocks(enc["buf"], enc["block_off"], nb, in_status=enc["status"]),
         "dec": gpu.decode_blocks(enc["buf"], enc["block_off"], nb),
         "table": gpu.write_table(d_items, block_size=256),
         "run_start": torch.tensor([0, 15, 30], dtype=torch.int64, device="cuda")}
    t = c["table"]
    assert t["block_count"] == nb
    key10 = bytes(items.keys[int(items.key_off[10]):int(items.key_off[11])])
    lo, lo_off = gpu.to_device_bytes(key10), torch.tensor([0, 0, len(key10)], dtype=torch.int64, device="cuda")
    hi, hi_off = gpu.to_device_bytes(b""), torch.zeros(3, dtype=torch.int64, device="cuda")
    flags = torch.tensor([0, gpu.SEEK_LO], dtype=torch.uint8, device="cuda")  # every row; the rows from item 10 on
    c["pos"] = gpu.table_range(t["file"], t, lo, lo_off, hi, hi_off, flags,
                               scan={"block_off": t["block_off"], "item_start": t["starts"]})
    torch.cuda.synchronize()
    assert c["pos"]["outcome"].cpu().tolist() == [gpu.RANGE_ROWS] * 2
    return c


def sync():
    """Everything queued has run: what follows a call reads its outputs."""
    import torch
    torch.cuda.synchronize()


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else x


def parsed(gpu, out, nb):
    """A decode output dict over the blocks and rows it defines (handle_off: index blocks only)."""
    n = int(out["item_start"][nb].item())
    got = {f: host(out[f])[:n] for f, _ in gpu.PARSED_FIELDS if f != "handle_off"}
    got.update(n=n, item_start=host(out["item_start"])[:nb + 1], status=host(out["status"])[:nb])
    return got


def items_rows(out, n, key_bytes, val_bytes):
    """An lsm_items-shaped output dict over its first n rows."""
    return {"keys": host(out["keys"])[:key_bytes], "vals": host(out["vals"])[:val_bytes],
            "key_off": host(out["key_off"])[:n + 1], "val_off": host(out["val_off"])[:n + 1],
            "seqno": host(out["seqno"])[:n], "vtype": host(out["vtype"])[:n]}


def lz4_decompress_blocks(c, s):
    out, off, status = c["gpu"].lz4_decompress_blocks(c["lz"]["buf"], c["lz"]["block_off"], c["nb"], stream=s)
    sync()
    assert out.numel() == int(off[-1].item()) > 0
    return {"out": host(out), "off": host(off), "status": host(status)}


def decode_lz4_blocks(c, s):
    out = c["gpu"].decode_lz4_blocks(c["lz"]["buf"], c["lz"]["block_off"], c["nb"], stream=s)
    sync()
    got = parsed(c["gpu"], out, c["nb"])
    end = int(out["frame_off"][-1].item())
    got.update(frames=host(out["frames"])[:end], frame_off=host(out["frame_off"]),
               decode_status=host(out["decode_status"])[:c["nb"]])
    return got


def materialize_keys(c, s):
    keys, key_off = c["gpu"].materialize_keys(c["enc"]["buf"], c["enc"]["block_off"], c["nb"], c["dec"], stream=s)
    sync()
    assert key_off.numel() == 31
    return {"keys": host(keys)[:int(key_off[-1].item())], "key_off": host(key_off)}


def scan_table(c, s, host_sync):
    t = c["table"]
    out = c["gpu"].scan_table(t["file"], t["file"].numel(), t["tli_off"], t["tli_size"], stream=s, sync=host_sync,
                              data_blocks_hint=0 if host_sync else c["nb"])
    sync()
    nb, status = (out[f] if host_sync else int(out[f].item()) for f in ("n_blocks", "table_status"))
    assert (nb, status) == (c["nb"], 0)
    got = parsed(c["gpu"], out, nb)
    got.update(block_off=host(out["block_off"])[:nb + 1])
    return got


def xxh3_128_file(c, s):
    t = c["table"]
    digest = c["gpu"].xxh3_128_file(t["file"], t["file"].numel(), stream=s)
    sync()
    return {"digest": np.array(digest, dtype=np.uint64)}


def cut_blocks_device(c, s):
    starts = c["gpu"].cut_blocks_device(c["items"], 256, stream=s)
    sync()
    assert starts.numel() == c["nb"] + 1
    return {"starts": host(starts)}


def merge_runs(c, s):
    out = c["gpu"].merge_runs(c["items"], c["run_start"], stream=s)
    sync()
    n = int(out["n_out"].item())
    assert 0 < n <= 30
    got = items_rows(out, n, int(out["key_off"][n].item()), int(out["val_off"][n].item()))
    got.update(src=host(out["src"])[:n], status=host(out["status"])[:2])
    return got


def table_range_rows(c, s):
    t = c["table"]
    out = c["gpu"].table_range_rows(t["file"], t, c["pos"], t["block_off"], stream=s)
    sync()
    rows, key_bytes, val_bytes = out["end"].cpu().tolist()
    assert rows == out["seqno"].numel() > 30  # (every row, then the rows from item 10's key on)
    got = items_rows(out, rows, key_bytes, val_bytes)
    got.update({f: host(out[f]) for f in ("run_start", "row_status", "end", "need", "result", "plan_result")})
    return got


CALLS = [(lz4_decompress_blocks, ()), (decode_lz4_blocks, ()), (materialize_keys, ()), (scan_table, (True,)),
         (scan_table, (False,)), (xxh3_128_file, ()), (cut_blocks_device, ()), (merge_runs, ()),
         (table_range_rows, ())]


@pytest.mark.parametrize("call,args", CALLS,
                         ids=[f.__name__ + "".join(f"-sync={a}" for a in args) for f, args in CALLS])
def test_side_stream_gives_the_current_streams_answer(case, call, args):
    import torch
    want = call(case, None, *args)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    got = call(case, side, *args)
    assert sorted(got) == sorted(want)
    for f in want:
        assert np.array_equal(got[f], want[f]), f
