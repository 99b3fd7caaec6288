"""bench.py's command line: a plain run reports the headline only, --full adds the
rest, --dump-outputs writes what the last timed step computed."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from helpers import counter_items

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

HEAD_KEYS = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus"}
FULL_ONLY_KEYS = {"roofline", "roofline_decode", "roofline_encode", "cpu_baseline", "encode", "decode",
                  "decode_compact", "host_inclusive", "point_read", "config4", "config5", "large_blocks"}


def load_dump(d):
    return {p.name[:-4]: np.load(p) for p in sorted(Path(d).glob("*.npy"))}


def test_dump_outputs_layout(oracle, tmp_path):
    """dump_outputs over a batch the oracle encoded and decoded (host tensors of the
    wrappers' dtypes): float32 / float64 files, the whole per-block arrays, chunk sums
    over every byte and item, and the sampled blocks' bytes and fields, the same twice."""
    import torch
    import bench
    nb_items = 52 * 1500  # more blocks than the sample, more bytes than one chunk
    items = counter_items(nb_items, seed=5)
    starts = oracle.cut_blocks(items, 4096)
    nb = len(starts) - 1
    assert nb > bench.DUMP_SAMPLE_BLOCKS
    buf, off = oracle.encode_blocks(items, starts, nthreads=2)
    parsed, item_start, status = oracle.decode_blocks(buf, off, nthreads=2)
    n = int(item_start[-1])
    assert n == nb_items and int(off[-1]) > bench.DUMP_CHUNK and int(off[-1]) % bench.DUMP_CHUNK
    enc = {"buf": torch.from_numpy(np.concatenate([buf, np.zeros(64, np.uint8)])),
           "block_off": torch.from_numpy(off.astype(np.int64)),
           "status": torch.zeros(nb, dtype=torch.int32)}
    signed = {"uint64": np.int64, "uint32": np.int32, "uint16": np.int16, "uint8": np.uint8}
    out = {f: torch.from_numpy(parsed[f].astype(bench.FIELD_NP[f]).view(signed[bench.FIELD_NP[f]]).copy())
           for f in bench.DATA_FIELDS}
    out["item_start"] = torch.from_numpy(item_start.astype(np.int32))
    out["status"] = torch.from_numpy(status.astype(np.int32))
    bench.dump_outputs(torch, tmp_path / "a", enc, out, nb, n)
    bench.dump_outputs(torch, tmp_path / "b", enc, out, nb, n)
    a, b = load_dump(tmp_path / "a"), load_dump(tmp_path / "b")
    assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert np.array_equal(a["enc_block_off"], off.astype(np.float64))
    assert np.array_equal(a["dec_item_start"], item_start.astype(np.float64))
    assert not a["enc_status"].any() and np.array_equal(a["dec_status"], status.astype(np.float32))
    ids = a["sample_blocks"].astype(np.int64)
    assert len(ids) == bench.DUMP_SAMPLE_BLOCKS == len(set(ids)) and (np.diff(ids) > 0).all() and ids[-1] < nb
    exp = np.concatenate([buf[int(off[i]):int(off[i + 1])] for i in ids])
    assert np.array_equal(a["enc_buf_sample"], exp.astype(np.float32))
    total = int(off[-1])
    sums = a["enc_buf_chunk_sums"]
    assert len(sums) == -(-total // bench.DUMP_CHUNK) and sums.sum() == buf[:total].sum(dtype=np.int64)
    assert sums[0] == buf[:bench.DUMP_CHUNK].sum(dtype=np.int64)
    for f in bench.DATA_FIELDS:
        exp = np.concatenate([parsed[f][int(item_start[i]):int(item_start[i + 1])] for i in ids])
        assert np.array_equal(a[f"dec_{f}_sample"], exp.astype(np.float64)), f
        assert a[f"dec_{f}_chunk_sums"].sum() == parsed[f][:n].sum(dtype=np.int64), f


@pytest.mark.gpu
def test_plain_run_reports_the_headline_only(gpu, tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR` at a small batch: one JSON
    line with the headline fields and none of the --full legs, K timed steps, and a dump
    under 64 MB whose arrays agree with the line and with the synthetic input."""
    nb, steps = 3000, 3
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                        "--blocks", str(nb), "--dump-outputs", str(tmp_path / "d")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert HEAD_KEYS <= set(line) and not (FULL_ONLY_KEYS & set(line))
    assert line["steps"] == steps and line["warmup"] == 1 and line["unit"] == "GiB/s" and line["dtype"] == "u8"
    assert line["higher_is_better"] is True and line["value"] > 0 and line["ms_per_step"] > 0
    nbytes = line["config"]["block_bytes_per_gpu"]
    assert line["value"] == pytest.approx(nbytes / (line["ms_per_step"] * 1e-3) / 2 ** 30, rel=1e-3)
    d = load_dump(tmp_path / "d")
    assert sum(v.nbytes for v in d.values()) <= 64 << 20
    assert all(v.dtype in (np.float32, np.float64) for v in d.values())
    assert len(d["enc_block_off"]) == nb + 1 and d["enc_block_off"][-1] == nbytes
    assert d["dec_item_start"][-1] == line["config"]["items_per_gpu"] == 52 * nb
    assert not d["enc_status"].any() and not d["dec_status"].any()
    assert len(d["sample_blocks"]) == 1024 and len(d["dec_seqno_sample"]) == 1024 * 52
    assert (d["dec_seqno_sample"] == 63).all() and (d["dec_val_len_sample"] == 64).all()
    assert d["enc_buf_chunk_sums"].sum() > 0 and len(d["enc_buf_sample"]) > 1024 * 3700
