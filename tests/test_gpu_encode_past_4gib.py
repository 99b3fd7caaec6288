"""lsm_encode_blocks (u64 offsets) with an output that passes 2^31 and 2^32.

The encode writes from offset 0, so its block offsets only pass a line when the output does: one
batch of about 4 GiB + 8 MiB (tests/far_offsets.py encode_layout).  Filler blocks hold one item
with a 4 MiB value, generated on the device and never copied to the host; about 1 MiB before
each line the batch switches to a mix of about 300 small blocks (4 KiB and 16 KiB blocks, a block
above 96 KiB, a run of 130-item blocks), so that every encode writer computes output addresses on
both sides of both lines.  Checked: every status, the small blocks and the fillers next to them
byte for byte against the oracle's encoding of the same items, every block offset against the
oracle's sizes, a decode of the whole output on the device (a write that went astray would have
broken a block's checksum), and lsm_index_entries over the real offsets.  Run once with the
workspace pool and once with the run plan fused into the group kernel (which the pool excludes).
Needs about 9 GiB of device memory."""
import numpy as np
import pytest

import far_offsets as F
import pyoracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def batch(gpu):
    """The device items of the layout: counter keys, random values made on the device."""
    import torch
    lay = F.encode_layout()
    n = len(lay["val_len"])
    val_off = np.concatenate([[0], np.cumsum(lay["val_len"])]).astype(np.int64)
    try:
        vals = torch.empty(int(val_off[-1]) + gpu.LSM_INPUT_PADDING, dtype=torch.uint8, device="cuda")
    except RuntimeError as e:
        pytest.skip(f"cannot allocate the {int(val_off[-1]) >> 20} MiB value arena: {e}")
    vals.random_(0, 256)
    items = {"keys": gpu.to_device_bytes(F.enc_keys(0, n)),
             "key_off": torch.arange(n + 1, dtype=torch.int64, device="cuda") * F.ENC_KEY,
             "vals": vals, "val_off": torch.from_numpy(val_off).cuda(),
             "seqno": torch.full((n,), 63, dtype=torch.int64, device="cuda"),
             "vtype": torch.zeros(n, dtype=torch.uint8, device="cuda")}
    yield lay, items, val_off, torch.from_numpy(lay["starts"].astype(np.int32)).cuda()
    del items, vals
    torch.cuda.empty_cache()


def _oracle_blocks(lay, items, val_off, b0, b1):
    """pyoracle.encode_blocks of blocks [b0, b1), their values copied from the device."""
    i0, i1 = int(lay["starts"][b0]), int(lay["starts"][b1])
    vals = items["vals"][int(val_off[i0]):int(val_off[i1])].cpu().numpy()
    buf, off = pyoracle.encode_blocks(*F.enc_slice(lay, b0, b1, vals), nthreads=4)
    return buf, off


@pytest.mark.parametrize("variant", ["pool", "fused-run-plan"])
def test_encode_output_past_4gib(gpu, batch, variant):
    import torch
    lay, items, val_off, d_starts = batch
    nb = len(lay["kind"])
    try:
        enc = gpu.Encoder().encode(items, d_starts, nb, pool=(variant == "pool"), run_plan=(variant != "pool"))
    except torch.cuda.OutOfMemoryError as e:
        pytest.skip(f"cannot allocate the output: {e}")
    torch.cuda.synchronize()
    assert int((enc["status"][:nb] != 0).sum().item()) == 0
    off = enc["block_off"].cpu().numpy().view(np.uint64)
    assert off[0] == 0 and (np.diff(off).astype(np.int64) == lay["size"]).all()
    assert (off == lay["off"]).all() and int(off[-1]) > F.L32 + (6 << 20)
    # the mixes, the short filler below and the full filler above each: byte for byte
    for first, last in lay["mixes"]:
        for b0, b1 in ((first - 1, first), (first, last), (last, last + 1)):
            want, woff = _oracle_blocks(lay, items, val_off, b0, b1)
            assert (woff + off[b0] == off[b0:b1 + 1]).all()
            got = enc["buf"][int(off[b0]):int(off[b1])].cpu().numpy()
            assert got.tobytes() == want.tobytes(), (variant, b0, b1)
    # the whole output decodes: no write went astray
    n = len(lay["val_len"])
    out = gpu.decode_blocks(enc["buf"], enc["block_off"], nb, expect_type=0, item_cap=n + 64, pool=True,
                            fields=["seqno", "key_off", "key_len", "prefix_len", "val_off", "val_len", "vtype"])
    torch.cuda.synchronize()
    assert int((out["status"][:nb] != 0).sum().item()) == 0
    assert out["item_start"].cpu().numpy().view(np.uint32).tolist() == lay["starts"].tolist()
    assert (out["val_len"][:n].cpu().numpy().view(np.uint32) == lay["val_len"]).all()
    # the index entries over the real offsets
    idx = gpu.index_entries(items, d_starts, enc["block_off"], nb)
    torch.cuda.synchronize()
    assert int(idx["result"].item()) == 0
    assert (idx["handle_off"].cpu().numpy().view(np.uint64) == off[:-1]).all()
    assert (idx["handle_size"].cpu().numpy().astype(np.int64) == lay["size"]).all()
    last = lay["starts"][1:] - 1
    assert idx["keys"][:nb * F.ENC_KEY].cpu().numpy().reshape(nb, F.ENC_KEY).tolist() == \
        F.enc_keys(0, len(lay["val_len"])).reshape(-1, F.ENC_KEY)[last].tolist()
