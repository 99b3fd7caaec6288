"""Fixtures for the tests of 64-bit input offsets past 2 GiB and 4 GiB.

One device buffer of ARENA_BYTES stands for every input arena of the C ABI (blocks, needles,
bounds, keys, values, a table image).  A small batch is laid at an absolute offset so that bit 31
or bit 32 of its offsets is set, the pointer handed to the library stays the buffer's first byte,
and the regions a truncated offset would reach (the same bytes 2^32 and 2^31 lower) are filled
with CANARY, as are GUARD bytes on both sides of the batch: a kernel that loses a bit reads bytes
that are no block and the comparison with the oracle fails, instead of reading stale data."""
from __future__ import annotations

import numpy as np

import pyoracle
from helpers import counter_items, index_items, prefix_items, random_sorted_items

L31, L32 = 1 << 31, 1 << 32
ARENA_BYTES = L32 + (16 << 20)
ABOVE = L32 + (1 << 20) + 5  # base of the batch laid wholly above L32
GUARD = 4096
CANARY = 0xA5
MARGIN = 64                  # a line "inside" a block lies at least this far from both its ends

LDS_STAGE = 34560            # 33.75 KiB: payloads above it leave the group kernel (big path)
HUGE_PAYLOAD = 72 << 10      # payloads above it take the pool that spreads a block over the GPU


# ---- the batch under test ---------------------------------------------------------------------

def item_keys(items):
    """The keys of a pyoracle.Items, as bytes."""
    ko = items.key_off
    return [items.keys[int(ko[i]):int(ko[i + 1])].tobytes() for i in range(items.n)]


_batch = None


def batch():
    """The deterministic block mix (built once): dict(blocks = list of on-disk blocks, classes =
    one tag per block, items = the pyoracle.Items a block was encoded from or None, buf / off = the
    compact batch from offset 0, k_small = a block in the middle of the first small-block group,
    k_largest = the largest block)."""
    global _batch
    if _batch is not None:
        return _batch
    blocks, classes, src = [], [], []

    def add(tag, items, payload=None, block_type=0, **kw):
        if payload is None:
            payload = pyoracle.data_block_encode(items, **kw)
        blocks.append(pyoracle.block_write(payload, block_type=block_type))
        classes.append(tag)
        src.append(items)

    def small(i):
        items = random_sorted_items(70, seed=100 + i, kmin=2, kmax=14, vmax=60)
        add("small", items, restart_interval=(1, 16)[i & 1], hash_ratio=(0.0, 1.33)[(i >> 1) & 1])

    for i in range(10):
        small(i)
    add("prefix16k", prefix_items(60, seed=6))
    add("big", counter_items(520, seed=7))
    for i in range(10, 14):
        small(i)
    add("huge", counter_items(1800, val_len=200, seed=8))
    add("index", index_items(60), payload=pyoracle.index_block_encode(index_items(60)), block_type=1)
    flipped = bytearray(blocks[3])
    flipped[33 + 50] ^= 0x10
    blocks.append(bytes(flipped)); classes.append("cksum"); src.append(None)
    broken = bytearray(pyoracle.data_block_encode(random_sorted_items(70, seed=131, kmin=2, kmax=14, vmax=60)))
    broken[-31 + 2] ^= 0x7F  # the trailer's restart count: structurally broken, sealed with a valid checksum
    add("parse", None, payload=bytes(broken))
    add("tomb", random_sorted_items(80, seed=140, kmin=2, kmax=14, vmax=40, big_seq=True))
    for i in range(14, 20):
        small(i)
    off = np.zeros(len(blocks) + 1, np.uint64)
    off[1:] = np.cumsum([len(b) for b in blocks])
    buf = np.frombuffer(b"".join(blocks), np.uint8).copy()
    sizes = [len(b) for b in blocks]
    _batch = {"blocks": blocks, "classes": classes, "items": src, "buf": buf, "off": off,
              "k_small": 5, "k_largest": int(np.argmax(sizes))}
    return _batch


# ---- placement --------------------------------------------------------------------------------

def anchors(compact_off, k, line):
    """Base offsets for a contiguous batch (compact offsets compact_off, from 0) laid at that base,
    one per placement kind: "inside" = the line strictly inside block k, MARGIN or more from each
    end, the base no multiple of 16; "at" = the line exactly block k's first byte; "above" = the
    batch wholly above L32."""
    lo, hi = int(compact_off[k]), int(compact_off[k + 1])
    assert hi - lo >= 2 * MARGIN + 32, "block k too short to hold the line with its margins"
    inside = line - (lo + (hi - lo) // 2)
    if inside % 16 == 0:
        inside -= 3
    return {"inside": inside, "at": line - lo, "above": ABOVE}


def placements_of(off, k_small, k_largest):
    """Every (id, line, k, kind, base) a batch of compact offsets `off` is run at: per line, block k
    once in the middle of a small-block group and once the largest block, "inside" and "at"; and
    the batch above L32."""
    out = []
    for name, line in (("L31", L31), ("L32", L32)):
        for kname, k in (("small", k_small), ("largest", k_largest)):
            a = anchors(off, k, line)
            for kind in ("inside", "at"):
                out.append((f"{name}-{kname}-{kind}", line, k, kind, a[kind]))
    out.append(("above", L32, 0, "above", ABOVE))
    return out


def placements():
    """placements_of the batch under test."""
    b = batch()
    return placements_of(b["off"], b["k_small"], b["k_largest"])


def short_anchors(off, k):
    """[(id, base)] for an arena of short pieces (keys, values; compact offsets `off`): per line,
    the line one byte into piece k and exactly at its first byte; and the arena above L32."""
    lo = int(off[k])
    assert int(off[k + 1]) - lo >= 2
    out = []
    for name, line in (("L31", L31), ("L32", L32)):
        out += [(f"{name}-inside", line - lo - 1), (f"{name}-at", line - lo)]
    return out + [("above", ABOVE)]


def _alias_regions(o, n):
    """Where a read of [o, o + n) lands when bit 32 and above are dropped (2^32 lower) or bit 31 is
    dropped (2^31 lower): the part of the piece at or above each distance, moved down by it."""
    out = []
    for d in (L32, L31):
        lo = max(o, d)
        if lo < o + n:
            out.append((lo - d, o + n - lo))
    return out


def layout(pieces, at, guard=True):
    """pieces: [(offset relative to `at`, length)].  -> dict(placed, guards, aliases), each a list of
    (absolute offset, length): the pieces, the GUARD bytes below the lowest and above the highest
    piece, and the alias regions of every piece part that lies at or above 2^31."""
    placed = [(at + int(r), int(n)) for r, n in pieces if n]
    lo = min(o for o, _ in placed)
    hi = max(o + n for o, n in placed)
    guards = [(lo - GUARD, GUARD), (hi, GUARD)] if guard else []
    aliases = [a for o, n in placed for a in _alias_regions(o, n)]
    return {"placed": placed, "guards": guards, "aliases": aliases}


def overlaps(a, b):
    return [(x, y) for x in a for y in b if x[0] < y[0] + y[1] and y[0] < x[0] + x[1]]


def place(arena, pieces, at, guard=True):
    """Copy small host pieces [(offset relative to `at`, bytes or uint8 array)] to absolute offsets
    of the device arena; fill the alias regions and the guards with CANARY first.  Returns the
    layout (see layout())."""
    import torch
    data = [(r, np.frombuffer(bytes(p), np.uint8).copy() if not isinstance(p, np.ndarray) else p) for r, p in pieces]
    lay = layout([(r, len(p)) for r, p in data], at, guard)
    for o, n in lay["aliases"] + lay["guards"]:
        assert 0 <= o and o + n <= arena.numel(), (o, n)
        arena[o:o + n].fill_(CANARY)
    for r, p in data:
        if len(p):
            o = at + int(r)
            assert 0 <= o and o + len(p) <= arena.numel(), (o, len(p))
            arena[o:o + len(p)].copy_(torch.from_numpy(np.ascontiguousarray(p)))
    return lay


def assert_untouched(arena, *layouts):
    """The guards and alias regions still hold CANARY (for entry points that write nothing into
    the arena)."""
    for lay in layouts:
        for o, n in lay["guards"] + lay["aliases"]:
            assert bool((arena[o:o + n] == CANARY).all().item()), ("arena written at", o, n)


def allocate_arena():
    """The far arena (never filled whole), or a pytest skip when it cannot be allocated."""
    import pytest
    import torch
    try:
        return torch.empty(ARENA_BYTES, dtype=torch.uint8, device="cuda")
    except RuntimeError as e:  # (torch.cuda.OutOfMemoryError is a RuntimeError)
        pytest.skip(f"cannot allocate the {ARENA_BYTES >> 20} MiB arena: {e}")


# ---- a table image larger than 4 GiB ------------------------------------------------------------

def _index_entries(block):
    """An index block as stored -> [(end key, seqno, handle offset, handle size)]."""
    payload = block[33:]
    n, p = pyoracle.data_block_decode(payload, index=True)
    assert n > 0
    out = []
    for i in range(n):
        ko, kl = int(p["key_off"][i]), int(p["key_len"][i])
        assert int(p["prefix_len"][i]) == 0
        out.append((payload[ko:ko + kl], int(p["seqno"][i]), int(p["handle_off"][i]), int(p["val_len"][i])))
    return out


def _index_block(entries):
    it = pyoracle.Items(np.frombuffer(b"".join(e[0] for e in entries), np.uint8),
                        np.concatenate([[0], np.cumsum([len(e[0]) for e in entries])]).astype(np.uint64),
                        np.zeros(0, np.uint8), np.zeros(len(entries) + 1, np.uint64),
                        [e[1] for e in entries], np.zeros(len(entries), np.uint8),
                        [e[2] for e in entries], [e[3] for e in entries])
    return pyoracle.block_write(pyoracle.index_block_encode(it), block_type=1)


def relocate_table(file, table, D, two_level=None):
    """The table pyoracle.table_write wrote (file = its bytes, table = its dict; full or two-level
    index) laid out D bytes into a file.  Data blocks go to old offset + D, back to back; the index
    partitions and the TLI are re-encoded with the oracle's index-block encoder with every handle
    offset moved, and laid after the data blocks in order (their sizes grow with the longer
    varints).  Returns dict(pieces = [(absolute offset, bytes)], map = {old block offset: new
    block offset} for every data block, partition and the TLI, sizes = {new offset: size},
    tli_off, tli_size, file_len, block_off = the data blocks' new offsets (uint64 [n + 1]))."""
    if two_level is None:
        two_level = table["tli_off"] != table["index_off"]
    off = [int(x) for x in table["block_off"]]
    pieces, omap, sizes = [], {}, {}
    for b in range(len(off) - 1):
        pieces.append((off[b] + D, file[off[b]:off[b + 1]]))
        omap[off[b]] = off[b] + D
        sizes[off[b] + D] = off[b + 1] - off[b]
    pos = off[-1] + D
    tli = _index_entries(file[table["tli_off"]:table["tli_off"] + table["tli_size"]])
    if two_level:
        parts = []
        for key, seq, poff, psize in tli:
            ent = [(k, s, omap[o], z) for k, s, o, z in _index_entries(file[poff:poff + psize])]
            blk = _index_block(ent)
            pieces.append((pos, blk))
            omap[poff] = pos
            sizes[pos] = len(blk)
            parts.append((key, seq, pos, len(blk)))
            pos += len(blk)
        tli = parts
    else:
        tli = [(k, s, omap[o], z) for k, s, o, z in tli]
    blk = _index_block(tli)
    pieces.append((pos, blk))
    omap[table["tli_off"]] = pos
    sizes[pos] = len(blk)
    return {"pieces": pieces, "map": omap, "sizes": sizes, "tli_off": pos, "tli_size": len(blk),
            "file_len": pos + len(blk), "two_level": two_level,
            "block_off": np.array([o + D for o in off], np.uint64)}


def table_shift(file, table, where, line=L32):
    """The D at which relocate_table puts `line` strictly inside a data block (where = "data": the
    middle one) or inside an index block (where = "index": the middle partition of a two-level
    index, the TLI of a full one; found by laying the index out again until it holds)."""
    off = [int(x) for x in table["block_off"]]
    if where == "data":
        k = (len(off) - 1) // 2
        return line - (off[k] + (off[k + 1] - off[k]) // 2)
    D = line - off[-1] - 40
    for _ in range(8):
        r = relocate_table(file, table, D)
        index = sorted(o for o in r["sizes"] if o >= off[-1] + D)
        target = index[(len(index) - 1) // 2]
        if target < line < target + r["sizes"][target]:
            return D
        D += line - (target + r["sizes"][target] // 2)
    raise AssertionError("no shift puts the line inside an index block")


def block_holding(reloc, line):
    """(offset, size) of the relocated block that holds `line` strictly inside, None if none does."""
    for o, n in reloc["sizes"].items():
        if o < line < o + n:
            return o, n
    return None


def materialize_file(reloc):
    """The relocated table as real host bytes (for a small D only)."""
    out = bytearray(reloc["file_len"])
    for o, p in reloc["pieces"]:
        out[o:o + len(p)] = p
    return bytes(out)


# ---- an encode batch whose output passes 2^31 and 2^32 -----------------------------------------------
ENC_FILL = 4 << 20     # value bytes of a filler block's one item
ENC_LEAD = 1 << 20     # the small-block mix starts about this far below a line
ENC_TAIL = 2           # filler blocks after the last mix: the batch ends about 8 MiB past L32
ENC_KEY = 16
# half a mix, as (blocks, items per block, value bytes): 4 KiB counter blocks, 16 KiB blocks, one block above
# 96 KiB, a run of blocks of 130 items (the fused run plan's class); a mix is two halves, so that with the line
# inside the second half's 4 KiB blocks every kind lies on both sides of it
ENC_HALF = ((135, 52, 64), (2, 52, 300), (1, 520, 200), (16, 130, 8))
ENC_KINDS = ("4k", "16k", "big", "run")


def enc_keys(first, n):
    """n 16-byte big-endian counters from `first`, flat."""
    ctr = np.arange(first, first + n, dtype=np.uint64)
    keys = np.zeros((n, ENC_KEY), np.uint8)
    for b in range(8):
        keys[:, ENC_KEY - 1 - b] = ((ctr >> np.uint64(8 * b)) & np.uint64(0xFF)).astype(np.uint8)
    return keys.reshape(-1)


def enc_slice(lay, b0, b1, vals=None):
    """Blocks [b0, b1) of an encode layout as (pyoracle.Items, rebased starts); vals: their value
    bytes (uint8 array), default zeros (a block's size does not depend on them)."""
    i0, i1 = int(lay["starts"][b0]), int(lay["starts"][b1])
    vl = lay["val_len"][i0:i1]
    val_off = np.concatenate([[0], np.cumsum(vl)]).astype(np.uint64)
    if vals is None:
        vals = np.zeros(int(val_off[-1]), np.uint8)
    n = i1 - i0
    items = pyoracle.Items(enc_keys(i0, n), np.arange(n + 1, dtype=np.uint64) * np.uint64(ENC_KEY), vals, val_off,
                           np.full(n, 63, np.uint64), np.zeros(n, np.uint8))
    return items, (lay["starts"][b0:b1 + 1] - i0).astype(np.uint32)


def _enc_sizes(lay, b0, b1):
    _, off = pyoracle.encode_blocks(*enc_slice(lay, b0, b1), nthreads=4)
    return np.diff(off).astype(np.int64)


_enc_layout = None


def encode_layout():
    """The batch of the encode test, from sizes alone (built once): dict(starts = item index of each
    block [n_blocks + 1], val_len per item, kind per block ("fill", "short" or one of ENC_KINDS),
    size / off = the oracle's size and output offset of each block, mixes = [(first block, end
    block)] of the two small-block mixes).  Keys are 16-byte big-endian item counters."""
    global _enc_layout
    if _enc_layout is not None:
        return _enc_layout
    counts, vlens, kinds = [], [], []

    def add(kind, items, val_len):
        counts.append(items); vlens.append(val_len); kinds.append(kind)

    def lay_of():
        starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        return {"starts": starts, "val_len": np.repeat(np.array(vlens, np.int64), counts)}

    add("fill", 1, ENC_FILL)
    fill = int(_enc_sizes(lay_of(), 0, 1)[0])
    counts, vlens, kinds = [], [], []
    end, mixes = 0, []
    for line in (L31, L32):
        n = (line - ENC_LEAD - end) // fill
        for _ in range(n):
            add("fill", 1, ENC_FILL)
        end += n * fill
        add("short", 1, line - ENC_LEAD - end - (fill - ENC_FILL))
        first = len(counts)
        for _ in range(2):
            for kind, (blocks, items, val_len) in zip(ENC_KINDS, ENC_HALF):
                for _ in range(blocks):
                    add(kind, items, val_len)
        mixes.append((first, len(counts)))
        end += int(_enc_sizes(lay_of(), first - 1, len(counts)).sum())
    for _ in range(ENC_TAIL):
        add("fill", 1, ENC_FILL)
    lay = lay_of()
    size = np.full(len(counts), fill, np.int64)
    for first, last in mixes:
        size[first - 1:last] = _enc_sizes(lay, first - 1, last)
    lay.update(kind=kinds, size=size, off=np.concatenate([[0], np.cumsum(size)]).astype(np.uint64), mixes=mixes)
    _enc_layout = lay
    return lay
