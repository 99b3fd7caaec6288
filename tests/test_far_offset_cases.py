"""CPU checks of the fixtures in tests/far_offsets.py, so that the GPU tests of offsets past
2 GiB and 4 GiB cannot pass vacuously: the batch holds every block class, every placement puts
the line where it claims, the alias regions lie inside the arena and touch nothing placed, the
relocated table answers the CPU models as the compact one does, and the encode layout has small
blocks on both sides of both lines."""
import numpy as np
import pytest

import far_offsets as F
import pyoracle
from table_get_model import GET_HIT, TableModel, mvcc_queries, mvcc_table
from table_range_model import RANGE_ROWS, RangeModel, mvcc_range_queries

OK, CKSUM, PARSE = 0, 4, 5


def test_batch_holds_every_block_class():
    b = F.batch()
    classes, blocks = b["classes"], b["blocks"]
    payload = [len(x) - 33 for x in blocks]
    assert classes.count("small") == 20 and all(payload[i] <= 4096 for i, c in enumerate(classes) if c == "small")
    # restart intervals 1 and 16, with and without a hash index, among the small blocks
    shapes = set()
    for i, c in enumerate(classes):
        if c == "small":
            tr = blocks[i][-31:]
            shapes.add((tr[0], int.from_bytes(tr[10:14], "little") > 0))
    assert shapes == {(1, False), (1, True), (16, False), (16, True)}
    one = {c: payload[classes.index(c)] for c in ("prefix16k", "big", "huge", "index", "cksum", "parse", "tomb")}
    assert 14 << 10 <= one["prefix16k"] <= 18 << 10
    assert F.LDS_STAGE < one["big"] <= 0xFFFF
    assert one["huge"] > F.HUGE_PAYLOAD
    assert blocks[classes.index("index")][4] == 1
    assert 380 << 10 <= len(b["buf"]) <= 640 << 10
    _, _, status = pyoracle.decode_blocks(b["buf"], b["off"])
    want = np.zeros(len(blocks), np.int32)
    want[classes.index("cksum")], want[classes.index("parse")] = CKSUM, PARSE
    assert status.tolist() == want.tolist()
    # the tombstone / full-width seqno block
    items = b["items"][classes.index("tomb")]
    assert (items.vtype != 0).any() and int(items.seqno.max()) >= 1 << 62
    # block k once in the middle of a small-block group, once the largest block
    ks, kl = b["k_small"], b["k_largest"]
    assert all(c == "small" for c in classes[ks - 2:ks + 3])
    assert len(blocks[kl]) == max(len(x) for x in blocks) and classes[kl] == "huge"


@pytest.mark.parametrize("name,line,k,kind,base", F.placements(), ids=[p[0] for p in F.placements()])
def test_placement_puts_the_line_where_it_claims(name, line, k, kind, base):
    b = F.batch()
    off = [int(o) for o in b["off"]]
    lo, hi = base + off[k], base + off[k + 1]
    if kind == "inside":
        assert lo + F.MARGIN <= line <= hi - F.MARGIN and base % 16 != 0
        assert 0 < k < len(off) - 2  # blocks below, around and above the line
    elif kind == "at":
        assert lo == line and 0 < k
    else:
        assert base == F.L32 + (1 << 20) + 5 and base + off[0] > F.L32
    lay = F.layout([(off[i], off[i + 1] - off[i]) for i in range(len(off) - 1)], base)
    assert lay["placed"][0][0] == base and len(lay["placed"]) == len(off) - 1
    assert lay["guards"] == [(base - F.GUARD, F.GUARD), (base + off[-1], F.GUARD)]
    # every piece part at or above a line has its alias, 2^32 and 2^31 lower, inside the arena
    want = []
    for o, n in lay["placed"]:
        for d in (F.L32, F.L31):
            if o + n > d:
                want.append((max(o, d) - d, o + n - max(o, d)))
    assert lay["aliases"] == want and len(want) > 0
    if line == F.L32:
        assert any(a[0] < (1 << 26) for a in want) and any(a[0] >= F.L31 - (1 << 26) for a in want)
    for o, n in lay["aliases"] + lay["guards"] + lay["placed"]:
        assert 0 <= o and o + n <= F.ARENA_BYTES
    assert F.overlaps(lay["aliases"], lay["placed"] + lay["guards"]) == []


def _subset(queries, step):
    return queries[::step]


@pytest.mark.parametrize("two_level", [False, True], ids=["full", "two_level"])
def test_relocated_table_answers_as_the_compact_one(two_level):
    """relocate_table with a small D, as real host bytes: table_get_model and table_range_model
    give the compact table's answers with every file offset passed through the map."""
    items, t = mvcc_table(1, two_level)
    D = 12345
    r = F.relocate_table(t["file"], t, D, two_level)
    file = F.materialize_file(r)
    assert r["two_level"] == two_level and len(file) == r["file_len"] > len(t["file"]) + D - 1
    off = [int(o) for o in t["block_off"]]
    assert [r["map"][o] for o in off[:-1]] == [o + D for o in off[:-1]]
    assert r["block_off"].tolist() == [o + D for o in off]
    for o, p in r["pieces"]:  # back to back from D, nothing overlapping
        assert file[o:o + len(p)] == p
    ends = sorted((o, o + len(p)) for o, p in r["pieces"])
    assert ends[0][0] == D and all(a[1] == b[0] for a, b in zip(ends, ends[1:])) and ends[-1][1] == r["file_len"]
    get0 = TableModel(t["file"], t["tli_off"], t["tli_size"], two_level)
    get1 = TableModel(file, r["tli_off"], r["tli_size"], two_level)
    hits = 0
    for needle, snap in _subset(mvcc_queries(items, 1), 5):
        st, e = get0.lookup(needle, snap)
        if e[0] == GET_HIT:
            e = (e[0], r["map"][e[1]]) + e[2:]
            hits += 1
        assert get1.lookup(needle, snap) == (st, e)
    assert hits > 100
    rng0 = RangeModel(t["file"], t["tli_off"], t["tli_size"], two_level)
    rng1 = RangeModel(file, r["tli_off"], r["tli_size"], two_level)
    rows = 0
    for q in _subset(mvcc_range_queries(1, two_level), 10):
        st, e = rng0.answer(*q)
        if e[0] == RANGE_ROWS:
            e = (e[0], r["map"][e[1]], e[2], e[3], r["map"][e[4]], e[5], e[6])
            rows += 1
        assert rng1.answer(*q) == (st, e)
    assert rows > 40


@pytest.mark.parametrize("two_level", [False, True], ids=["full", "two_level"])
def test_table_shifts_put_the_line_inside_a_data_and_an_index_block(two_level):
    _, t = mvcc_table(1, two_level)
    off = [int(o) for o in t["block_off"]]
    for where in ("data", "index"):
        D = F.table_shift(t["file"], t, where)
        r = F.relocate_table(t["file"], t, D, two_level)
        o, n = F.block_holding(r, F.L32)
        assert (o < off[-1] + D) == (where == "data")
        if where == "index" and two_level:
            assert o != r["tli_off"]  # a partition, not the TLI
        assert F.L32 < r["file_len"] <= F.L32 + (4 << 20)
        lay = F.layout([(p[0], len(p[1])) for p in r["pieces"]], 0)
        for a, m in lay["aliases"]:
            assert 0 <= a and a + m <= F.ARENA_BYTES
        assert F.overlaps(lay["aliases"], lay["placed"] + lay["guards"]) == []


def test_encode_layout_has_small_blocks_on_both_sides_of_both_lines():
    """From sizes alone (no 4 GiB allocation): every kind of small block ends below and starts
    above 2^31 and 2^32 within 1.5 MiB of the line, a 4 KiB block holds each line strictly inside,
    and the batch ends about 8 MiB past 2^32."""
    lay = F.encode_layout()
    off, kind = [int(o) for o in lay["off"]], lay["kind"]
    assert len(kind) == len(lay["size"]) == len(lay["starts"]) - 1 and len(lay["val_len"]) == lay["starts"][-1]
    assert (np.diff(lay["off"]).astype(np.int64) == lay["size"]).all()
    for (first, last), line in zip(lay["mixes"], (F.L31, F.L32)):
        assert last - first == 2 * sum(h[0] for h in F.ENC_HALF) and 280 <= last - first <= 320
        assert abs(off[first] - (line - F.ENC_LEAD)) <= 64
        assert kind[first - 1] == "short" and kind[last] == "fill" and kind[first - 2] == "fill"
        for want in F.ENC_KINDS:
            below = [b for b in range(first, last) if kind[b] == want and off[b + 1] <= line]
            above = [b for b in range(first, last) if kind[b] == want and off[b] >= line]
            assert below and above, (line, want)
            assert line - off[below[0]] <= 3 << 19 and off[above[-1] + 1] - line <= 3 << 19
        k = next(b for b in range(first, last) if off[b] < line < off[b + 1])
        assert kind[k] == "4k" and off[k] + 64 <= line <= off[k + 1] - 64
    sizes = {want: [int(lay["size"][b]) for b in range(*lay["mixes"][0]) if kind[b] == want] for want in F.ENC_KINDS}
    assert max(sizes["4k"]) <= 4096 + 33 + 400 and 14 << 10 <= min(sizes["16k"]) <= max(sizes["16k"]) <= 18 << 10
    assert min(sizes["big"]) > (96 << 10) + 33
    per_block = np.diff(lay["starts"])
    assert all(per_block[b] >= 128 for b in range(*lay["mixes"][0]) if kind[b] == "run")
    assert F.L32 + (6 << 20) <= off[-1] <= F.L32 + (12 << 20)
    assert int(lay["val_len"].sum()) + off[-1] < 9 << 30  # the values and the output: about 9 GiB of device memory
