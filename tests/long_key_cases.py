"""Inputs of the long-key lookup tests (pure Python and the oracle, fixed seeds): keys and
needles longer than one 16-byte compare window, for lsm_point_read_blocks, lsm_seek_blocks,
lsm_table_get and lsm_table_range.  tests/test_long_key_cases.py asserts on the CPU that the
inputs hold what they were built for (coverage()), so that tests/test_gpu_lookup_long_keys.py
cannot pass vacuously.

Keys: for every stem length of STEM_LENS a random stem over ALPHABET and, for every position d
of positions(len), the stem with byte d bumped by one (0xFF, which has no successor, is
lowered to 0xFE), that key cut after d + 1 bytes, and the stem cut to d bytes.  Sorted, a
family reads  stem[:d] < stem < bumped[:d + 1] < bumped  for every d: neighbours that differ
first at byte d, and neighbours of which one is a strict prefix of the other.
Needles: every key, key + b"\\0", key[:-1], and the key with byte 15, 16, 17 or its last byte
XOR 0x80 or decremented (mod 256); the empty needle; huge_needle(), 70,000 bytes, longer than
any key can be.
"""
import bisect
import functools
import random

import numpy as np

import pyoracle
from table_get_model import TableModel, with_filter
from table_range_model import RangeModel

ALPHABET = bytes([0x00, 0x61, 0x7F, 0x80, 0xFF])
STEM_LENS = (15, 16, 17, 31, 32, 33, 47, 48, 49, 64, 127, 128, 129, 239, 240, 241, 255, 256, 257, 300)
RESTART_INTERVALS = (1, 3, 16)
HASH_RATIOS = (0.0, 1.33)
SNAP_ALL = 1 << 63   # _run of test_gpu_point_read clamps it to 2^63 - 1: every seqno here is below
TABLE_SNAP = 1 << 62
HUGE = 70000
CLASSES = ((0, 16), (17, 128), (129, 240), (241, 1 << 32))  # needle lengths by XXH3 path
HASH_FREE, HASH_CONFLICT = 254, 255
TABLE_ARGS = dict(block_size=512, restart_interval=4, hash_ratio=1.33, partition_size=256)


def positions(n):
    return sorted(d for d in {0, 1, 7, 8, 15, 16, 17, 31, 32, 33, n - 17, n - 16, n - 1} if 0 <= d < n)


@functools.lru_cache(maxsize=None)
def keys():
    """The distinct keys, sorted."""
    rng = random.Random(0x10E6)
    out = set()
    for n in STEM_LENS:
        stem = bytes(rng.choice(ALPHABET) for _ in range(n))
        out.add(stem)
        for d in positions(n):
            bumped = stem[:d] + bytes([stem[d] + 1 if stem[d] != 0xFF else 0xFE]) + stem[d + 1:]
            out |= {bumped, bumped[:d + 1], stem[:d]}
    return sorted(out)


@functools.lru_cache(maxsize=None)
def rows():
    """[(key, value, seqno, vtype)] in table order: 1-5 versions per key, seqnos descending,
    a quarter tombstones, values of 0-20 bytes."""
    rng = random.Random(0x10E7)
    out = []
    for k in keys():
        for s in sorted(rng.sample(range(1, 1000), rng.randint(1, 5)), reverse=True):
            tomb = rng.random() < 0.25
            out.append((k, b"" if tomb else bytes(rng.getrandbits(8) for _ in range(rng.randint(0, 20))), s,
                        1 if tomb else 0))
    return out


@functools.lru_cache(maxsize=None)
def items():
    return pyoracle.Items.from_list(rows())


def near_misses(k):
    out = {k, k + b"\0", k[:-1]}
    for p in {15, 16, 17, len(k) - 1}:
        if 0 <= p < len(k):
            out.add(k[:p] + bytes([k[p] ^ 0x80]) + k[p + 1:])
            out.add(k[:p] + bytes([(k[p] - 1) & 0xFF]) + k[p + 1:])
    return out


@functools.lru_cache(maxsize=None)
def needles():
    """The distinct needles, sorted (the empty one first); huge_needle() is not among them."""
    out = {b""}
    for k in keys():
        out |= near_misses(k)
    return sorted(out)


def huge_needle(head):
    """70,000 bytes that begin with head: above every key that head is not below."""
    return head + bytes((i * 7 + 3) & 0xFF for i in range(HUGE - len(head)))


# ---- the blocks of the point-read and seek tests
@functools.lru_cache(maxsize=None)
def block_starts():
    """Block cuts of 1-40 items: versions of one key straddle blocks."""
    rng = random.Random(0x10E8)
    starts = [0]
    while starts[-1] < len(rows()):
        starts.append(min(len(rows()), starts[-1] + rng.randint(1, 40)))
    return np.array(starts, np.uint32)


@functools.lru_cache(maxsize=None)
def blocks(ri, ratio):
    """(buf, off) of the oracle's encoding of the items at the cuts of block_starts()."""
    return pyoracle.encode_blocks(items(), block_starts(), restart_interval=ri, hash_ratio=ratio)


def payload(buf, off, b):
    return bytes(buf[int(off[b]) + 33:int(off[b + 1])])


def near(first_key, last_key, margin=2):
    """The needles that sort within [first_key, last_key] and the `margin` next to it on each side."""
    n = needles()
    return n[max(0, bisect.bisect_left(n, first_key) - margin):bisect.bisect_right(n, last_key) + margin]


@functools.lru_cache(maxsize=None)
def block_needles():
    """Per block of block_starts(): the needles near its key range."""
    r, s = rows(), block_starts()
    return [near(r[int(s[b])][0], r[int(s[b + 1]) - 1][0]) for b in range(len(s) - 1)]


@functools.lru_cache(maxsize=None)
def point_queries():
    """[(block, needle, snapshot)]: per block every needle near it at SNAP_ALL and each of its
    own keys at seqno + 1 and at seqno; the empty needle on the first and a middle block, the
    huge needle behind the last block's largest key."""
    r, s = rows(), block_starts()
    nb = len(s) - 1
    qs = []
    for b, ns in enumerate(block_needles()):
        qs += [(b, n, SNAP_ALL) for n in ns]
        for i in range(int(s[b]), int(s[b + 1])):
            qs += [(b, r[i][0], r[i][2] + 1), (b, r[i][0], r[i][2])]
    qs += [(0, b"", SNAP_ALL), (nb // 2, b"", SNAP_ALL), (nb - 1, huge_needle(r[-1][0]), SNAP_ALL)]
    return qs


@functools.lru_cache(maxsize=None)
def seek_queries():
    """[(block, lo, hi, flags)]: per block every needle near it paired with a second bound drawn
    from the same needles (the needle is the lower bound of every other pair, so about half the
    pairs are crossed), each pair under all 16 flag values, in that order: query 16 * p + f is
    pair p under flags f.  The last pair is the huge needle on the last block."""
    rng = random.Random(0x10E9)
    qs = []
    p = 0
    for b, ns in enumerate(block_needles()):
        for n in ns:
            other = rng.choice(ns)
            lo, hi = (n, other) if p % 2 == 0 else (other, n)
            qs += [(b, lo, hi, f) for f in range(16)]
            p += 1
    nb = len(block_starts()) - 1
    huge = huge_needle(rows()[-1][0])
    qs += [(nb - 1, huge, huge, f) for f in range(16)]
    return qs


def one_flag_per_pair(qs):
    """Of seek_queries(): pair p under flags p % 16 only."""
    return [qs[16 * p + p % 16] for p in range(len(qs) // 16)]


# ---- the tables of the table_get and table_range tests
@functools.lru_cache(maxsize=None)
def table(two_level, filtered):
    """(file, table dict, filter handle or None) of one of the four table variants."""
    t = pyoracle.table_write(items(), two_level=two_level, **TABLE_ARGS)
    file, flt = with_filter(t, items()) if filtered else (t["file"], None)
    return file, dict(t, two_level=two_level), flt


def get_queries_of(r, ns):
    """Every needle at TABLE_SNAP, every row's key at seqno + 1, seqno and 0, and the huge needle
    behind the largest key."""
    qs = [(n, TABLE_SNAP) for n in ns]
    for k, _, s, _ in r:
        qs += [(k, s + 1), (k, s), (k, 0)]
    return qs + [(huge_needle(r[-1][0]), TABLE_SNAP)]


@functools.lru_cache(maxsize=None)
def get_queries():
    return get_queries_of(rows(), needles())


@functools.lru_cache(maxsize=None)
def get_expected(two_level, filtered):
    file, t, flt = table(two_level, filtered)
    model = TableModel(file, t["tli_off"], t["tli_size"], two_level, filter=flt)
    return [model.lookup(k, s) for k, s in get_queries()]


@functools.lru_cache(maxsize=None)
def range_queries():
    """[(lo, hi, lo_excl, hi_excl)], None = unbounded.  Every present key and every seventh
    needle (absent neighbours, strict prefixes) n[i] as the lower bound with n[i + d], d in 0, 1, 9
    and -3 (crossed), as the upper, under the four flag values that keep both bounds.  The drain
    model reads every block between the bounds, so the twelve flag values that drop a bound (the
    range then runs to the table's end) are given to every 80th such pair only, and three
    table-wide pairs close the list."""
    n = needles()
    present = set(keys())
    qs = []
    for j, i in enumerate(i for i in range(3, len(n) - 9) if i % 7 == 0 or n[i] in present):
        for d in (0, 1, 9, -3):
            for le in (False, True):
                for he in (False, True):
                    qs.append((n[i], n[i + d], le, he))
        if j % 80 == 0:
            for f in range(16):
                if f & 3 != 3:
                    qs.append((n[i] if f & 1 else None, n[i + 9] if f & 2 else None, bool(f & 4), bool(f & 8)))
    huge = huge_needle(rows()[-1][0])
    qs += [(b"", huge, False, False), (huge, None, False, False), (n[1], n[-1], True, True)]
    return qs


@functools.lru_cache(maxsize=None)
def range_expected(two_level):
    file, t, _ = table(two_level, False)
    model = RangeModel(file, t["tli_off"], t["tli_size"], two_level)
    return [model.answer(*q) for q in range_queries()]


# ---- the u16 limit: keys of 65,534 and 65,535 bytes
U16_STEM = b"\x80" * 65535


def u16_rows():
    return [(U16_STEM[:65534], b"short", 9, 0), (U16_STEM[:65534] + b"\x7f", b"low", 8, 0),
            (U16_STEM, b"full", 7, 0), (U16_STEM, b"", 5, 1)]


def u16_needles():
    """The four row keys' near misses (key + b"\\0" is longer than a key can be) and the huge needle."""
    out = {b""}
    for k, *_ in u16_rows():
        out |= near_misses(k)
    return sorted(out) + [huge_needle(U16_STEM)]


@functools.lru_cache(maxsize=None)
def u16_blocks():
    """(buf, off) of the four rows as one block at restart interval 1 and one at 2, both with a
    hash index.  At interval 2 row 1 shares 65,534 bytes with its head, and row 3 shares 65,535
    and has a zero-byte suffix."""
    it = pyoracle.Items.from_list(u16_rows())
    blks = [pyoracle.block_write(pyoracle.data_block_encode(it, restart_interval=ri, hash_ratio=1.33)) for ri in (1, 2)]
    off = np.zeros(3, np.uint64)
    off[1:] = np.cumsum([len(b) for b in blks])
    return np.frombuffer(b"".join(blks), np.uint8).copy(), off


def u16_point_queries():
    qs = []
    for b in (0, 1):
        for k, _, s, _ in u16_rows():
            qs += [(b, k, s + 1), (b, k, s), (b, k, SNAP_ALL), (b, k, 0)]
        qs += [(b, n, SNAP_ALL) for n in u16_needles()]
    return qs


def u16_bound_pairs():
    """(lo, hi) around the row keys: neighbouring distinct keys both ways round, each key with
    itself, with key + b"\\0" and with key[:-1], and the huge needle as either bound."""
    k = sorted({r[0] for r in u16_rows()})
    huge = huge_needle(U16_STEM)
    pairs = list(zip(k, k[1:])) + list(zip(k[1:], k)) + [(x, x) for x in k] + [(x, x + b"\0") for x in k]
    return pairs + [(x[:-1], x) for x in k] + [(huge, huge), (k[-1], huge), (huge, k[0])]


def u16_seek_queries():
    """[(block, lo, hi, flags)]: u16_bound_pairs() under all 16 flag values on both blocks.  A
    bound its flags do not use is sent empty (the arenas stay small)."""
    return [(b, lo if f & 1 else b"", hi if f & 2 else b"", f)
            for b in (0, 1) for lo, hi in u16_bound_pairs() for f in range(16)]


@functools.lru_cache(maxsize=None)
def u16_table():
    """The four rows as a two-level table: one row per data block, one handle per partition, so
    every index block holds end keys at the u16 limit."""
    it = pyoracle.Items.from_list(u16_rows())
    t = pyoracle.table_write(it, two_level=True, **TABLE_ARGS)
    return t["file"], dict(t, two_level=True)


def u16_get_queries():
    return get_queries_of(u16_rows(), u16_needles()[:-1])


def u16_range_queries():
    return [(lo if f & 1 else None, hi if f & 2 else None, bool(f & 4), bool(f & 8))
            for lo, hi in u16_bound_pairs() for f in range(16)]


# ---- what the inputs hold
def window(sorted_keys, lo, hi, lo_excl=False, hi_excl=False):
    """[a, b) of a sorted key list inside the bounds (None = unbounded), by bisection."""
    a = 0 if lo is None else (bisect.bisect_right if lo_excl else bisect.bisect_left)(sorted_keys, lo)
    b = len(sorted_keys) if hi is None else (bisect.bisect_left if hi_excl else bisect.bisect_right)(sorted_keys, hi)
    return a, max(a, b)


def common_prefix(a, b):
    n = 0
    while n < min(len(a), len(b)) and a[n] == b[n]:
        n += 1
    return n


def bucket_of(pl, needle):
    """The hash-index bucket value a point read of needle finds in payload pl (None: no hash index)."""
    tr = len(pl) - 31
    hash_len = int.from_bytes(pl[tr + 10:tr + 14], "little")
    hash_off = int.from_bytes(pl[tr + 14:tr + 18], "little")
    return pyoracle.hash_index_get(pl[hash_off:hash_off + hash_len], needle) if hash_len else None


def coverage():
    """The counts behind the coverage conditions, each asserted here on the oracle's own output."""
    c = {"keys": len(keys()), "items": len(rows()), "needles": len(needles()), "blocks": len(block_starts()) - 1}
    k = keys()
    spans = {"[16,32)": 0, "[32,128)": 0, "[128,256)": 0, ">=256": 0}
    prefix_pairs = 0
    for a, b in zip(k, k[1:]):
        n = common_prefix(a, b)
        for name, lo, hi in (("[16,32)", 16, 32), ("[32,128)", 32, 128), ("[128,256)", 128, 256), (">=256", 256, 1 << 20)):
            spans[name] += lo <= n < hi
        prefix_pairs += n == len(a) >= 16
    c["adjacent common prefix"] = spans
    c["adjacent strict-prefix pairs, shorter >= 16"] = prefix_pairs
    assert all(v >= 1 for v in spans.values()) and prefix_pairs >= 20, (spans, prefix_pairs)

    for ri in (3, 16):
        parsed, _, status = pyoracle.decode_blocks(*blocks(ri, 1.33))
        assert (status == 0).all()
        p16, p128 = int((parsed["prefix_len"] >= 16).sum()), int((parsed["prefix_len"] >= 128).sum())
        c["prefix_len >= 16 / >= 128 at interval %d" % ri] = (p16, p128)
        assert p16 >= 200 and p128 >= 50, (ri, p16, p128)

    qs = point_queries()
    buckets = {cl: {"interval": 0, "free": 0, "conflict": 0} for cl in CLASSES}
    hits = 0
    for ri in RESTART_INTERVALS:
        buf, off = blocks(ri, 1.33)
        pls = [payload(buf, off, b) for b in range(len(off) - 1)]
        for b, needle, snap in qs:
            m = bucket_of(pls[b], needle)
            cl = next(cl for cl in CLASSES if cl[0] <= len(needle) <= cl[1])
            buckets[cl]["free" if m == HASH_FREE else "conflict" if m == HASH_CONFLICT else "interval"] += 1
            if ri == 3:
                hits += pyoracle.point_read(pls[b], needle, min(snap, SNAP_ALL - 1)) >= 0
    c["point-read buckets by needle class"] = buckets
    for cl, n in buckets.items():
        assert n["interval"] >= 20 and n["free"] >= 5 and n["conflict"] >= 5, (cl, n)
    c["point-read queries / hits"] = (len(qs), hits)
    assert 10 * hits >= len(qs), (hits, len(qs))

    residues, at = set(), 0
    for _, needle, _ in qs:
        if len(needle) >= 33:
            residues.add(at % 16)
        at += len(needle)
    c["start residues of needles >= 33 bytes"] = len(residues)
    assert residues == set(range(16)), residues
    return c
