"""Inputs of the lsm_merge_runs tests that aim at one edge each (pure Python, fixed
seeds; every generator returns a list of runs of (key, value, seqno, vtype) items).
tests/test_merge_cases.py asserts on the CPU that each set still has the property it
was built for; the test_gpu_merge_*.py files run them on the device."""
import itertools
import random

from merge_gpu import deal, sort_run

SEG = 64          # kMergeSeg (csrc/merge.hip): items of one run per segment, merged positions per gather step
MERGE_BUF = 8192  # kMergeBuf: a step's span (+ its pad) up to this size is assembled in LDS
MERGE_LONG = 256  # kMergeLong: keys / values from this length on are copied by the whole wave
FLAG_PAIRS = ((False, False), (True, False), (False, True), (True, True))


# ---------------------------------------------------------------- full-width seqnos
WIDE_BASES = (0, 2 ** 31 - 2, 2 ** 32 - 2, 2 ** 63 - 2, 2 ** 64 - 5)
WIDE_THRESHOLDS = (0, 2 ** 32, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1)
HIGH_DWORD_PAIR = (7 << 32 | 5, 3 << 32 | 9)  # ordered by the high dword; the low dwords order them the other way
BIT63_PAIR = (2 ** 63 + 1, 2 ** 63 - 1)       # ordered as unsigned; as signed the first is negative
WIDE_SINGLES = (2 ** 32 - 1, 2 ** 32, 2 ** 63 - 2, 2 ** 63 - 1, 2 ** 63)  # one-version keys: zeroed or not by thr alone


def wide_seqnos():
    """40 keys with versions at base + 0..3 around 0, 2^31, 2^32, 2^63 and 2^64, one key whose
    versions differ only in the high dword, one whose versions straddle bit 63 and five keys of
    one version each next to the thresholds (zero_seqnos decides on them alone); 3 runs."""
    rng = random.Random(4001)
    items = []
    for k in range(40):
        for base in WIDE_BASES:
            for d in range(4):
                t = rng.choice((0, 0, 1, 2, 4))
                items.append((b"wide%03d" % k, b"" if t in (1, 2) else b"%d+%d" % (base, d), base + d, t))
    for s in HIGH_DWORD_PAIR:
        items.append((b"x-high-dword", b"%x" % s, s, 0))
    for s in BIT63_PAIR:
        items.append((b"y-bit-63", b"%x" % s, s, 0))
    for s in WIDE_SINGLES:
        items.append((b"z-single-%x" % s, b"%x" % s, s, 0))
    rng.shuffle(items)
    return deal(rng, items, 3)


# ------------------------------------------------------------------------ long ties
TIE_KEY = b"tie/a-key-longer-than-the-head"  # > 16 bytes: every comparison goes through cmp_key_tail
TIE_SEQ = 77


def _ties(r, n):
    return [(TIE_KEY, b"run %d item %d" % (r, i), TIE_SEQ, 0) for i in range(n)]


def long_ties(lens=(200, 130, 65)):
    """One key, one seqno: runs of 200, 130 and 65 equal items, the values naming (run, index)."""
    return [_ties(r, n) for r, n in enumerate(lens)]


def long_ties_orders():
    """long_ties() with the three run lengths in every order."""
    return [long_ties(p) for p in itertools.permutations((200, 130, 65))]


def long_ties_embedded():
    """A stretch of equal items between ordinary keys, starting and ending inside a segment
    in every run (37 + 260, 10 + 250 and 50 + 65 items, then the larger keys)."""
    rng = random.Random(4002)
    runs = []
    for r, (before, ties, after) in enumerate(((37, 260, 51), (10, 250, 70), (50, 65, 30))):
        lo = [(b"before%04d" % rng.randrange(400), b"b%d" % r, rng.randrange(100), 0) for _ in range(before)]
        hi = [(b"z-after%04d" % rng.randrange(400), b"a%d" % r, rng.randrange(100), 0) for _ in range(after)]
        runs.append(sort_run(lo) + _ties(r, ties) + sort_run(hi))
    return runs


def long_ties_64_runs():
    """64 runs of 3 equal items each."""
    return [_ties(r, 3) for r in range(64)]


def whole_tie_segments(run):
    """Number of whole 64-item segments of the run that hold nothing but the tie stretch."""
    return sum(all(it[0] == TIE_KEY and it[2] == TIE_SEQ for it in run[s:s + SEG])
               for s in range(0, len(run) - SEG + 1, SEG))


# --------------------------------------------------------------------- shared heads
HEAD16 = b"sixteen-byte-hd:"
PREFIX32 = b"a-prefix-of-thirty-two-bytes-....:"[:32]
HEAD_POSITIONS = {16: (16, 23, 24, 25, 31, 32, 33), 32: (32, 33, 39, 40, 41, 47, 48, 49)}
HEAD_LETTERS = {16: b"ab", 32: b"\x7f\x80"}  # (the second pair is ordered wrongly by a signed byte compare)


def shared_head_keys(head_len):
    """About 500 keys: the common head (HEAD16 or PREFIX32), then a suffix of 0..30 bytes over
    two letters.  Random suffixes, plus for every position p of HEAD_POSITIONS a pair that
    agrees up to byte p and differs there, and a key with its one-byte extension."""
    head = {16: HEAD16, 32: PREFIX32}[head_len]
    assert len(head) == head_len
    lo, hi = HEAD_LETTERS[head_len]
    rng = random.Random(4003 + head_len)
    word = lambda n: bytes(rng.choice((lo, hi)) for _ in range(n))
    keys = {head}
    while len(keys) < 470:
        keys.add(head + word(rng.randint(0, 30)))
    for p in HEAD_POSITIONS[head_len]:
        stem = word(p - head_len)
        keys.add(head + stem + bytes([lo]) + word(rng.randint(0, 30 - (p - head_len) - 1)))
        keys.add(head + stem + bytes([hi]) + word(rng.randint(0, 30 - (p - head_len) - 1)))
    stem = word(22)
    keys.update((head + stem, head + stem + bytes([lo])))
    return sorted(keys)


def shared_heads(head_len):
    """3000 items over shared_head_keys(head_len), 5 runs."""
    rng = random.Random(4004 + head_len)
    keys = shared_head_keys(head_len)
    items = []
    for i in range(3000):
        t = rng.choice((0, 0, 0, 1, 2, 4))
        items.append((rng.choice(keys), b"" if t in (1, 2) else b"v%d" % i, rng.randrange(1000), t))
    return deal(rng, items, 5)


def first_difference(a, b):
    """Index of the first byte at which a and b differ, or None when one is a prefix of the other."""
    for p in range(min(len(a), len(b))):
        if a[p] != b[p]:
            return p
    return None


# ------------------------------------------------------------ state between calls
def state_sorted():
    rng = random.Random(4005)
    items = []
    for i in range(900):
        t = rng.choice((0, 0, 0, 1, 2, 4))
        items.append((b"state%04d" % rng.randrange(300), b"" if t in (1, 2) else rng.randbytes(rng.randrange(60)),
                      rng.randrange(1000), t))
    return deal(rng, items, 3)


def state_unsorted():
    """state_sorted() with two unequal neighbours of run 1 swapped (the runs' lengths are kept)."""
    runs = [list(r) for r in state_sorted()]
    run = runs[1]
    k = next(i for i in range(len(run) // 2, len(run) - 1)
             if (run[i][0], -run[i][2]) != (run[i + 1][0], -run[i + 1][2]))
    run[k], run[k + 1] = run[k + 1], run[k]
    return runs


def state_one_run():
    rng = random.Random(4006)
    return [sort_run([(b"one%03d" % rng.randrange(90), b"v%d" % i, rng.randrange(1000), rng.choice((0, 1, 4)))
                      for i in range(200)])]


def state_second():
    """Another sorted merge, of another shape (2 runs, longer keys), for the second stream."""
    rng = random.Random(4007)
    items = [(b"second-stream/%05d" % rng.randrange(250), rng.randbytes(rng.randrange(30)), rng.randrange(1000),
              rng.choice((0, 0, 1, 4))) for _ in range(600)]
    return deal(rng, items, 2)


def malformed_run_starts(run_start):
    """name -> (run_start, per-run statuses by merge_setup_kernel's rule) for 3 runs.  Run r is
    rejected (10) when not s <= e <= n_items, or r is the first run and s != 0, or r is the last
    run and e != n_items, with s, e = run_start[r], run_start[r + 1]; every other run is 0."""
    z, a, b, n = run_start
    assert z == 0 < a < b < n
    return {
        "first_not_zero": ([1, a, b, n], [10, 0, 0]),
        "last_not_n_items": ([0, a, b, n - 1], [0, 0, 10]),
        "last_above_n_items": ([0, a, b, n + 3], [0, 0, 10]),
        "decreasing_pair": ([0, b, a, n], [0, 10, 0]),        # run 1 = [b, a): s > e
        "entry_above_n_items": ([0, a, n + 5, n], [0, 10, 10]),  # run 1 ends past n, run 2 starts past its end
    }


# ------------------------------------------------------------------ output extents
def nothing_dropped():
    """Distinct (key, seqno) everywhere and no tombstone: with thr = 0 the output is the input."""
    rng = random.Random(4008)
    items = [(b"keep%04d" % (i // 3) + b"x" * (i % 23), rng.randbytes((i * 37) % 150), i % 3, rng.choice((0, 4)))
             for i in range(700)]
    rng.shuffle(items)
    return deal(rng, items, 3)


def half_dropped():
    """Many versions per key and a mid threshold: about half of the items are dropped."""
    rng = random.Random(4009)
    items = []
    for i in range(800):
        t = rng.choice((0, 0, 0, 1, 2, 4))
        items.append((b"half%03d" % (k := rng.randrange(80)) + b"y" * (k % 9),
                      b"" if t in (1, 2) else rng.randbytes(rng.randrange(120)), rng.randrange(1000), t))
    return deal(rng, items, 3)


HALF_DROPPED_THR = 600


def span_limit(total, pad, field="vals"):
    """Merged positions 64 .. 127 (one gather step) hold 64 values (or, field="keys", 64 keys) of
    `total` bytes together (64 x 128 with the last one shortened or lengthened); the bytes of
    the step before are `pad` mod 16, so the step's first output byte sits `pad` bytes past a
    16-byte boundary.  Nothing is dropped (thr = 0, one version per key); two runs, dealt
    alternately."""
    assert 0 <= pad < 16 and abs(total - MERGE_BUF) < 100
    lens = [16] * 63 + [16 + pad] + [128] * 63 + [128 + total - MERGE_BUF] + [40] * 30
    if field == "keys":
        items = [(b"%04d" % i + bytes([i & 0xff]) * (n - 4), b"v%d" % i, 5, 0) for i, n in enumerate(lens)]
    else:
        items = [(b"span%04d" % i, bytes([i & 0xff]) * n, 5, 0) for i, n in enumerate(lens)]
    return [items[0::2], items[1::2]]


def mixed_keys():
    """Keys of 250..320 bytes next to keys of 1..20 bytes in merged order (they alternate),
    3 or 4 versions of each, 3 runs."""
    rng = random.Random(4010)
    items = []
    for i in range(120):
        first = bytes([1 + i])
        n = rng.randint(250, 320) if i & 1 else rng.randint(1, 20)
        key = first + bytes(rng.choice(b"kl") for _ in range(n - 1))
        for _ in range(rng.randint(3, 4)):
            t = rng.choice((0, 0, 1, 2, 4))
            v = b"" if t in (1, 2) else rng.randbytes(rng.choice((0, 3, 17, 40, 300)))
            items.append((key, v, rng.randrange(100), t))
    return deal(rng, items, 3)


MIXED_KEYS_THR = 50


# ---------------------------------------------------------------------- graph replay
def graph_sets():
    """(first, second, second_unsorted): data sets of one item count and one size of each arena
    (10-byte keys; item i of the flat input has (13 i) mod 60 value bytes), 3 runs of fixed
    lengths, so that one may overwrite another in place."""
    lens = (300, 180, 220)

    def one(seed):
        rng = random.Random(seed)
        runs, at = [], 0
        for n in lens:
            # sorting moves the values with their items, so the lengths are set afterwards, by position
            run = sort_run([(b"g%d/%07d" % (seed % 10, rng.randrange(260)), b"", rng.randrange(1000),
                             rng.choice((0, 0, 1, 2, 4))) for _ in range(n)])
            runs.append([(k, rng.randbytes(13 * (at + j) % 60), s, t) for j, (k, _, s, t) in enumerate(run)])
            at += n
        return runs

    first, second = one(4011), one(4012)
    bad = [list(r) for r in second]
    run = bad[2]
    k = next(i for i in range(100, len(run) - 1) if (run[i][0], -run[i][2]) != (run[i + 1][0], -run[i + 1][2]))
    run[k], run[k + 1] = (run[k + 1][0], run[k][1], run[k + 1][2], run[k + 1][3]), \
                         (run[k][0], run[k + 1][1], run[k][2], run[k][3])  # (the values stay: their lengths go by position)
    return first, second, bad


GRAPH_THR = 500

