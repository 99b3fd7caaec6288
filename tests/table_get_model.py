"""Python restatement of Table::get (src/table/mod.rs:229-340) over the bytes of a
table file, the model lsm_table_get is checked against.  Built from the oracle's
primitives only: header_decode, data_block_decode(index=True) for index entries,
point_read, bloom_contains, xxh3_64.

The rules, in the reference's order:
  1. snap' = snapshot.saturating_sub(global_seqno); lowest_seqno >= snap' -> SEQNO_SKIP
     (mod.rs:239-243);
  2. the filter block (Header ‖ Bloom image, type Filter, mod.rs:267-289):
     contains_hash false -> FILTERED;
  3. index_block::Iter::seek (index_block/iter.rs:25-34 over Decoder::seek(pred, true),
     block/decoder.rs:210-304): binary search for the first entry failing
     end_key < needle || (end_key == needle && seqno >= snap'); FullBlockIndex
     (block_index/full.rs:23-30) seeks the TLI, TwoLevelBlockIndex
     (block_index/two_level.rs:110-173) the TLI and then every partition from there on,
     ending at a partition whose seek finds nothing;
  4. Table::point_read's loop (mod.rs:317-340): a hit ends it, a miss in a block whose
     end key is greater than the needle ends it, else the next handle.

Block headers are taken as verified upstream (lsm_table_get checks their fields, not
their checksums); header_decode here does check the header checksum, so a test that
edits a header field re-seals it (reseal_header).
"""
import random

import numpy as np

import pyoracle
from helpers import random_sorted_items

GET_NONE, GET_SEQNO_SKIP, GET_FILTERED, GET_NO_BLOCK, GET_MISS, GET_HIT = range(6)
OK, BAD_MAGIC, BAD_TYPE, PARSE, TYPE_MISMATCH, TRUNCATED, UNSUPPORTED = 0, 1, 2, 5, 7, 8, 9
DATA, INDEX, FILTER = 0, 1, 2
BLOOM_MAX_K = 65536
NO_HIT = (0, 0, -1, 0, 0, 0, 0)  # block_off, block_size, item, seqno, val_off, val_len, vtype of a non-hit


class TableError(Exception):
    """The status at which the reference's get returns Err."""

    def __init__(self, status):
        super().__init__(status)
        self.status = status


class TableModel:
    def __init__(self, file, tli_off, tli_size, two_level, filter=None, lowest_seqno=0, global_seqno=0):
        self.file = bytes(file)
        self.tli = (tli_off, tli_size)
        self.two_level = bool(two_level)
        self.filter = filter
        self.lowest_seqno = lowest_seqno
        self.global_seqno = global_seqno
        self._index = {}
        self._data = {}

    # ---- blocks
    def _load(self, off, size, want):
        """load_block (src/table/util.rs:79-86) of an uncompressed block -> payload."""
        if size < 33 or off + size > len(self.file):
            raise TableError(TRUNCATED)
        st, h = pyoracle.header_decode(self.file[off:off + 33])
        if st:
            raise TableError(st)
        if h.block_type != want:
            raise TableError(TYPE_MISMATCH)
        if h.data_length != size - 33:
            raise TableError(TRUNCATED)
        if want != FILTER and h.uncompressed_length != h.data_length:
            raise TableError(UNSUPPORTED)
        return self.file[off + 33:off + size]

    def index_entries(self, off, size):
        """[(end_key, seqno, block offset, block size)] of the index block at (off, size)."""
        if (off, size) not in self._index:
            payload = self._load(off, size, INDEX)
            n, p = pyoracle.data_block_decode(payload, index=True)
            if n < 0:
                raise TableError(PARSE)
            self._index[(off, size)] = [
                (payload[int(p["key_off"][i]):int(p["key_off"][i]) + int(p["key_len"][i])], int(p["seqno"][i]),
                 int(p["handle_off"][i]), int(p["val_len"][i])) for i in range(n)]
        return self._index[(off, size)]

    def data_block(self, off, size):
        """(payload, parsed fields) of the data block at (off, size) (load_data_block)."""
        if (off, size) not in self._data:
            payload = self._load(off, size, DATA)
            n, p = pyoracle.data_block_decode(payload)
            if n < 0:
                raise TableError(PARSE)
            self._data[(off, size)] = (payload, p)
        return self._data[(off, size)]

    # ---- the index
    @staticmethod
    def seek(entries, needle, snap):
        """index_block::Iter::seek: the first entry failing the predicate, len(entries) = none."""
        lo, hi = 0, len(entries)
        while lo < hi:
            mid = lo + (hi - lo) // 2
            key, seqno = entries[mid][0], entries[mid][1]
            if key < needle or (key == needle and seqno >= snap):
                lo = mid + 1
            else:
                hi = mid
        return lo

    def handles(self, needle, snap):
        """BlockIndex::forward_reader(needle, snap): yields (partition index, entry) in order."""
        tli = self.index_entries(*self.tli)
        if not self.two_level:
            for e in tli[self.seek(tli, needle, snap):]:
                yield 0, e
            return
        for pi in range(self.seek(tli, needle, snap), len(tli)):
            part = self.index_entries(tli[pi][2], tli[pi][3])
            at = self.seek(part, needle, snap)
            if at == len(part):
                return
            for e in part[at:]:
                yield pi, e

    def first_handle(self, needle, snap):
        """(partition index, block offset) of the first yielded handle, None if there is none."""
        for pi, e in self.handles(needle, snap):
            return pi, e[2]
        return None

    # ---- Table::get
    def lookup(self, needle, snapshot, key_hash=None):
        """-> (status, (outcome, block_off, block_size, item, seqno, val_off, val_len, vtype))."""
        try:
            return OK, self.get(needle, snapshot, key_hash)
        except TableError as e:
            return e.status, (GET_NONE,) + NO_HIT

    def get(self, needle, snapshot, key_hash=None):
        snap = max(snapshot - self.global_seqno, 0)
        if self.lowest_seqno >= snap:
            return (GET_SEQNO_SKIP,) + NO_HIT
        if self.filter is not None and self.filter[1]:
            image = self._load(self.filter[0], self.filter[1], FILTER)
            h = key_hash if key_hash is not None else pyoracle.xxh3_64(needle)
            r = pyoracle.bloom_contains(image, h) if len(image) >= pyoracle.BLOOM_HDR else -1
            if r < 0:
                raise TableError(BAD_MAGIC)  # Error::InvalidHeader("BloomFilter")
            if int.from_bytes(image[14:22], "little") > BLOOM_MAX_K:
                raise TableError(UNSUPPORTED)
            if r == 0:
                return (GET_FILTERED,) + NO_HIT
        read_any = False
        for _, (end_key, _, off, size) in self.handles(needle, snap):
            payload, p = self.data_block(off, size)
            item = pyoracle.point_read(payload, needle, snap)
            if item == -2:
                raise TableError(PARSE)
            read_any = True
            if item >= 0:
                seqno = (int(p["seqno"][item]) + self.global_seqno) & (2 ** 64 - 1)
                return (GET_HIT, off, size, item, seqno, int(p["val_off"][item]), int(p["val_len"][item]),
                        int(p["vtype"][item]))
            if end_key > needle:
                return (GET_MISS,) + NO_HIT
        return (GET_MISS if read_any else GET_NO_BLOCK,) + NO_HIT


# ---- builders
def item_key(items, i):
    return bytes(items.keys[int(items.key_off[i]):int(items.key_off[i + 1])])


def filter_block(items, bpk=10.0):
    """The filter block FullFilterWriter writes for a table (writer/filter/full.rs:47-92):
    unique user keys -> xxh3_64 -> Bloom image -> block of type Filter."""
    keys = sorted({item_key(items, i) for i in range(items.n)})
    hashes = np.array([pyoracle.xxh3_64(k) for k in keys], np.uint64)
    m, k = pyoracle.bloom_shape(len(keys), bpk=bpk)
    return pyoracle.block_write(pyoracle.bloom_build(hashes, m, k), block_type=FILTER)


def with_filter(table, items, bpk=10.0):
    """table_write's result with the filter block appended -> (file bytes, (off, size))."""
    blk = filter_block(items, bpk)
    return table["file"] + blk, (len(table["file"]), len(blk))


def index_block(entries):
    """An index block from explicit (end_key, seqno, off, size) entries, as
    pyoracle.table_write's inner index_block builds it."""
    it = pyoracle.Items(np.frombuffer(b"".join(e[0] for e in entries), np.uint8),
                        np.concatenate([[0], np.cumsum([len(e[0]) for e in entries])]).astype(np.uint64),
                        np.zeros(0, np.uint8), np.zeros(len(entries) + 1, np.uint64),
                        [e[1] for e in entries], np.zeros(len(entries), np.uint8),
                        [e[2] for e in entries], [e[3] for e in entries])
    return pyoracle.block_write(pyoracle.index_block_encode(it), block_type=INDEX)


def reseal_header(block):
    """The block with its header checksum (low 32 bits of xxh3_128 over the first 29
    bytes, header.rs:103-110) recomputed after a header field was edited."""
    b = bytes(block)
    return b[:29] + (pyoracle.xxh3_128(b[:29]) & 0xFFFFFFFF).to_bytes(4, "little") + b[33:]


# ---- the shared test tables
def mvcc_table(seed, two_level):
    """The tables of the issue: few distinct keys, many versions each, small blocks."""
    items = random_sorted_items(600, seed, kmin=1, kmax=3, alphabet=b"abc", vmax=40)
    t = pyoracle.table_write(items, block_size=256, restart_interval=4, hash_ratio=1.33, two_level=two_level,
                             partition_size=128)
    return items, t


def mvcc_queries(items, seed):
    """Every item's key at snapshots seqno + 1, seqno, 0, 1 << 62, plus 300 random needles
    over b"abcd" of length 0-4 (the empty needle included)."""
    rng = random.Random(1000 + seed)
    qs = []
    for i in range(items.n):
        k, s = item_key(items, i), int(items.seqno[i])
        qs += [(k, s + 1), (k, s), (k, 0), (k, 1 << 62)]
    qs.append((b"", 1 << 62))
    for _ in range(299):
        qs.append((bytes(rng.choice(b"abcd") for _ in range(rng.randint(0, 4))), rng.choice([1 << 62, 500, 1001])))
    return qs
