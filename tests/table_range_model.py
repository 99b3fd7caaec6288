"""Python restatement of the forward drain of Table::range (src/table/mod.rs:391-422, table
Iter src/table/iter.rs:94-293) over the bytes of a table file, the model lsm_table_range is
checked against.  Built on TableModel (tests/table_get_model.py: load_block, index entries)
and pyoracle.seek (both data-block seeks, crossing clamp included).

The rules:
  span of one index block: with a lower bound a = the first entry failing
    end_key < lo || (end_key == lo && seqno >= u64::MAX) (index_block/iter.rs:25-34; no such
    entry ends the index drain), else 0; with an upper bound b = the first entry with
    end_key > hi, else the last entry (iter.rs:36-40 over partition_point_2,
    block/decoder.rs:210-256), without one the last entry; the block yields a..=b;
  handle list H: the TLI's span (full index); or the TLI's span names the partitions, each
    spanned with the same seeks, in order, a partition whose lower seek finds nothing ending
    the drain (block_index/two_level.rs:78-173);
  rows: every block of H, loaded as a Data block and seeked with both bounds
    (iter.rs:272-277), gives [first, end); the drain is those ranges in H order.

drain() is that, literally: every block of H, both seeks per block.  answer() derives from it
what lsm_table_range reports: the outcome, the first and the last row's position, and, for
the status, which blocks its reading order touches: the TLI, the drain up to the first row's
block, the drain from its end back to the last row's block.  A fault in a touched block is the
query's status; the blocks strictly between the two rows are not touched.
"""
import functools
import random

import pyoracle
from table_get_model import DATA, OK, PARSE, TableError, TableModel, item_key, mvcc_table

RANGE_NONE, RANGE_NO_BLOCK, RANGE_EMPTY, RANGE_ROWS = range(4)
SEEK_LO, SEEK_HI, SEEK_LO_EXCLUSIVE, SEEK_HI_EXCLUSIVE = 1, 2, 4, 8
U64_MAX = 2 ** 64 - 1
NO_ROWS = (0, 0, 0, 0, 0, 0)  # first block off, size, item; last block off, size, item of a non-ROWS answer


def flags_of(lo, hi, lo_excl, hi_excl):
    """The LSM_SEEK_* bits of a query (lo / hi: bytes, or None = unbounded)."""
    return ((SEEK_LO if lo is not None else 0) | (SEEK_HI if hi is not None else 0) |
            (SEEK_LO_EXCLUSIVE if lo_excl else 0) | (SEEK_HI_EXCLUSIVE if hi_excl else 0))


def brute_force(keys, lo, hi, lo_excl=False, hi_excl=False):
    """Indices of the keys (a table's, in table order) inside the bounds."""
    def inside(k):
        if lo is not None and (k < lo or (lo_excl and k == lo)):
            return False
        return hi is None or k < hi or (k == hi and not hi_excl)
    return [i for i, k in enumerate(keys) if inside(k)]


@functools.lru_cache(maxsize=None)
def mvcc_range_queries(seed, two_level):
    """The queries of the issue on mvcc_table(seed, two_level): [(lo, hi, lo_excl, hi_excl)],
    None = unbounded.  Bound values: every distinct key plus four keys the table does not hold
    plus unbounded, crossed as lo x hi x the inclusivity bits, shuffled with a fixed seed, the
    first 1500."""
    items, _ = mvcc_table(seed, two_level)
    values = sorted({item_key(items, i) for i in range(items.n)} | {b"", b"d", b"ab\0", b"bb\xff"}) + [None]
    qs = [(lo, hi, le, he) for lo in values for hi in values for le in (False, True) for he in (False, True)]
    random.Random(7000 + 10 * seed + two_level).shuffle(qs)
    return qs[:1500]


class RangeModel:
    def __init__(self, file, tli_off, tli_size, two_level):
        self.table = TableModel(file, tli_off, tli_size, two_level)

    @staticmethod
    def span(entries, lo, hi):
        """(a, b) of one index block, None if the lower seek finds nothing."""
        a, b = 0, len(entries) - 1
        if lo is not None:
            a = TableModel.seek(entries, lo, U64_MAX)
            if a == len(entries):
                return None
        if hi is not None:
            b = next((i for i, e in enumerate(entries) if e[0] > hi), len(entries) - 1)
        return a, b

    def handles(self, lo, hi):
        """H in drain order: [(off, size)] of the data blocks; a partition that does not load
        stands in it as the TableError it raises (the drain cannot go past it; the partitions
        after it are still listed, for the backward reading order)."""
        t = self.table
        tli = t.index_entries(*t.tli)
        s = self.span(tli, lo, hi)
        if s is None:
            return []
        if not t.two_level:
            return [(e[2], e[3]) for e in tli[s[0]:s[1] + 1]]
        out = []
        for p in tli[s[0]:s[1] + 1]:
            try:
                part = t.index_entries(p[2], p[3])
            except TableError as err:
                out.append(err)
                continue
            ps = self.span(part, lo, hi)
            if ps is None:
                break
            out += [(e[2], e[3]) for e in part[ps[0]:ps[1] + 1]]
        return out

    def block_range(self, h, lo, hi, lo_excl, hi_excl):
        """[first, end) of the data block at handle h under both seeks; raises TableError."""
        if isinstance(h, TableError):
            raise h
        payload = self.table._load(h[0], h[1], DATA)
        r = pyoracle.seek(payload, lo, hi, lo_excl, hi_excl)
        if r is None:
            raise TableError(PARSE)
        return r[0], r[1]

    def drain(self, lo, hi, lo_excl=False, hi_excl=False):
        """The literal drain: [(handle, first, end) or (handle, TableError)] for every block of H."""
        out = []
        for h in self.handles(lo, hi):
            try:
                out.append((h,) + self.block_range(h, lo, hi, lo_excl, hi_excl))
            except TableError as err:
                out.append((h, err))
        return out

    def answer(self, lo, hi, lo_excl=False, hi_excl=False):
        """-> (status, (outcome, first_off, first_size, first_item, last_off, last_size, last_item))."""
        try:
            d = self.drain(lo, hi, lo_excl, hi_excl)
        except TableError as err:  # the TLI
            return err.status, (RANGE_NONE,) + NO_ROWS

        def stops(x):  # a block that ends a walk: a fault, or a row
            return len(x) == 2 or x[1] < x[2]

        fi = next((i for i, x in enumerate(d) if stops(x)), None)
        if fi is None:
            return OK, ((RANGE_EMPTY if d else RANGE_NO_BLOCK),) + NO_ROWS
        li = next(i for i in range(len(d) - 1, fi - 1, -1) if stops(d[i]))
        for x in (d[fi], d[li]):  # the reading order: the lower walk's fault first
            if len(x) == 2:
                return x[1].status, (RANGE_NONE,) + NO_ROWS
        (fh, first, _), (lh, _, end) = d[fi], d[li]
        return OK, (RANGE_ROWS, fh[0], fh[1], first, lh[0], lh[1], end - 1)
