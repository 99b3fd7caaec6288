"""Python restatement of lsm_table_range_rows over the bytes of a table file: from the file, the
table's data-block offsets and per-query positions (what lsm_table_range reports) to the rows
of every query, its status, run_start and need.  Built on TableModel (tests/table_get_model.py:
load_block), RangeModel (tests/table_range_model.py: the positions) and
pyoracle.data_block_decode / pyoracle.materialize, never on the library.

The rules (include/lsmgpu.h):
  a query is live when its status is OK and its outcome RANGE_ROWS; one that is not gets an
    empty run and keeps its status;
  first_block > last_block or an ordinal >= n_blocks: BAD_ARG, no block touched;
  every block first_block ..= last_block is checked, in this order: the handle (shorter than a
    header, decreasing, ending past the file: TRUNCATED), load_block's header checks, the
    trailer (PARSE), the edge items (BAD_ARG), the whole block's records (PARSE);
  the query's status is that of the lowest-ordinal block that has one, and its run is then
    empty; else its rows are items first_item .. of the first block, every item of the blocks
    between, items ..= last_item of the last, each (key = head prefix + suffix, value (empty
    for tombstones), seqno + global_seqno wrapping, vtype).
"""
import functools

import pyoracle
from table_get_model import DATA, OK, PARSE, TRUNCATED, TableError, TableModel, item_key, mvcc_table
from table_range_model import RANGE_ROWS, RangeModel, mvcc_range_queries

BAD_ARG, OVERFLOW = 10, 6
U64 = 2 ** 64 - 1


def trailer_item_count(p):
    """read_trailer (oracle/block.c:302-318, trailer.rs:118-163): the item count, None = PARSE."""
    n = len(p)
    if n < 32:
        return None
    tr = p[n - 31:]
    ri, step = tr[0], tr[1]
    bin_len, bin_off = int.from_bytes(tr[2:6], "little"), int.from_bytes(tr[6:10], "little")
    item_count = int.from_bytes(tr[27:31], "little")
    if ri == 0 or step not in (2, 4) or bin_len == 0 or bin_off == 0:
        return None
    if bin_off + bin_len * step > n - 31 or p[bin_off - 1] != 0xFF:
        return None
    if bin_len != (item_count + ri - 1) // ri:
        return None
    return item_count


class RowsModel:
    def __init__(self, file, block_off, global_seqno=0):
        self.table = TableModel(file, 0, 0, False)
        self.off = [int(o) for o in block_off]
        self.global_seqno = global_seqno
        self._blocks = {}

    @property
    def n_blocks(self):
        return len(self.off) - 1

    def block(self, b):
        """-> (status before the edge check, item count, rows or None when the records do not parse)."""
        if b not in self._blocks:
            self._blocks[b] = self._block(b)
        return self._blocks[b]

    def _block(self, b):
        o0, o1 = self.off[b], self.off[b + 1]
        if o1 < o0 or o1 - o0 < 33 or o1 > len(self.table.file):
            return TRUNCATED, 0, None
        try:
            payload = self.table._load(o0, o1 - o0, DATA)
        except TableError as err:
            return err.status, 0, None
        count = trailer_item_count(payload)
        if count is None:
            return PARSE, 0, None
        n, p = pyoracle.data_block_decode(payload)
        if n < 0:
            return OK, count, None
        assert n == count
        rows = [(k, v, (s + self.global_seqno) & U64, t) for k, v, s, t in pyoracle.materialize(payload, p, payload[-31])]
        return OK, count, rows

    def block_rows(self, b, first, fi, last, li):
        """The status and the window's rows of block b (first / last: it is the query's first / last)."""
        st, count, rows = self.block(b)
        if st != OK:
            return st, []
        if (first and fi >= count) or (last and li >= count) or (first and last and fi > li):
            return BAD_ARG, []
        if rows is None:
            return PARSE, []
        return OK, rows[(fi if first else 0):(li + 1 if last else count)]

    def query(self, status, outcome, fb, fi, lb, li):
        """-> (row status, rows, pairs)."""
        if status != OK or outcome != RANGE_ROWS:
            return status, [], 0
        if fb > lb or lb >= self.n_blocks:
            return BAD_ARG, [], 0
        out = []
        bad = OK
        for b in range(fb, lb + 1):
            st, rows = self.block_rows(b, b == fb, fi, b == lb, li)
            if st != OK and bad == OK:
                bad = st  # (the lowest ordinal's)
            out += rows
        return bad, ([] if bad != OK else out), lb - fb + 1

    def answer(self, positions, base=(0, 0, 0)):
        """positions: [(status, outcome, first_block, first_item, last_block, last_item)] ->
        dict: runs (the rows of each query), row_status, run_start (absolute), need, end."""
        runs, statuses, pairs = [], [], 0
        for pos in positions:
            st, rows, np_ = self.query(*pos)
            runs.append(rows)
            statuses.append(st)
            pairs += np_
        run_start = [base[0]]
        for r in runs:
            run_start.append(run_start[-1] + len(r))
        flat = [r for run in runs for r in run]
        need = [pairs, len(flat), sum(len(r[0]) for r in flat), sum(len(r[1]) for r in flat)]
        end = [base[0] + need[1], base[1] + need[2], base[2] + need[3]]
        return {"runs": runs, "row_status": statuses, "run_start": run_start, "need": need, "end": end}


def positions_of(range_answers, block_off):
    """RangeModel.answer results -> the positions lsm_table_range reports with these offsets:
    [(status, outcome, first_block, first_item, last_block, last_item)]."""
    off = [int(o) for o in block_off]
    ordinal = {(off[i], off[i + 1] - off[i]): i for i in range(len(off) - 1)}
    out = []
    for st, e in range_answers:
        if st == OK and e[0] == RANGE_ROWS:
            out.append((st, e[0], ordinal[e[1:3]], e[3], ordinal[e[4:6]], e[6]))
        else:
            out.append((st, e[0], 0, 0, 0, 0))
    return out


def item_rows(items, global_seqno=0):
    """The item list as rows: (key, value (empty for tombstones), seqno + global_seqno, vtype)."""
    out = []
    for i in range(items.n):
        vt = int(items.vtype[i])
        val = b"" if vt in (1, 2) else bytes(items.vals[int(items.val_off[i]):int(items.val_off[i + 1])])
        out.append((item_key(items, i), val, (int(items.seqno[i]) + global_seqno) & U64, vt))
    return out


@functools.lru_cache(maxsize=None)
def mvcc_rows_case(seed, two_level):
    """The MVCC table of the issue, its queries, the positions the range model gives and the
    range answers they come from, computed once per table."""
    items, t = mvcc_table(seed, two_level)
    queries = mvcc_range_queries(seed, two_level)
    model = RangeModel(t["file"], t["tli_off"], t["tli_size"], two_level)
    answers = [model.answer(*q) for q in queries]
    return items, dict(t, two_level=two_level), queries, positions_of(answers, t["block_off"])
