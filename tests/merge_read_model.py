"""Python restatement of the reader's merge (TreeIter::create_range, src/range.rs:99-235), the
model lsm_merge_read is checked against: every source filtered by seqno_filter
(range.rs:22-24), Merger (merge_model.merge), MvccStream::next (src/mvcc_stream.rs:45-52) and
the tombstone filter, once as the reference writes it and once as the per-position rule the
device kernel applies.

Items are merge_model's tuples (key bytes, value bytes, seqno, vtype).  A grouped input is
runs[s][g]: the run of source s for group (query) g; flat order is source-major, run
s * n_groups + g, as lsm_merge_read takes it."""
import random

import merge_model as M

BAD_ARG = 10


def seqno_filter(item_seqno, seqno):
    """range.rs:22-24."""
    return item_seqno < seqno


def mvcc_stream(stream):
    """MvccStream::next run to the end (a peekable iterator, drain_key_min).
    stream: [(item, input index)] in merged order."""
    out = []
    pos, n = 0, len(stream)
    while pos < n:
        head = stream[pos]
        pos += 1
        while pos < n and stream[pos][0][0] == head[0][0]:  # drain_key_min(&head.key.user_key)
            pos += 1
        out.append(head)
    return out


def read_group(sources, snapshot, keep_tombstones=False, first_index=None):
    """One query as the reference composes it.  sources: the group's runs, lowest source
    first; first_index[s]: the input index of the first item of run s (default: the runs
    back to back).  Returns [(item, input index)]."""
    if first_index is None:
        first_index, at = [], 0
        for run in sources:
            first_index.append(at)
            at += len(run)
    # every source filtered, then the Merger (merge_model.merge: key, seqno descending, lower source first)
    filtered = [[it for it in run if seqno_filter(it[2], snapshot)] for run in sources]
    index = [first_index[s] + k for s, run in enumerate(sources) for k, it in enumerate(run)
             if seqno_filter(it[2], snapshot)]
    stream = [(it, index[i]) for it, i in M.merge(filtered)]
    out = mvcc_stream(stream)
    if not keep_tombstones:
        out = [(it, i) for it, i in out if not M.is_tombstone(it[3])]
    return out


def rule_group(sources, snapshot, keep_tombstones=False, first_index=None):
    """The same query decided per position of the merged stream of ALL the group's items:
    position j is kept iff it is visible, it is the group's first position or its predecessor
    has another user key or is not visible, and it is no tombstone (or they are kept)."""
    if first_index is None:
        first_index, at = [], 0
        for run in sources:
            first_index.append(at)
            at += len(run)
    base = []
    for s, run in enumerate(sources):
        base += [first_index[s] + k for k in range(len(run))]
    stream = [(it, base[i]) for it, i in M.merge(sources)]
    out = []
    for j, (it, i) in enumerate(stream):
        if not seqno_filter(it[2], snapshot):
            continue
        if j > 0:
            prev = stream[j - 1][0]
            if prev[0] == it[0] and seqno_filter(prev[2], snapshot):
                continue
        if M.is_tombstone(it[3]) and not keep_tombstones:
            continue
        out.append((it, i))
    return out


def brute_group(sources, snapshot, keep_tombstones=False):
    """A dict keeps the newest visible version of each key (of equal seqnos the lowest source's
    first one); tombstones dropped at the end.  Returns the items, key ascending."""
    best = {}
    for run in sources:
        for it in run:
            if it[2] < snapshot and (it[0] not in best or it[2] > best[it[0]][2]):
                best[it[0]] = it
    return [best[k] for k in sorted(best) if keep_tombstones or not M.is_tombstone(best[k][3])]


def n_groups_of(runs):
    return len(runs[0]) if runs else 0


def flat_runs(runs):
    """runs[s][g] -> the run list in the call's order (run s * n_groups + g)."""
    return [run for src in runs for run in src]


def merge_read(runs, snapshot, keep_tombstones=False, group_seqno=None, in_status=None, fn=read_group):
    """lsm_merge_read's answer for sorted-or-not inputs: dict(items, src, group_start, status).
    in_status: None or a flat list [n_sources * n_groups] in run order."""
    n_src, n_groups = len(runs), n_groups_of(runs)
    first, at = [], 0
    for run in flat_runs(runs):
        first.append(at)
        at += len(run)
    items, src, group_start, status = [], [], [0], []
    for g in range(n_groups):
        sources = [runs[s][g] for s in range(n_src)]
        fault = 0
        if in_status is not None:
            fault = next((in_status[s * n_groups + g] for s in range(n_src) if in_status[s * n_groups + g]), 0)
        if not fault and not all(M.run_is_sorted(r) for r in sources):
            fault = BAD_ARG
        status.append(fault)
        if not fault:
            snap = group_seqno[g] if group_seqno is not None else snapshot
            got = fn(sources, snap, keep_tombstones, [first[s * n_groups + g] for s in range(n_src)])
            items += [it for it, _ in got]
            src += [i for _, i in got]
        group_start.append(len(items))
    return {"items": items, "src": src, "group_start": group_start, "status": status}


def random_grouped(rng, n_src, n_groups, max_len=6, n_keys=3, max_seq=10):
    """Random runs[s][g] over a few keys with many versions, duplicate seqnos and all four
    value types; neighbouring groups share their keys."""
    keys = [bytes([97 + k]) for k in range(n_keys)]
    runs = []
    for _ in range(n_src):
        src = []
        for _ in range(n_groups):
            run = [(rng.choice(keys), b"v%d" % rng.randrange(100), rng.randrange(max_seq),
                    rng.choice((M.VALUE, M.TOMBSTONE, M.WEAK_TOMBSTONE, M.INDIRECTION)))
                   for _ in range(rng.randrange(0, max_len + 1))]
            src.append(sorted(run, key=lambda it: (it[0], -it[2])))
        runs.append(src)
    return runs


def cross_check(n_inputs, seed=0):
    """rule_group == read_group on random grouped inputs, snapshots below, inside and above the
    seqno range, both flag values.  Returns the number of comparisons made."""
    rng = random.Random(seed)
    done = 0
    for _ in range(n_inputs):
        max_seq = rng.randrange(1, 10)
        runs = random_grouped(rng, rng.randrange(1, 5), rng.randrange(1, 4), n_keys=rng.randrange(1, 4),
                              max_seq=max_seq)
        for snap in (0, rng.randrange(0, max_seq + 1), max_seq, max_seq + 5):
            for keep in (False, True):
                want = merge_read(runs, snap, keep, fn=read_group)
                got = merge_read(runs, snap, keep, fn=rule_group)
                assert got == want, (runs, snap, keep, got, want)
                done += 1
    return done
