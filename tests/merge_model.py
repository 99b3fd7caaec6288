"""Python restatement of Merger (src/merge.rs:34-100) and CompactionStream::next
(src/compaction/stream.rs:145-219, NoFilter), the model lsm_merge_runs is
checked against.

An item is a tuple (key bytes, value bytes, seqno, vtype).  Value types as in
src/value_type.rs:36-58: 0 Value, 1 Tombstone, 2 WeakTombstone, 4 Indirection.
"""
import random

VALUE, TOMBSTONE, WEAK_TOMBSTONE, INDIRECTION = 0, 1, 2, 4


def is_tombstone(vtype):
    """InternalValue::is_tombstone: Tombstone or WeakTombstone."""
    return vtype in (TOMBSTONE, WEAK_TOMBSTONE)


def merge(runs):
    """Merger over sorted runs: InternalKey order (key.rs:69-71: user key ascending,
    seqno descending); items with equal (key, seqno) come out lower run first (the
    reference's heap leaves that order open).  Returns [(item, input index)], the
    input index counting through the runs back to back."""
    tagged = []
    i = 0
    for r, run in enumerate(runs):
        for it in run:
            tagged.append((it, i, r))
            i += 1
    tagged.sort(key=lambda t: (t[0][0], -t[0][2], t[2]))  # (stable: equal neighbours of one run keep their order)
    return [(it, i) for it, i, _ in tagged]


def compaction_stream(stream, gc_seqno_threshold, evict_tombstones=False, zero_seqnos=False):
    """CompactionStream::next run to the end, written as the reference writes it
    (a peekable iterator, drain_key).  stream: [(item, input index)] in merged order.
    Returns (emitted [(item, input index)], drained input indices): drained is what
    DroppedKvCallback::on_dropped receives, in call order."""
    out, drained = [], []
    pos = 0
    n = len(stream)

    def drain_key(key):
        nonlocal pos
        while pos < n and stream[pos][0][0] == key:
            drained.append(stream[pos][1])
            pos += 1

    while pos < n:
        head, head_idx = stream[pos]
        pos += 1
        key, value, seqno, vtype = head
        if pos < n:
            peeked = stream[pos][0]
            if peeked[0] > key:
                if is_tombstone(vtype) and evict_tombstones:
                    continue
            elif peeked[2] < gc_seqno_threshold:
                if vtype == TOMBSTONE and evict_tombstones:
                    drain_key(key)
                    continue
                drop_weak_tombstone = peeked[3] == VALUE and vtype == WEAK_TOMBSTONE
                drain_key(key)
                if drop_weak_tombstone:
                    continue
        elif is_tombstone(vtype) and evict_tombstones:
            continue
        if zero_seqnos and seqno < gc_seqno_threshold:
            seqno = 0
        out.append(((key, value, seqno, vtype), head_idx))
    return out, drained


def per_item_rule(stream, gc_seqno_threshold, evict_tombstones=False, zero_seqnos=False):
    """The same stream decided per merged position from its two neighbours (what the
    device kernel does).  Returns the emitted [(item, input index)]."""
    out = []
    n = len(stream)
    thr = gc_seqno_threshold
    for j, ((key, value, seqno, vtype), idx) in enumerate(stream):
        if j > 0 and stream[j - 1][0][0] == key and seqno < thr:
            continue  # in a drained tail
        nxt = stream[j + 1][0] if j + 1 < n and stream[j + 1][0][0] == key else None
        if nxt is None:
            if is_tombstone(vtype) and evict_tombstones:
                continue
        elif nxt[2] < thr:
            if vtype == TOMBSTONE and evict_tombstones:
                continue
            if vtype == WEAK_TOMBSTONE and nxt[3] == VALUE:
                continue
        if zero_seqnos and seqno < thr:
            seqno = 0
        out.append(((key, value, seqno, vtype), idx))
    return out


def merge_runs(runs, gc_seqno_threshold=0, evict_tombstones=False, zero_seqnos=False):
    """CompactionStream::new(Merger::new(runs), thr).evict_tombstones(..).zero_seqnos(..).
    Returns (items, src, dropped): emitted items, their input indices, and the
    input indices that were not emitted (ascending)."""
    stream = merge(runs)
    out, _ = compaction_stream(stream, gc_seqno_threshold, evict_tombstones, zero_seqnos)
    src = [i for _, i in out]
    kept = set(src)
    return [it for it, _ in out], src, [i for i in range(len(stream)) if i not in kept]


def run_is_sorted(run):
    """InternalKey order inside a run; equal neighbours are accepted."""
    return all((a[0], -a[2]) <= (b[0], -b[2]) for a, b in zip(run, run[1:]))


def random_stream(rng, n, n_keys=4, max_seq=12, dup_seqnos=True):
    """A sorted random stream of n items over a few keys (so keys have many versions)."""
    keys = [bytes([97 + k]) for k in range(n_keys)]
    items = []
    for _ in range(n):
        items.append((rng.choice(keys), b"v%d" % rng.randrange(100), rng.randrange(max_seq),
                      rng.choice((VALUE, TOMBSTONE, WEAK_TOMBSTONE, INDIRECTION))))
    if not dup_seqnos:
        seen, uniq = set(), []
        for it in items:
            if (it[0], it[2]) not in seen:
                seen.add((it[0], it[2]))
                uniq.append(it)
        items = uniq
    items.sort(key=lambda it: (it[0], -it[2]))
    return [(it, i) for i, it in enumerate(items)]


def cross_check(n_streams, seed=0):
    """per_item_rule == compaction_stream on random streams, all four flag
    combinations, thresholds below, inside and above the seqno range.  Returns the
    number of comparisons made; raises AssertionError on the first difference."""
    rng = random.Random(seed)
    done = 0
    for _ in range(n_streams):
        stream = random_stream(rng, rng.randrange(0, 14), n_keys=rng.randrange(1, 4), max_seq=rng.randrange(1, 10),
                               dup_seqnos=rng.random() < 0.5)
        thr = rng.randrange(0, 12)
        for evict in (False, True):
            for zero in (False, True):
                want, _ = compaction_stream(stream, thr, evict, zero)
                got = per_item_rule(stream, thr, evict, zero)
                assert got == want, (stream, thr, evict, zero, got, want)
                done += 1
    return done
