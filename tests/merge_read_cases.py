"""Inputs of the lsm_merge_read tests (pure Python, fixed seeds).  grouped_case() builds
runs[s][g] (the run of source s for group g) of one shape with every edge of EDGES planted;
edges_of() finds the edges in a finished input, so that tests/test_merge_read_model.py can
assert on the CPU that each case still holds what it was built for and the GPU file cannot
pass vacuously."""
import random

import merge_model as M
from merge_cases import HEAD16, PREFIX32

SHAPES = ((1, 1), (2, 1), (3, 65), (64, 2), (4, 300))  # (n_sources, n_groups)
RUN_LENS = (0, 1, 2, 63, 64, 65, 200)
VAL_LENS = (0, 255, 256, 20000)
SNAP = 2 ** 63  # the seqnos lie in [SNAP - 8, SNAP + 8): half of them are >= 2^63 and invisible
POOL = sorted([b"a", b"a\x00", b"aa", HEAD16, HEAD16 + b"a", HEAD16 + b"b", PREFIX32 + b"\x7f", PREFIX32 + b"\x80",
               PREFIX32 + b"\x80x", b"\x00", b"\xff\xfe"] + [b"k%02d" % i for i in range(13)])
WINDOW = 9  # keys of one group when the groups are many: the first and the last are the boundary keys
# edges a shape cannot hold
NEEDS_TWO_SOURCES = {"tie_across_sources"}
NEEDS_TWO_GROUPS = {"group_boundary"}
NEEDS_MANY_GROUPS = {"empty_group"}
EDGES = ("group_boundary", "seqno_equals_snapshot", "all_invisible_key", "invisible_tombstone_over_visible_value",
         "visible_tombstone_over_values", "tie_across_sources", "head16", "head32", "prefix_key", "wide_seqnos",
         "empty_group", "empty_run", "long_value", "value_255", "value_256", "value_0") + \
    tuple("run_len_%d" % n for n in RUN_LENS)


def expected_edges(n_src, n_groups):
    out = set(EDGES)
    if n_src < 2:
        out -= NEEDS_TWO_SOURCES
    if n_groups < 2:
        out -= NEEDS_TWO_GROUPS
    if n_groups < 3:
        out -= NEEDS_MANY_GROUPS
    if n_src * n_groups < len(RUN_LENS):  # one or two runs: the lengths they can hold
        out -= {"run_len_%d" % n for n in RUN_LENS} | {"empty_run"}
    return out


def _val(rng, t, n=None):
    """n value bytes (default: a random short length), none for a tombstone."""
    if t in (M.TOMBSTONE, M.WEAK_TOMBSTONE):
        return b""
    if n is None:
        n = rng.choice((0, 1, 5, 40, 255, 256))
    return (bytes(rng.getrandbits(8) for _ in range(min(n, 97))) * (n // 97 + 1))[:n]


def _plants(rng, window, n_src):
    """source -> planted items of one group over the interior keys of its window."""
    k = window[1:-1]
    plants = {
        0: [(k[0] + b"~gone", b"gone-a", SNAP + 3, M.VALUE), (k[0] + b"~gone", b"gone-b", SNAP, M.VALUE),
            (k[1] + b"~t", b"", SNAP + 1, M.TOMBSTONE), (k[1] + b"~t", b"seen", SNAP - 1, M.VALUE),
            (k[2] + b"~d", b"", SNAP - 1, M.TOMBSTONE), (k[2] + b"~d", b"old", SNAP - 2, M.VALUE),
            (k[2] + b"~d", b"older", SNAP - 3, M.VALUE),
            (k[3] + b"~e", b"source 0", SNAP - 4, M.VALUE),
            (k[0] + b"~long", _val(rng, M.VALUE, 20000), SNAP - 1, M.VALUE),
            (k[0] + b"~255", _val(rng, M.VALUE, 255), SNAP - 1, M.INDIRECTION),
            (k[0] + b"~256", _val(rng, M.VALUE, 256), SNAP - 1, M.VALUE),
            (k[0] + b"~empty", b"", SNAP - 1, M.VALUE)]}
    if n_src > 1:
        plants[1] = [(k[3] + b"~e", b"source 1", SNAP - 4, M.VALUE)]
    return plants


def grouped_case(n_src, n_groups, seed=0):
    """-> runs[s][g].  Every run is sorted; the lengths come from RUN_LENS (most runs hold 0, 1
    or 2 items, a few 63, 64, 65 and 200); with 3 groups or more every seventh group is empty;
    group g + 1 starts with the user key group g ends with."""
    rng = random.Random(5000 + 1000 * n_src + n_groups + seed)
    n_runs = n_src * n_groups
    many = n_groups > 2
    empty = {g for g in range(n_groups) if many and g % 7 == 3}
    lens = {}
    live = [(s, g) for s in range(n_src) for g in range(n_groups) if g not in empty]
    for s, g in live:
        lens[(s, g)] = rng.choice((0, 1, 1, 2, 2)) if n_runs > 2 else 200 if s == 0 else 65
    big = [(0, g) for g in range(n_groups) if g not in empty][:2]  # the groups that take the plants
    if n_runs > 2:
        free = [r for r in live if r not in big and not (n_src > 1 and r[0] == 1 and (0, r[1]) in big)]
        for r, n in zip(rng.sample(free, min(len(free), 8)), (63, 64, 65, 200, 63, 64, 65, 0)):
            lens[r] = n
        lens[big[0]] = 200
        if len(big) > 1:
            lens[big[1]] = 65
    windows, at = [], 0
    for g in range(n_groups):
        if not many:  # one or two groups: the whole pool, the second group's keys behind the first's last key
            windows.append(POOL if g == 0 else [POOL[-1]] + [POOL[-1] + k for k in POOL[1:]])
            continue
        if at + WINDOW > len(POOL):  # the last window ends with the pool; then from the start again
            at = 0 if at - (WINDOW - 1) == len(POOL) - WINDOW else len(POOL) - WINDOW
        windows.append(POOL[at:at + WINDOW])
        at += WINDOW - 1
    runs = [[[] for _ in range(n_groups)] for _ in range(n_src)]
    for g in range(n_groups):
        if g in empty:
            continue
        window = windows[g]
        plants = _plants(rng, window, n_src) if (0, g) in big else {}
        for s in range(n_src):
            run = list(plants.get(s, []))
            if s == 0 and g + 1 < n_groups and g + 1 not in empty and windows[g + 1][0] == window[-1]:
                run.append((window[-1], b"ends group %d" % g, SNAP - 6, M.VALUE))
            if s == n_src - 1 and g > 0 and g - 1 not in empty and windows[g - 1][-1] == window[0]:
                run.append((window[0], b"starts group %d" % g, SNAP - 5, M.VALUE))
            n = max(lens[(s, g)], len(run)) if run else lens[(s, g)]
            if run and n not in RUN_LENS:
                n = min(x for x in RUN_LENS if x >= n)
            while len(run) < n:
                t = rng.choice((M.VALUE, M.VALUE, M.TOMBSTONE, M.WEAK_TOMBSTONE, M.INDIRECTION))
                run.append((rng.choice(window[1:-1]), _val(rng, t), SNAP - 8 + rng.randrange(16), t))
            runs[s][g] = sorted(run, key=lambda it: (it[0], -it[2]))
    return runs


def edges_of(runs, snap=SNAP):
    """The names of EDGES that the input holds (at snapshot snap)."""
    n_src, n_groups = len(runs), len(runs[0])
    found = set()
    streams = []
    for g in range(n_groups):
        sources = [runs[s][g] for s in range(n_src)]
        for run in sources:
            found.add("run_len_%d" % len(run))
            if not run:
                found.add("empty_run")
        stream = [it for it, _ in M.merge(sources)]
        streams.append(stream)
        if not stream:
            found.add("empty_group")
            continue
        seen = {}
        for s, run in enumerate(sources):
            for it in run:
                if seen.setdefault((it[0], it[2]), s) != s:
                    found.add("tie_across_sources")
                if it[2] == snap:
                    found.add("seqno_equals_snapshot")
                if it[2] >= 2 ** 63:
                    found.add("wide_seqnos")
        by_key = {}
        for it in stream:
            by_key.setdefault(it[0], []).append(it)
        for key, versions in by_key.items():
            visible = [it for it in versions if it[2] < snap]
            if not visible:
                found.add("all_invisible_key")
                continue
            head = visible[0]
            if versions[0][2] >= snap and M.is_tombstone(versions[0][3]) and head[3] == M.VALUE:
                found.add("invisible_tombstone_over_visible_value")
            if M.is_tombstone(head[3]) and len(visible) > 1:
                found.add("visible_tombstone_over_values")
            if not M.is_tombstone(head[3]):
                found.add({0: "value_0", 255: "value_255", 256: "value_256"}.get(len(head[1]), "value_other"))
                if len(head[1]) >= 20000:
                    found.add("long_value")
        keys = sorted(by_key)
        for a, b in zip(keys, keys[1:]):
            if b.startswith(a):
                found.add("prefix_key")
            for n in (16, 32):
                if len(a) > n and len(b) > n and a[:n] == b[:n] and a[n] != b[n]:
                    found.add("head%d" % n)
    for a, b in zip(streams, streams[1:]):
        if a and b and a[-1][0] == b[0][0] and a[-1][2] < snap and b[0][2] < snap:
            found.add("group_boundary")
    found.discard("value_other")
    return found


def group_between_neighbours(runs, group_start):
    """The first group that unsorted_group() can break and that, like its two neighbours,
    emits rows (group_start: the model's answer for the sorted input)."""
    emits = lambda g: group_start[g] < group_start[g + 1]
    for g in range(1, len(runs[0]) - 1):
        breakable = any((a[0], -a[2]) != (b[0], -b[2]) for src in runs for a, b in zip(src[g], src[g][1:]))
        if breakable and emits(g - 1) and emits(g) and emits(g + 1):
            return g
    raise AssertionError("no such group")


def unsorted_group(runs, g):
    """A copy of runs with two unequal neighbours of one run of group g swapped.
    Returns (runs, source)."""
    out = [[list(r) for r in src] for src in runs]
    for s, src in enumerate(out):
        run = src[g]
        for i in range(len(run) - 1):
            if (run[i][0], -run[i][2]) != (run[i + 1][0], -run[i + 1][2]):
                run[i], run[i + 1] = run[i + 1], run[i]
                return out, s
    raise AssertionError("group %d has no run with two unequal neighbours" % g)
