"""Host models of the writer's block cut (writer/mod.rs:284-290,374; with `extra` and no values
PartitionedIndexWriter::register_data_block, writer/index/partitioned.rs:166-179).

  loop_cut   the rule as the writer states it: a running weight, item by item;
  chain_cut  the closed form lsm_cut_blocks_device rests on: P[i] = key_off[i] + val_off[i] +
             extra * i, next(s) = the least j in (s, n] with P[j] - P[s] >= block_size (n if
             none), blocks = the chain 0 -> next(0) -> ...;
  tiled_cut  the same chain taken the way the kernels take it: per tile jump / cnt of every
             item, one walk over the tiles, a scan of the tiles' counts, per-tile emission.

All return the starts as a list of ints (n_blocks + 1 entries, [0] for no items)."""
import numpy as np


def _prefix(key_off, val_off, extra):
    key_off = np.asarray(key_off, np.uint64)
    n = len(key_off) - 1
    p = key_off.copy()
    if val_off is not None:
        p = p + np.asarray(val_off, np.uint64)
    return p + np.uint64(extra) * np.arange(n + 1, dtype=np.uint64), n


def loop_cut(key_off, val_off, block_size, extra=0):
    n = len(key_off) - 1
    starts, chunk, count = [0], 0, 0
    for i in range(n):
        chunk += int(key_off[i + 1]) - int(key_off[i]) + extra
        if val_off is not None:
            chunk += int(val_off[i + 1]) - int(val_off[i])
        count += 1
        if chunk >= block_size:
            starts.append(i + 1)
            chunk = count = 0
    if count:
        starts.append(n)
    return starts


def next_items(key_off, val_off, block_size, extra=0):
    """next(i) for every i in [0, n) (non-decreasing offsets)."""
    p, n = _prefix(key_off, val_off, extra)
    nx = np.searchsorted(p, p[:n] + np.uint64(block_size), side="left")
    return np.clip(nx, np.arange(1, n + 1), n).astype(np.int64), n


def chain_cut(key_off, val_off, block_size, extra=0):
    nx, n = next_items(key_off, val_off, block_size, extra)
    starts, s = [0], 0
    while s < n:
        s = int(nx[s])
        starts.append(s)
    return starts


def tiled_cut(key_off, val_off, block_size, extra=0, tile=8):
    nx, n = next_items(key_off, val_off, block_size, extra)
    n_tiles = max(1, -(-n // tile))
    jump, cnt = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for i in range(n - 1, -1, -1):  # (the kernel gets these by pointer doubling)
        end = min((i // tile + 1) * tile, n)
        if nx[i] >= end:
            jump[i], cnt[i] = nx[i], 1
        else:
            jump[i], cnt[i] = jump[nx[i]], cnt[nx[i]] + 1
    entry, tcnt = [None] * n_tiles, [0] * n_tiles
    s = 0
    while s < n:  # the walk: one hop per tile the chain enters
        entry[s // tile], tcnt[s // tile] = s, int(cnt[s])
        s = int(jump[s])
    base = np.concatenate([[0], np.cumsum(tcnt)])
    starts = [0] * (int(base[-1]) + 1)
    for t in range(n_tiles):
        if entry[t] is None:
            continue
        s, end = entry[t], min((t + 1) * tile, n)
        for k in range(tcnt[t]):
            starts[int(base[t]) + k] = s
            s = int(nx[s])
        assert s >= end
    starts[int(base[-1])] = n
    return starts
