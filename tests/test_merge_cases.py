"""CPU checks of tests/merge_cases.py: every generated set is sorted (unless it is meant
not to be), still has the structure it was built for, and the per-item GC rule agrees
with the reference loop on its merged stream.  The GPU tests run these sets; a later
edit of a generator that makes a set miss its edge fails here."""
import merge_cases as MC
import merge_model as M

SETS = {
    "wide_seqnos": (MC.wide_seqnos, MC.WIDE_THRESHOLDS),
    "long_ties": (MC.long_ties, (0, MC.TIE_SEQ, MC.TIE_SEQ + 1)),
    "long_ties_embedded": (MC.long_ties_embedded, (0, 50, MC.TIE_SEQ + 1)),
    "long_ties_64_runs": (MC.long_ties_64_runs, (0, MC.TIE_SEQ + 1)),
    "shared_heads_16": (lambda: MC.shared_heads(16), (500,)),
    "shared_heads_32": (lambda: MC.shared_heads(32), (500,)),
    "state_sorted": (MC.state_sorted, (400,)),
    "state_one_run": (MC.state_one_run, (400,)),
    "state_second": (MC.state_second, (400,)),
    "nothing_dropped": (MC.nothing_dropped, (0,)),
    "half_dropped": (MC.half_dropped, (MC.HALF_DROPPED_THR,)),
    "span_limit": (lambda: MC.span_limit(MC.MERGE_BUF, 15), (0,)),
    "mixed_keys": (MC.mixed_keys, (MC.MIXED_KEYS_THR,)),
    "graph_first": (lambda: MC.graph_sets()[0], (MC.GRAPH_THR,)),
    "graph_second": (lambda: MC.graph_sets()[1], (MC.GRAPH_THR,)),
}


def test_generators_are_deterministic_and_sorted():
    for name, (gen, _) in SETS.items():
        runs = gen()
        assert runs == gen(), name
        assert all(M.run_is_sorted(r) for r in runs), name
    for runs in MC.long_ties_orders():
        assert all(M.run_is_sorted(r) for r in runs)


def test_per_item_rule_on_every_set():
    done = 0
    for name, (gen, thresholds) in SETS.items():
        stream = M.merge(gen())
        for thr in thresholds:
            for evict, zero in MC.FLAG_PAIRS:
                want, _ = M.compaction_stream(stream, thr, evict, zero)
                assert M.per_item_rule(stream, thr, evict, zero) == want, (name, thr, evict, zero)
                done += 1
    assert done == 4 * sum(len(t) for _, t in SETS.values())


def test_wide_seqnos_shape():
    runs = MC.wide_seqnos()
    flat = [it for r in runs for it in r]
    assert len(runs) == 3 and len(flat) == 40 * 5 * 4 + 4 + len(MC.WIDE_SINGLES) and min(len(r) for r in runs) > 200
    seqs = {it[2] for it in flat}
    for base in MC.WIDE_BASES:
        assert {base + d for d in range(4)} <= seqs
    assert max(seqs) == 2 ** 64 - 2 and set(MC.HIGH_DWORD_PAIR) | set(MC.BIT63_PAIR) <= seqs
    hi, lo = MC.HIGH_DWORD_PAIR
    assert hi > lo and (hi & 0xFFFFFFFF) < (lo & 0xFFFFFFFF)  # the low dwords alone order them the other way
    a, b = MC.BIT63_PAIR
    assert a > b and a - 2 ** 64 < b                          # as int64 the larger one is negative
    # every threshold cuts somewhere else: five different output counts, without and with eviction
    for evict in (False, True):
        counts = [len(M.merge_runs(runs, thr, evict, True)[0]) for thr in MC.WIDE_THRESHOLDS]
        assert len(set(counts)) == 5, counts
    assert len(M.merge_runs(runs, 0)[0]) == len(flat)
    # zero_seqnos zeroes some and not all of the emitted seqnos at the thresholds inside the range
    for thr in MC.WIDE_THRESHOLDS[1:4]:
        out, src, _ = M.merge_runs(runs, thr, False, True)
        zeroed = sum(1 for it, i in zip(out, src) if it[2] == 0 and flat[i][2] != 0)
        assert 0 < zeroed < len(out)


def test_long_ties_shape():
    runs = MC.long_ties()
    assert [len(r) for r in runs] == [200, 130, 65] and len(MC.TIE_KEY) > 16
    assert len({(it[0], it[2]) for r in runs for it in r}) == 1
    assert len({it[1] for r in runs for it in r}) == 395  # the values tell every item apart
    assert M.merge_runs(runs, 0)[1] == list(range(395))
    assert M.merge_runs(runs, MC.TIE_SEQ + 1)[1] == [0]
    assert [MC.whole_tie_segments(r) for r in runs] == [3, 2, 1]
    orders = MC.long_ties_orders()
    assert len({tuple(len(r) for r in runs) for runs in orders}) == 6
    for runs in orders:
        assert M.merge_runs(runs, 0)[1] == list(range(395))
    many = MC.long_ties_64_runs()
    assert [len(r) for r in many] == [3] * 64 and M.merge_runs(many, 0)[1] == list(range(192))


def test_long_ties_embedded_shape():
    runs = MC.long_ties_embedded()
    # in at least two runs the stretch covers three or more whole segments ...
    assert sum(MC.whole_tie_segments(r) >= 3 for r in runs) >= 2
    for r in runs:  # ... and starts and ends inside a segment, between smaller and larger keys
        at = [i for i, it in enumerate(r) if it[0] == MC.TIE_KEY]
        assert at == list(range(at[0], at[-1] + 1))
        assert at[0] % MC.SEG and (at[-1] + 1) % MC.SEG and at[0] > 0 and at[-1] + 1 < len(r)
        assert r[at[0] - 1][0] < MC.TIE_KEY < r[at[-1] + 1][0]
    stream = M.merge(runs)
    ties = [i for it, i in stream if it[0] == MC.TIE_KEY]
    assert ties == sorted(ties) and len(ties) == 260 + 250 + 65  # lower run first, each run in its own order


def test_shared_heads_shape():
    for head_len, head in ((16, MC.HEAD16), (32, MC.PREFIX32)):
        keys = MC.shared_head_keys(head_len)
        assert 450 <= len(keys) <= 520 and all(k.startswith(head) and len(k) <= head_len + 30 for k in keys)
        assert all(set(k[head_len:]) <= set(MC.HEAD_LETTERS[head_len]) for k in keys)
        pairs = list(zip(keys, keys[1:]))
        differ_at = {MC.first_difference(a, b) for a, b in pairs}
        assert set(MC.HEAD_POSITIONS[head_len]) <= differ_at, sorted(x for x in differ_at if x is not None)
        assert any(b.startswith(a) and len(a) >= 16 and len(b) > len(a) for a, b in pairs)
        runs = MC.shared_heads(head_len)
        flat = [it for r in runs for it in r]
        assert len(runs) == 5 and len(flat) == 3000
        used = sorted({it[0] for it in flat})
        used_pairs = list(zip(used, used[1:]))
        assert set(MC.HEAD_POSITIONS[head_len]) <= {MC.first_difference(a, b) for a, b in used_pairs}
        assert any(b.startswith(a) and len(a) >= 16 for a, b in used_pairs)
        kept = len(M.merge_runs(runs, 500)[0])
        assert len(used) < kept < 3000  # a mid-range threshold: versions dropped and versions kept


def test_state_sets_shape():
    good, bad = MC.state_sorted(), MC.state_unsorted()
    assert [len(r) for r in good] == [len(r) for r in bad] and len(good) == 3
    assert [M.run_is_sorted(r) for r in bad] == [True, False, True]
    assert sorted(it for r in good for it in r) == sorted(it for r in bad for it in r)
    n = sum(len(r) for r in good)
    assert sum(len(r) for r in MC.state_one_run()) < n and len(MC.state_one_run()) == 1
    a, b = len(good[0]), len(good[0]) + len(good[1])
    forms = MC.malformed_run_starts([0, a, b, n])
    assert len(forms) == 5
    for name, (rs, status) in forms.items():
        want = []
        for r in range(3):  # merge_setup_kernel's rule, restated
            s, e = rs[r], rs[r + 1]
            ok = s <= e <= n and (r != 0 or s == 0) and (r != 2 or e == n)
            want.append(0 if ok else 10)
        assert status == want and 10 in status, name


def test_extent_sets_shape():
    runs = MC.nothing_dropped()
    flat = [it for r in runs for it in r]
    out, src, dropped = M.merge_runs(runs, 0)
    assert not dropped and sorted(out) == sorted(flat)
    runs = MC.half_dropped()
    out, src, dropped = M.merge_runs(runs, MC.HALF_DROPPED_THR)
    n = sum(len(r) for r in runs)
    assert 0.35 * n < len(dropped) < 0.65 * n


def test_span_limit_shape():
    for field, at in (("vals", 1), ("keys", 0)):
        for total in (MC.MERGE_BUF - 1, MC.MERGE_BUF, MC.MERGE_BUF + 1):
            for pad in (0, 1, 15):
                runs = MC.span_limit(total, pad, field)
                out, src, dropped = M.merge_runs(runs, 0)
                assert not dropped and len(out) > 2 * MC.SEG
                lens = [len(it[at]) for it in out]
                assert sum(lens[:MC.SEG]) % 16 == pad and sum(lens[MC.SEG:2 * MC.SEG]) == total
                assert max(len(it[0]) for it in out) < MC.MERGE_LONG  # nothing long: the span rule alone
                assert max(len(it[1]) for it in out) < MC.MERGE_LONG  # picks the path
                assert sum(len(it[1 - at]) for it in out[MC.SEG:2 * MC.SEG]) < MC.MERGE_BUF // 4


def test_mixed_keys_shape():
    runs = MC.mixed_keys()
    stream = M.merge(runs)
    kept = set(M.merge_runs(runs, MC.MIXED_KEYS_THR)[1])
    lens = {len(it[0]) for it, _ in stream}
    assert min(lens) == 1 and max(l for l in lens if l <= 20) >= 15 and all(l <= 20 or 250 <= l <= 320 for l in lens)
    assert any(250 <= l < MC.MERGE_LONG for l in lens) and any(l >= MC.MERGE_LONG for l in lens)
    both = 0
    for c in range(0, len(stream), MC.SEG):  # gather steps: 64 merged positions each
        step = stream[c:c + MC.SEG]
        long_kept = any(len(it[0]) >= MC.MERGE_LONG and i in kept for it, i in step)
        long_dropped = any(len(it[0]) >= MC.MERGE_LONG and i not in kept for it, i in step)
        short_kept = any(len(it[0]) <= 20 and i in kept for it, i in step)
        both += long_kept and long_dropped and short_kept
    assert both >= 3


def test_graph_sets_shape():
    first, second, bad = MC.graph_sets()
    size = lambda runs: ([len(r) for r in runs], [len(it[0]) for r in runs for it in r],
                         [len(it[1]) for r in runs for it in r])
    assert size(first) == size(second) == size(bad)
    assert first != second and [M.run_is_sorted(r) for r in bad] == [True, True, False]
    assert M.merge_runs(first, MC.GRAPH_THR)[1] != M.merge_runs(second, MC.GRAPH_THR)[1]
