"""CPU-only: the reference of the kept-ESA query tests (tests/esa_ref.py) against loops over the bytes -- on every text over {a, b}
up to 7 bytes and on seeded random, Fibonacci, periodic and unary texts up to about 200 bytes: every pair (a, b) for the longest
common extension at 0, 1, 2 and 16 mismatches, every (start, len) for find, and compare on every pair of substrings of the short
texts and on sampled pairs of the long ones; its arrays against a direct sort; and the worked examples of include/textcomp.h."""
import itertools

import numpy as np

import esa_ref as R

MS = (0, 1, 2, 16)


def _texts():
    rng = np.random.default_rng(0xE5A0)
    for n in (1, 2, 3, 17, 64, 150, 200):
        for sigma in (2, 4):
            yield bytes(b"acgt"[int(c)] for c in rng.integers(0, sigma, n))
    yield bytes(rng.integers(0, 256, 120, dtype=np.uint8))
    yield from (R.fibonacci(144), R.fibonacci(55), b"ab" * 40, b"abc" * 33 + b"a", b"abcde" * 9, b"a" * 60, b"a" * 1, b"b" + b"a" * 50)


def _check_arrays(t, ref):
    n = len(t)
    sufs = sorted(range(n + 1), key=lambda i: t[i:])
    assert ref.sa.tolist() == sufs
    assert ref.isa[ref.sa].tolist() == list(range(n + 1))
    for r in range(n + 1):
        want = 0 if r == 0 else R.brute_lce(t, sufs[r - 1], sufs[r], 0)[0]
        assert int(ref.lcp[r]) == want


def _check_lce(t, ref, pairs):
    a = np.array([p[0] for p in pairs])
    b = np.array([p[1] for p in pairs])
    for m in MS:
        ln, mm = ref.lce(a, b, m)
        want = [R.brute_lce(t, x, y, m) for x, y in pairs]
        assert ln.tolist() == [w[0] for w in want], (t, m)
        assert mm.tolist() == [w[1] for w in want], (t, m)


def _check_find(t, ref, queries, sufs):
    s = np.array([q[0] for q in queries])
    l = np.array([q[1] for q in queries])
    row, occ, pos = ref.find(s, l)
    n = len(t)
    for k, (s0, l0) in enumerate(queries):
        if l0 == 0:
            want = (0, n + 1, 0)
        else:
            w = t[s0:s0 + l0]
            rows = [r for r, i in enumerate(sufs) if t[i:i + l0] == w]
            assert rows == list(range(rows[0], rows[0] + len(rows)))        # an interval
            want = (rows[0], len(rows), min(sufs[r] for r in rows))
        assert (int(row[k]), int(occ[k]), int(pos[k])) == want, (t, s0, l0)


def _check_compare(t, ref, quads):
    a, la, b, lb = (np.array([q[k] for q in quads]) for k in range(4))
    order, common = ref.compare(a, la, b, lb)
    want = [R.brute_compare(t, *q) for q in quads]
    assert order.tolist() == [w[0] for w in want], t
    assert common.tolist() == [w[1] for w in want], t


def _all(t, all_compares):
    n = len(t)
    ref = R.Ref(t)
    _check_arrays(t, ref)
    sufs = ref.sa.tolist()
    _check_lce(t, ref, [(a, b) for a in range(n + 1) for b in range(n + 1)])
    subs = [(s, l) for s in range(n + 1) for l in range(n - s + 1)]
    _check_find(t, ref, subs, sufs)
    if all_compares:
        quads = [x + y for x in subs for y in subs]
    else:
        rng = np.random.default_rng(len(t))
        idx = rng.integers(0, len(subs), (3000, 2))
        quads = [subs[i] + subs[j] for i, j in idx] + [x + x for x in subs[:200]]
        quads += [(s, l, s2, l) for (s, l) in subs[::7] for s2 in range(0, n - l + 1, max(1, n // 5))]      # equal lengths, other places
    _check_compare(t, ref, quads)


def test_every_binary_text_up_to_7():
    for n in range(0, 8):
        for t in itertools.product(b"ab", repeat=n):
            _all(bytes(t), n <= 5)


def test_random_fibonacci_periodic_and_unary_texts():
    for t in _texts():
        _all(t, False)


def test_brute_find_agrees_with_the_interval_form():
    for t in (b"mississippi", b"abab", b"aaaa"):
        ref = R.Ref(t)
        subs = [(s, l) for s in range(len(t) + 1) for l in range(len(t) - s + 1)]
        row, occ, pos = ref.find([s for s, _ in subs], [l for _, l in subs])
        for k, (s, l) in enumerate(subs):
            assert (int(row[k]), int(occ[k]), int(pos[k])) == R.brute_find(t, s, l)


def test_worked_examples():
    ref = R.Ref(b"mississippi")
    assert ref.sa.tolist() == [11, 10, 7, 4, 1, 0, 9, 8, 6, 3, 5, 2]
    assert ref.lcp.tolist() == [0, 0, 1, 1, 4, 0, 0, 1, 0, 2, 1, 3]
    for m, want in ((0, (4, 0)), (1, (5, 1)), (2, (7, 2)), (16, (7, 2))):
        ln, mm = ref.lce([1], [4], m)
        assert (int(ln[0]), int(mm[0])) == want
    assert [int(x[0]) for x in ref.lce([0], [0], 0)] == [11, 0]
    assert [int(x[0]) for x in ref.lce([3], [11], 3)] == [0, 0]
    assert [tuple(int(v) for v in col) for col in zip(*ref.find([1, 2, 0], [4, 1, 0]))] == [(3, 2, 1), (8, 4, 2), (0, 12, 0)]
    order, common = ref.compare([1, 1, 8], [4, 4, 2], [4, 4, 5], [4, 3, 2])
    assert order.tolist() == [0, 1, -1] and common.tolist() == [4, 3, 0]
    empty = R.Ref(b"")
    assert empty.sa.tolist() == [0] and empty.lcp.tolist() == [0]
    assert [int(x[0]) for x in empty.lce([0], [0], 2)] == [0, 0]
    assert [int(x[0]) for x in empty.find([0], [0])] == [0, 1, 0]
    assert [int(x[0]) for x in empty.compare([0], [0], [0], [0])] == [0, 0]
