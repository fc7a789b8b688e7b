"""CPU-only: the two references of tests/tr_ref.py agree -- the definition of a run taken literally (brute) and the numpy
shift method (runs) that the device tests compare tc_tandem_repeats with -- on every binary text up to 12 bytes, on the
examples of include/textcomp.h and on Fibonacci strings, whose number of runs is known in closed form: the string of length
F_k has 2 F_(k-2) - 3 of them."""
import itertools

import numpy as np

import tr_ref


def _runs(t, **kw):
    return tr_ref.as_triples(*tr_ref.runs(t, **kw))


def test_header_examples():
    assert tr_ref.brute(b"mississippi") == [(1, 7, 3), (2, 3, 1), (5, 6, 1), (8, 9, 1)]
    assert tr_ref.brute(b"aabaabaab") == [(0, 1, 1), (0, 8, 3), (3, 4, 1), (6, 7, 1)]
    for t in (b"mississippi", b"aabaabaab"):
        assert _runs(t) == tr_ref.brute(t)
    for n in range(0, 9):
        want = [(0, n - 1, 1)] if n >= 2 else []
        assert tr_ref.brute(b"a" * n) == want and _runs(b"a" * n) == want


def test_every_binary_text_up_to_12_bytes():
    for n in range(0, 13):
        for bits in itertools.product(b"ab", repeat=n):
            t = bytes(bits)
            got = _runs(t)
            assert got == tr_ref.brute(t), t
            assert len(got) < max(n, 1)             # the runs theorem


def test_fibonacci_strings():
    fib = [0, 1, 1]
    while len(fib) <= 16:
        fib.append(fib[-1] + fib[-2])
    for k in range(5, 17):
        t = tr_ref.fibonacci(k)
        assert len(t) == fib[k]
        got = _runs(t)
        assert len(got) == 2 * fib[k - 2] - 3, k
        if k <= 9:                                  # 34 bytes: the definition is still affordable
            assert got == tr_ref.brute(t)
    # eleven runs share one start in the string of 987 bytes
    start = tr_ref.runs(tr_ref.fibonacci(16))[0]
    assert np.bincount(start).max() == 11


def test_order_and_filters():
    t = b"aabaabaab" + b"acacacac" + b"tttttt"
    s, l, p = tr_ref.runs(t)
    keys = list(zip(s.tolist(), p.tolist()))
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    everything = set(tr_ref.as_triples(s, l, p))
    for kw in (dict(min_period=2), dict(max_period=1), dict(min_copies=3), dict(min_len=7), dict(min_period=2, max_period=2, min_len=8)):
        want = {r for r in everything if tr_ref.passes(r[1] - r[0] + 1, r[2], **kw)}
        assert 0 < len(want) < len(everything), kw
        assert set(_runs(t, **kw)) == want, kw
