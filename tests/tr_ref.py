"""The runs (maximal repetitions) of a text, written twice for the tests of tc_tandem_repeats (include/textcomp.h has the
definition).  brute(t) is the definition itself, condition by condition, over every triple (s, e, p): cubic and worse, for
texts of a few dozen bytes.  runs(t, ...) is a numpy shift method -- for every period p the maximal stretches of
t[k] == t[k + p], kept where they are at least p long and no proper divisor of p is a period of the stretch as well -- and
applies the four filters; its output is in the order the call writes: increasing start, then increasing period.
tests/test_tr_ref.py holds the two together."""
import numpy as np


def _u8(t):
    if isinstance(t, str):
        t = t.encode()
    if isinstance(t, (bytes, bytearray)):
        return np.frombuffer(bytes(t), np.uint8)
    return np.ascontiguousarray(t, dtype=np.uint8)


def brute(t):
    """every (start, end, period) of the definition, sorted by (start, period)"""
    t = bytes(_u8(t))
    n = len(t)
    out = []
    for s in range(n):
        for e in range(s, n):
            w = t[s:e + 1]
            for p in range(1, (e - s + 1) // 2 + 1):
                if any(t[k] != t[k + p] for k in range(s, e - p + 1)):
                    continue
                if any(all(w[k] == w[k + q] for k in range(len(w) - q)) for q in range(1, p)):
                    continue        # p is not the smallest period of text[s..e]
                if s > 0 and t[s - 1] == t[s + p - 1]:
                    continue
                if e < n - 1 and t[e + 1] == t[e + 1 - p]:
                    continue
                out.append((s, e, p))
    return sorted(out, key=lambda r: (r[0], r[2]))


def passes(length, period, min_period=1, max_period=0, min_copies=2, min_len=1):
    return (period >= min_period and (max_period == 0 or period <= max_period) and length // period >= min_copies
            and length >= min_len)


def runs(t, min_period=1, max_period=0, min_copies=2, min_len=1):
    """(run_start, run_len, run_period), three uint32 arrays, as tc_tandem_repeats writes them"""
    t = _u8(t)
    n = len(t)
    found = []
    top = n // 2 if max_period == 0 else min(n // 2, max_period)
    for p in range(max(min_period, 1), top + 1):
        eq = np.concatenate(([0], (t[:-p] == t[p:]).astype(np.int8), [0]))
        edge = np.flatnonzero(np.diff(eq))          # stretches [edge[2k], edge[2k + 1]) of equal pairs
        first, behind = edge[0::2], edge[1::2]
        long_enough = behind - first >= p
        for a, b in zip(first[long_enough].tolist(), behind[long_enough].tolist()):
            s, e = a, b - 1 + p                     # the run text[s..e]
            w = t[s:e + 1]
            if any(p % q == 0 and np.array_equal(w[:-q], w[q:]) for q in range(1, p // 2 + 1)):
                continue
            if passes(e - s + 1, p, min_period, max_period, min_copies, min_len):
                found.append((s, p, e - s + 1))
    found.sort()
    a = np.array(found, dtype=np.uint32).reshape(-1, 3)
    return a[:, 0].copy(), a[:, 2].copy(), a[:, 1].copy()


def as_triples(start, length, period):
    """(start, end, period) tuples of three arrays"""
    return [(int(s), int(s) + int(l) - 1, int(p)) for s, l, p in zip(start, length, period)]


def fibonacci(k):
    """the Fibonacci string of length F_k (F_1 = F_2 = 1): b, a, ab, aba, abaab, ..."""
    a, b = b"b", b"a"
    if k <= 1:
        return a
    for _ in range(k - 2):
        a, b = b, b + a
    return b
