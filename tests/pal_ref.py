"""The palindromes and inverted repeats of a text, with mismatches, written twice for the tests of tc_palindromes
(include/textcomp.h has the definition).  brute(t, ...) is the definition itself over every substring: count the mismatching
pairs, keep those within the budget whose outermost pair matches, and of each centre the longest; cubic, for texts of a few
dozen bytes.  palindromes(t, ...) is a numpy method -- all centres are extended together, one array step per radius, each
centre carrying its mismatch count and the last radius whose pair matched -- with a closed form for unary texts, where the
radii are as long as the text; its output is in the order the call writes: increasing centre.  tests/test_pal_ref.py holds
the two together."""
import numpy as np

IDENTITY = np.arange(256, dtype=np.uint8)
DNA = IDENTITY.copy()
for _a, _b in (b"AT", b"CG", b"at", b"cg"):
    DNA[_a], DNA[_b] = _b, _a


def _u8(t):
    if isinstance(t, str):
        t = t.encode()
    if isinstance(t, (bytes, bytearray)):
        return np.frombuffer(bytes(t), np.uint8)
    return np.ascontiguousarray(t, dtype=np.uint8)


def _sigma(comp):
    s = IDENTITY if comp is None else _u8(comp)
    assert len(s) == 256 and np.array_equal(s[s], IDENTITY), "comp is not an involution"
    return s


def brute(t, comp=None, max_mismatch=0, min_len=1):
    """every (start, len, mm) of the definition, by increasing centre"""
    t = bytes(_u8(t))
    s_ = _sigma(comp).tolist()
    n = len(t)
    best = {}
    for s in range(n):
        for ln in range(1, n - s + 1):
            mm = sum(1 for k in range((ln + 1) // 2) if t[s + k] != s_[t[s + ln - 1 - k]])
            if mm > max_mismatch or t[s] != s_[t[s + ln - 1]] or ln < min_len:
                continue
            c = 2 * s + ln - 1
            if c not in best or best[c][1] < ln:
                best[c] = (s, ln, mm)
    return [best[c] for c in sorted(best)]


def _words(t, sigma, m):
    """per centre: (the radius of the longest palindrome, 0 for none; its mismatches)"""
    n = len(t)
    c = np.arange(max(2 * n - 1, 0), dtype=np.int64)
    l0, r0 = c // 2, (c + 1) // 2
    bound = np.minimum(l0 + 1, n - r0)
    best = np.zeros(len(c), np.int64)
    best_mm = np.zeros(len(c), np.int64)
    if n and (t == t[0]).all():                     # unary: every pair matches, or none does
        if sigma[t[0]] == t[0]:
            best = bound.copy()
        return best, best_mm
    live = c.copy()
    mm = np.zeros(len(c), np.int64)
    k = 0
    st = sigma[t]
    while len(live):
        live = live[bound[live] > k]
        miss = t[l0[live] - k] != st[r0[live] + k]
        mm[live] += miss
        hit = live[~miss]
        best[hit] = k + 1
        best_mm[hit] = mm[hit]
        live = live[mm[live] <= m]
        k += 1
    return best, best_mm


def palindromes(t, comp=None, max_mismatch=0, min_len=1):
    """(pal_start, pal_len, pal_mm), three uint32 arrays, as tc_palindromes writes them"""
    t = _u8(t)
    best, best_mm = _words(t, _sigma(comp), max_mismatch)
    c = np.arange(len(best), dtype=np.int64)
    ln = 2 * best - 1 + (c & 1)
    keep = (best > 0) & (ln >= min_len)
    return (((c + 1 - ln) // 2)[keep].astype(np.uint32), ln[keep].astype(np.uint32), best_mm[keep].astype(np.uint32))


def longest(t, comp=None, max_mismatch=0):
    """(start, len, mm) of the longest palindrome, of equal lengths the one with the smallest centre; (0, 0, 0) for none"""
    s, ln, mm = palindromes(t, comp, max_mismatch)
    if not len(ln):
        return 0, 0, 0
    k = int(np.argmax(ln))                          # (the first of the maxima: the list is in increasing centre)
    return int(s[k]), int(ln[k]), int(mm[k])


def as_triples(start, length, mm):
    return [(int(s), int(l), int(m)) for s, l, m in zip(start, length, mm)]


def fibonacci(k):
    """the Fibonacci string of length F_k (F_1 = F_2 = 1): b, a, ab, aba, abaab, ..."""
    a, b = b"b", b"a"
    if k <= 1:
        return a
    for _ in range(k - 2):
        a, b = b, b + a
    return b


def planted(rng, n, comp=None, count=6):
    """random ACGT of n bytes with palindromes under comp planted into it: one touches position 0, one position n - 1, and
    they carry 0 .. 3 substitutions, some right next to the centre and some at the outer edge"""
    sigma = _sigma(comp)
    t = rng.choice(np.frombuffer(b"ACGT", np.uint8), n).astype(np.uint8)
    if n < 8:
        return t
    top = max(min(n // 3, 60), 4)
    for j in range(count):
        ln = int(rng.integers(4, top + 1))
        s = 0 if j == 0 else n - ln if j == 1 else int(rng.integers(0, n - ln + 1))
        half = rng.choice(np.frombuffer(b"ACGT", np.uint8), (ln + 1) // 2).astype(np.uint8)
        w = np.concatenate((half, sigma[half[::-1]][ln & 1:]))
        for e in range(j % 4):                      # substitutions: next to the centre, at the edge, anywhere
            at = (ln // 2 - 1, 0, int(rng.integers(0, ln)))[(j + e) % 3]
            w[at] = ord("ACGT"[(b"ACGT".index(bytes([w[at]])) + 1) % 4])
        t[s:s + ln] = w
    return t
