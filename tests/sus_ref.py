"""CPU reference of the unique-substring calls (tc_unique_prefixes, tc_unique_substrings, tc_shortest_unique; include/textcomp.h
has the definitions), written twice:

  brute(t)                 straight from the definitions, for short texts: every substring is counted (overlaps included); up, the
                           MUS list and the point answers are read off the counts, the point answers by trying every unique
                           substring over the position;
  from_esa(sa, lcp, n)     numpy over the suffix array and the LCP array (N = n + 1 rows, as tc_lcp_array defines them): up by
                           scatter, the MUS rule vectorised, the point answers from the three candidates -- the predecessor and the
                           successor by searchsorted over the ends and the starts, the shortest covering MUS by a sparse table over
                           len << 32 | index, so that the minimum is the leftmost of its length.
  esa(t)                   its own suffix sort (prefix doubling in numpy) and LCP array (Kasai's loop) for small n -- some
                           ten thousand bytes -- so that this file needs nothing else.

tests/test_sus_ref.py holds the two together.  No oracle is involved: the reference has no such operation."""
import numpy as np


def esa(t):
    """(sa, lcp) of t, N = n + 1 rows, row 0 the empty suffix, lcp[0] = 0"""
    t = bytes(t)
    n = len(t)
    if n == 0:
        return np.array([0], np.uint32), np.array([0], np.uint32)
    # prefix doubling: rank[i] = the rank of t[i : i + k], 1-based, 0 behind the end (the end of the text sorts first)
    rank = np.frombuffer(t, np.uint8).astype(np.int64) + 1
    k = 1
    while True:
        nxt = np.zeros(n, np.int64)
        nxt[:n - k] = rank[k:]
        order = np.lexsort((nxt, rank))
        key = rank[order] * (max(n, 256) + 2) + nxt[order]
        new = np.empty(n, np.int64)
        new[order] = np.cumsum(np.append(1, key[1:] != key[:-1]))
        rank = new
        if int(rank.max()) == n or k >= n:
            break
        k *= 2
    order = np.argsort(rank, kind="stable")
    sa = [n] + order.tolist()
    isa = (rank).tolist()                               # the row of suffix i (row 0 is the empty suffix)
    lcp = [0] * (n + 1)
    h = 0
    for i in range(n):                                  # Kasai's loop
        j = sa[isa[i] - 1]
        if isa[i] == 1:
            h = 0
            continue
        while i + h < n and j + h < n and t[i + h] == t[j + h]:
            h += 1
        lcp[isa[i]] = h
        if h:
            h -= 1
    return np.array(sa, np.uint32), np.array(lcp, np.uint32)


def unique_prefixes(sa, lcp, n):
    sa = np.asarray(sa, np.int64)
    lcp = np.asarray(lcp, np.int64)
    up = np.zeros(n, np.uint32)
    if n == 0:
        return up
    m = np.maximum(lcp, np.append(lcp[1:], 0))[1:]      # rows 1 .. n
    i = sa[1:]
    up[i] = np.where(i + m < n, m + 1, 0)
    return up


def mus_from_up(up, min_len=1, max_len=0):
    """-> (start, len) uint32, by increasing start"""
    up = np.asarray(up, np.int64)
    nxt = np.append(up[1:], 0)
    is_mus = (up != 0) & ((nxt == 0) | (nxt >= up))
    keep = is_mus & (up >= min_len) & ((up <= max_len) if max_len else True)
    s = np.nonzero(keep)[0]
    return s.astype(np.uint32), up[s].astype(np.uint32)


def point_from_mus(ms, ml, n):
    """-> (start, len) uint32 of the shortest unique substring over every position, from the whole MUS list"""
    ms = np.asarray(ms, np.int64)
    ml = np.asarray(ml, np.int64)
    if n == 0:
        return np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    me = ms + ml - 1
    K = len(ms)
    assert K >= 1 and (np.diff(ms) > 0).all() and (np.diff(me) > 0).all()
    p = np.arange(n, dtype=np.int64)
    big = np.int64(1) << 62
    ipred = np.searchsorted(me, p, side="left") - 1     # the last MUS that ends before p
    isucc = np.searchsorted(ms, p, side="right")        # the first MUS that starts behind p
    best = np.full(n, big)
    hp = ipred >= 0
    sp = ms[np.maximum(ipred, 0)]
    best = np.where(hp, np.minimum(best, (p - sp + 1) << 32 | sp), best)
    hs = isucc < K
    es = me[np.minimum(isucc, K - 1)]
    best = np.where(hs, np.minimum(best, (es - p + 1) << 32 | p), best)
    # the covering ones are the MUS ipred + 1 .. isucc - 1: the minimum of len << 32 | index over that range
    key = ml << 32 | np.arange(K, dtype=np.int64)
    table = [key]
    w = 1
    while 2 * w <= K:
        prev = table[-1]
        table.append(np.minimum(prev[:-w], prev[w:]))
        w *= 2
    lo, hi = ipred + 1, isucc - 1
    has = lo <= hi
    span = np.where(has, hi - lo + 1, 1)
    lev = np.floor(np.log2(span)).astype(np.int64)
    cov = np.full(n, big)
    for j, tab in enumerate(table):
        sel = has & (lev == j)
        if sel.any():
            a = lo[sel]
            b = hi[sel] - (1 << j) + 1
            cov[sel] = np.minimum(tab[a], tab[b])
    ci = cov & 0xFFFFFFFF
    cand = (cov >> 32) << 32 | ms[np.where(has, ci, 0)]
    best = np.where(has, np.minimum(best, cand), best)
    assert (best < big).all()
    return (best & 0xFFFFFFFF).astype(np.uint32), (best >> 32).astype(np.uint32)


def from_esa(sa, lcp, n):
    """-> up, (mus_start, mus_len), (sus_start, sus_len)"""
    up = unique_prefixes(sa, lcp, n)
    ms, ml = mus_from_up(up)
    return up, (ms, ml), point_from_mus(ms, ml, n)


def reference(t):
    t = bytes(t)
    sa, lcp = esa(t)
    return from_esa(sa, lcp, len(t))


def brute(t):
    """up, [(s, len)] of the MUS, [(s, len)] of the point answers -- by counting every substring"""
    t = bytes(t)
    n = len(t)
    cnt = {}
    for i in range(n):
        for j in range(i + 1, n + 1):
            cnt[t[i:j]] = cnt.get(t[i:j], 0) + 1
    occ = lambda w: 2 if not w else cnt.get(w, 0)       # the empty string counts as occurring twice
    up = [0] * n
    for i in range(n):
        for l in range(1, n - i + 1):
            if cnt[t[i:i + l]] == 1:
                up[i] = l
                break
    mus = []
    for s in range(n):
        for l in range(1, n - s + 1):
            w = t[s:s + l]
            if cnt[w] == 1 and occ(w[1:]) >= 2 and occ(w[:-1]) >= 2:
                mus.append((s, l))
    point = []
    for p in range(n):
        best = None
        for s in range(p + 1):
            for l in range(p - s + 1, n - s + 1):
                if cnt[t[s:s + l]] == 1:
                    if best is None or (l, s) < best:
                        best = (l, s)
                    break
        point.append((best[1], best[0]))
    return up, mus, point


def fibonacci(n):
    a, b = b"a", b"ab"
    while len(b) < n:
        a, b = b, b + a
    return b[:n]


def staircase(seed=7, base=200, steps=140, stride=4):
    """many MUS over one position, the shortest of them in the middle: A, then per step a separator byte and a copy of a
    stretch of A that starts `stride` further right and whose length wanders"""
    import random
    rng = random.Random(seed)
    A = bytes(rng.choice(b"ACGT") for _ in range(2 * base + steps * stride + 8))
    out = bytearray(A)
    ln = base + steps
    for k in range(steps):
        if k:
            ln = max(base, ln + rng.randint(-(stride - 1), stride - 1))
        out.append(128 + k % 100)
        out += A[k * stride:k * stride + ln]
    out.append(255)
    return bytes(out)
