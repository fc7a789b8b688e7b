"""Reference for the suffix array + LCP array tests: pure Python / numpy, independent of the code under test.

  esa_direct(text)   suffixes sorted directly (the empty suffix first), neighbours compared byte by byte: n <= ~4000
  kasai(text, sa)    the LCP array of a given suffix array (Kasai et al. 2001): larger texts, over a suffix array the
                     existing suite pins (tc_suffix_array)
  unary_lcp(n), periodic_lcp(text, p)   closed forms, a second opinion at the larger sizes

Conventions of include/textcomp.h: sa has n + 1 rows, 0-based starts, row 0 the empty suffix (sa[0] = n); lcp[0] = 0,
lcp[j] = longest common prefix of the suffixes at sa[j - 1] and sa[j]; the end of the text matches nothing."""
import numpy as np


def esa_direct(text):
    t = bytes(text)
    n = len(t)
    sa = sorted(range(n + 1), key=lambda i: t[i:])
    lcp = [0] * (n + 1)
    for j in range(1, n + 1):
        a, b = t[sa[j - 1]:], t[sa[j]:]
        l = 0
        while l < len(a) and l < len(b) and a[l] == b[l]:
            l += 1
        lcp[j] = l
    return np.array(sa, np.uint32), np.array(lcp, np.uint32)


def _match_len(t, a, b, n):
    """longest common prefix of t[a:] and t[b:], by doubling blocks (numpy compares the blocks)"""
    l, step = 0, 64
    while True:
        k = min(step, n - a - l, n - b - l)
        if k <= 0:
            return l
        x, y = t[a + l:a + l + k], t[b + l:b + l + k]
        d = np.flatnonzero(x != y)
        if len(d):
            return l + int(d[0])
        l += k
        step *= 2


def kasai(text, sa):
    """LCP array of suffix array sa (n + 1 rows, row 0 the empty suffix) in text order, h decreasing by at most one a
    step; the byte comparisons go through numpy blocks, so that a long repeat costs no Python loop per byte"""
    t = np.frombuffer(bytes(text), np.uint8) if not isinstance(text, np.ndarray) else text
    n = len(t)
    sa = np.asarray(sa, np.int64)
    rank = np.empty(n + 1, np.int64)
    rank[sa] = np.arange(n + 1)
    lcp = np.zeros(n + 1, np.uint32)
    sal, rankl = sa.tolist(), rank.tolist()
    tb = t.tobytes()
    out = [0] * (n + 1)
    h = 0
    for i in range(n):
        j = sal[rankl[i] - 1]     # rank[i] >= 1: row 0 is the empty suffix
        m = n - max(i, j)
        while h < m and tb[i + h] == tb[j + h]:
            h += 1
            if h & 63 == 0 and h < m:      # a long match: leave the byte loop
                h += _match_len(t, i + h, j + h, n)
                break
        out[rankl[i]] = h
        if h:
            h -= 1
    lcp[:] = out
    return lcp


def unary_lcp(n):
    """text = one byte n times: sa = n, n - 1, .., 0 and lcp[j] = j - 1 (lcp[0] = 0)"""
    lcp = np.arange(-1, n, dtype=np.int64)
    lcp[0] = 0
    return np.arange(n, -1, -1).astype(np.uint32), lcp.astype(np.uint32)


def periodic_lcp_of_rows(sa, n, p):
    """text of period p whose first p bytes are pairwise distinct as ROTATIONS (e.g. a random block: every suffix pair
    at a distance that is a multiple of p agrees to the end of the shorter one): for neighbouring rows whose starts
    differ by a multiple of p, lcp = n - max of the two starts.  -> (mask of such rows, their lcp)"""
    sa = np.asarray(sa, np.int64)
    a, b = sa[:-1], sa[1:]
    mask = np.zeros(len(sa), bool)
    val = np.zeros(len(sa), np.uint32)
    same = ((a - b) % p == 0) & (a < n) & (b < n)
    mask[1:] = same
    val[1:][same] = (n - np.maximum(a, b))[same]
    return mask, val
