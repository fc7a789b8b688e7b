"""CPU reference of the queries on a kept enhanced suffix array (tc_esa_lce, tc_esa_find, tc_esa_compare; include/textcomp.h has the
definitions), in numpy: a suffix array by prefix doubling (the empty suffix is row 0), the LCP array by Kasai's walk, the inverse
permutation, and a sparse table of minima over lcp and over sa, so that a batch of queries is a handful of array operations:

  Ref(t).lce(a, b, m)              -> (len, mm): at most m + 1 exact extensions, each a range minimum over lcp between two rows;
  Ref(t).find(start, length)       -> (first_row, occ, first_pos): the interval by two binary searches over range minima of lcp
                                      around the row of `start`, the earliest occurrence as the range minimum of sa over it;
  Ref(t).compare(a, la, b, lb)     -> (order, common): the exact extension clamped to both lengths, then one byte or the lengths.

tests/test_esa_ref.py holds all three to loops over the bytes.  No oracle is involved: the reference has no such operation."""
import numpy as np


def suffix_array(t):
    """sa of n + 1 rows, row 0 the empty suffix (a proper prefix sorts first), by prefix doubling"""
    a = np.frombuffer(bytes(t), np.uint8).astype(np.int64)
    n = len(a)
    rank = np.concatenate((a + 1, [0]))             # position n: the empty suffix, below every byte
    N = n + 1
    sa = np.argsort(rank, kind="stable")
    k = 1
    while True:
        second = np.zeros(N, np.int64)
        second[:N - k] = rank[k:] + 1 if k < N else 0
        sa = np.lexsort((second, rank))
        key = rank[sa] * (N + 2) + second[sa]
        new = np.zeros(N, np.int64)
        new[sa] = np.concatenate(([0], np.cumsum(key[1:] != key[:-1])))
        rank = new
        if rank.max() == N - 1 or k >= N:
            break
        k *= 2
    return sa.astype(np.int64)


def lcp_array(t, sa):
    """lcp[r] = the common prefix of the suffixes of rows r - 1 and r, lcp[0] = 0 (Kasai)"""
    t = bytes(t)
    n = len(t)
    N = n + 1
    isa = np.empty(N, np.int64)
    isa[sa] = np.arange(N)
    lcp = [0] * N
    sal, isal = sa.tolist(), isa.tolist()
    h = 0
    for i in range(n):
        r = isal[i]                                 # r >= 1: only the empty suffix has row 0
        j = sal[r - 1]
        while i + h < n and j + h < n and t[i + h] == t[j + h]:
            h += 1
        lcp[r] = h
        if h:
            h -= 1
    return np.array(lcp, np.int64), isa


class _Sparse:
    """range minima of one array"""

    def __init__(self, v):
        self.lev = [np.asarray(v, np.int64)]
        k = 1
        while 2 * k <= len(v):
            p = self.lev[-1]
            self.lev.append(np.minimum(p[:len(p) - k], p[k:]))
            k *= 2

    def query(self, lo, hi):
        """min v[lo .. hi] (inclusive, lo <= hi), arrays"""
        lo, hi = np.asarray(lo, np.int64), np.asarray(hi, np.int64)
        out = np.empty(len(lo), np.int64)
        k = np.floor(np.log2(np.maximum(hi - lo + 1, 1))).astype(np.int64)
        for lv in np.unique(k):
            m = k == lv
            tab = self.lev[int(lv)]
            out[m] = np.minimum(tab[lo[m]], tab[hi[m] - (1 << int(lv)) + 1])
        return out


class Ref:
    def __init__(self, t):
        self.t = bytes(t)
        self.n = len(self.t)
        self.N = self.n + 1
        self.bytes = np.frombuffer(self.t + b"\0", np.uint8).astype(np.int64)
        self.sa = suffix_array(self.t)
        self.lcp, self.isa = lcp_array(self.t, self.sa)
        self._lcp = _Sparse(self.lcp)
        self._sa = _Sparse(self.sa)

    def _exact(self, a, b):
        """the longest common prefix of the suffixes a and b (0 .. n each)"""
        out = np.zeros(len(a), np.int64)
        same = a == b
        out[same] = self.n - a[same]
        d = ~same
        ra, rb = self.isa[a[d]], self.isa[b[d]]
        out[d] = self._lcp.query(np.minimum(ra, rb) + 1, np.maximum(ra, rb))
        return out

    def lce(self, a, b, m=0):
        a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
        assert ((a >= 0) & (a <= self.n) & (b >= 0) & (b <= self.n)).all()
        bound = self.n - np.maximum(a, b)
        R = np.zeros(len(a), np.int64)
        mm = np.zeros(len(a), np.int64)
        for turn in range(m + 1):
            R = R + np.minimum(self._exact(a + R, b + R), bound - R)
            if turn == m:
                break
            hit = R < bound                         # position R is a mismatch
            R[hit] += 1
            mm[hit] += 1
        return R.astype(np.uint32), mm.astype(np.uint32)

    def find(self, start, length):
        s, l = np.asarray(start, np.int64), np.asarray(length, np.int64)
        assert ((s >= 0) & (l >= 0) & (s + l <= self.n)).all()
        nq = len(s)
        r = self.isa[s]
        # lo = the smallest row with min lcp[lo + 1 .. r] >= l; hi = the largest with min lcp[r + 1 .. hi - 1] >= l
        lo_a, lo_b = np.zeros(nq, np.int64), r.copy()
        while (lo_a < lo_b).any():
            mid = (lo_a + lo_b) // 2
            act = lo_a < lo_b
            ok = np.ones(nq, bool)
            q = act & (mid < r)
            ok[q] = self._lcp.query(mid[q] + 1, r[q]) >= l[q]
            lo_b = np.where(act & ok, mid, lo_b)
            lo_a = np.where(act & ~ok, mid + 1, lo_a)
        hi_a, hi_b = r + 1, np.full(nq, self.N, np.int64)
        while (hi_a < hi_b).any():
            mid = (hi_a + hi_b + 1) // 2            # is hi >= mid: min lcp[r + 1 .. mid - 1] >= l
            act = hi_a < hi_b
            ok = np.ones(nq, bool)
            q = act & (mid - 1 > r)
            ok[q] = self._lcp.query(r[q] + 1, mid[q] - 1) >= l[q]
            hi_a = np.where(act & ok, mid, hi_a)
            hi_b = np.where(act & ~ok, mid - 1, hi_b)
        lo, hi = lo_a, hi_a
        z = l == 0
        lo[z], hi[z] = 0, self.N
        pos = self._sa.query(lo, hi - 1)
        pos[z] = 0
        return lo.astype(np.uint32), (hi - lo).astype(np.uint32), pos.astype(np.uint32)

    def compare(self, a, la, b, lb):
        a, la, b, lb = (np.asarray(x, np.int64) for x in (a, la, b, lb))
        assert ((a >= 0) & (la >= 0) & (a + la <= self.n) & (b >= 0) & (lb >= 0) & (b + lb <= self.n)).all()
        lim = np.minimum(la, lb)
        c = np.minimum(self._exact(a, b), lim)
        order = np.sign(la - lb)
        d = c < lim
        order[d] = np.where(self.bytes[a[d] + c[d]] < self.bytes[b[d] + c[d]], -1, 1)
        return order.astype(np.int8), c.astype(np.uint32)


# ---- straight from the definitions, by loops over the bytes: what tests/test_esa_ref.py holds the above to
def brute_lce(t, a, b, m):
    n = len(t)
    L = mm = 0
    while a + L < n and b + L < n:
        if t[a + L] != t[b + L]:
            if mm == m:
                break
            mm += 1
        L += 1
    return L, mm


def brute_find(t, s, l):
    """(first_row, occ, first_pos) with the rows counted among the sorted suffixes, the empty one first"""
    n = len(t)
    w = t[s:s + l]
    sufs = sorted(range(n + 1), key=lambda i: t[i:])
    rows = [r for r, i in enumerate(sufs) if t[i:i + l] == w and i + l <= n]
    if l == 0:
        return 0, n + 1, 0
    return rows[0], len(rows), min(sufs[r] for r in rows)


def brute_compare(t, a, la, b, lb):
    x, y = t[a:a + la], t[b:b + lb]
    c = 0
    while c < len(x) and c < len(y) and x[c] == y[c]:
        c += 1
    return (x > y) - (x < y), c


def fibonacci(n):
    a, b = b"a", b"ab"
    while len(b) < n:
        a, b = b, b + a
    return b[:n]
