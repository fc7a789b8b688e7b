"""Brute-force reference of FM-index matching statistics and maximal exact matches (numpy and Python bytes only; shares
nothing with the code under test, and does not shrink intervals or look at an LCP array).

For a pattern p and every position i: ms_len[i] = the largest l such that p[i : i + l] occurs in the text t -- found by
substring search (`in`; occurring is monotone in l, so the largest l is searched by bisection); ms_pos[i] = the 1-based
text position of the occurrence whose suffix is the first among the directly sorted suffixes of t, the empty suffix
included and first (Python's bytes order puts a proper prefix first, which is exactly that); ms_occ[i] = the overlapping
occurrences of p[i : i + l] in t, counted one by one.  All three are 0 where p[i] does not occur in t.

Maximal exact matches: the pairs (i, l), l >= 1, such that p[i : i + l] occurs in t and no other such pair (i2, l2)
contains it (i2 <= i and i2 + l2 >= i + l).  mems_enumerated() lists them exactly so, from nothing but `in` -- quartic, for
small patterns.  Because every prefix and every suffix of an occurring string occurs, (i, l) is contained in no other pair
exactly when l = ms_len[i] (it cannot grow to the right) and i = 0 or ms_len[i - 1] <= ms_len[i] (ms_len[i - 1] >
ms_len[i] would mean p[i - 1 : i + ms_len[i]] occurs: it grows to the left; ms_len[i - 1] <= ms_len[i] + 1 always).
mems_by_rule() applies that rule to a ms_len array; tests assert both equal where the enumeration is affordable."""
import bisect

import numpy as np


class Ref:
    """the directly sorted suffixes of one text"""

    def __init__(self, t):
        self.t = t = bytes(t)
        n = len(t)
        self.sa = sorted(range(n + 1), key=lambda i: t[i:])
        self.suffixes = [t[i:] for i in self.sa]

    def longest(self, p, i):
        """largest l with p[i : i + l] in t"""
        t = self.t
        lo, hi = 0, min(len(p) - i, len(t))          # p[i : i + lo] occurs; nothing longer than hi can
        while lo < hi:
            mid = (lo + hi + 1) // 2
            if p[i:i + mid] in t:
                lo = mid
            else:
                hi = mid - 1
        return lo

    def first_row(self, w):
        """the first row among the sorted suffixes whose suffix starts with w (w occurs)"""
        j = bisect.bisect_left(self.suffixes, w)
        assert self.suffixes[j].startswith(w)
        return j

    def occurrences(self, w):
        t, k, i = self.t, 0, self.t.find(w)
        while i >= 0:
            k += 1
            i = t.find(w, i + 1)
        return k

    def match_stats_one(self, p):
        p = bytes(p)
        out = []
        for i in range(len(p)):
            l = self.longest(p, i)
            if l == 0:
                out.append((0, 0, 0))
            else:
                w = p[i:i + l]
                out.append((l, self.sa[self.first_row(w)] + 1, self.occurrences(w)))
        return out

    def match_stats(self, pats):
        """-> (ms_len uint32, ms_pos uint64, ms_occ uint32), each [total pattern bytes], pattern after pattern"""
        rows = [r for p in pats for r in self.match_stats_one(p)]
        a = np.array(rows, np.uint64).reshape(-1, 3)
        return a[:, 0].astype(np.uint32), a[:, 1].astype(np.uint64), a[:, 2].astype(np.uint32)

    def mems_enumerated(self, p):
        """[(i, l)] by enumeration, in increasing i"""
        p, t = bytes(p), self.t
        m = len(p)
        occ = [(i, l) for i in range(m) for l in range(1, m - i + 1) if p[i:i + l] in t]
        return sorted((i, l) for i, l in occ
                      if not any((i2, l2) != (i, l) and i2 <= i and i2 + l2 >= i + l for i2, l2 in occ))


def mems_by_rule(ms_len, min_len=1):
    """the positions i of one pattern's ms_len with ms_len[i] >= min_len and (i == 0 or ms_len[i - 1] <= ms_len[i])"""
    return [i for i in range(len(ms_len)) if ms_len[i] >= min_len and (i == 0 or ms_len[i - 1] <= ms_len[i])]


def mems(pats, ms, min_len):
    """the MEM arrays of a batch from its matching statistics ms = (ms_len, ms_pos, ms_occ):
    -> (mem_offs uint64 [npat + 1], mem_start uint64, mem_pos uint64, mem_len uint32)"""
    offs, start, pos, ln = [0], [], [], []
    o = 0
    for p in pats:
        m = len(p)
        for i in mems_by_rule(ms[0][o:o + m].tolist(), min_len):
            start.append(i)
            pos.append(int(ms[1][o + i]))
            ln.append(int(ms[0][o + i]))
        offs.append(len(start))
        o += m
    return np.array(offs, np.uint64), np.array(start, np.uint64), np.array(pos, np.uint64), np.array(ln, np.uint32)
