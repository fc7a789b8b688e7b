"""CPU reference of the maximal and supermaximal repeats of a text (tc_repeats; include/textcomp.h has the definitions),
written twice:

  brute(t, ...)    straight from the definitions, for short texts: every substring that occurs twice, its occurrences, its
                   left and right extensions; supermaximal = a maximal repeat that is a substring of no other;
  repeats(t, ...)  the suffix-array rule: a naive sort and Kasai's loop (tests/lz_ref.py), one stack walk over the LCP
                   array that closes every LCP interval [lb, rb] of length l, the left contexts compared directly, every
                   interval keyed by its representative row (the smallest j in (lb, rb] with lcp[j] = l) and listed in
                   increasing j.

tests/test_rep_ref.py holds the two together.  No oracle is involved: the reference has no such operation."""
import numpy as np

import lz_ref

MAXIMAL, SUPERMAXIMAL = 0, 1
NOTHING = -1        # left of the suffix that starts the text


def esa(t):
    """-> (sa, lcp, left) as int64 arrays of n + 1 rows"""
    t = bytes(t)
    sa = lz_ref.suffix_array(t)
    lcp = np.array(lz_ref.lcp_array(t, sa), np.int64)
    tb = np.frombuffer(t, np.uint8).astype(np.int64)
    left = np.where(sa > 0, tb[np.maximum(sa, 1) - 1] if len(t) else 0, NOTHING)
    return sa, lcp, left


def intervals(lcp):
    """every LCP interval (l, lb, rb) with l >= 1 and lb < rb, by the stack walk (in the order the walk closes them)"""
    N = len(lcp)
    out, stack = [], [(0, 0)]           # (l, lb)
    vals = lcp.tolist() + [0]
    for r in range(1, N + 1):
        lb = r - 1
        while stack[-1][0] > vals[r]:
            l, lb = stack.pop()
            out.append((l, lb, r - 1))
        if stack[-1][0] < vals[r]:
            stack.append((vals[r], lb))
    return out


def repeats(t, kind=MAXIMAL, min_len=1, min_occ=2):
    """-> (pos, len, occ, row, sa) as uint32 arrays, in the order tc_repeats writes them"""
    t = bytes(t)
    sa, lcp, left = esa(t)
    found = []
    for l, lb, rb in intervals(lcp):
        occ = rb - lb + 1
        if l < min_len or occ < min_occ:
            continue
        ctx = left[lb:rb + 1]
        if kind == MAXIMAL:
            if not (ctx != ctx[0]).any():
                continue
        else:
            if (lcp[lb + 1:rb + 1] != l).any() or len(np.unique(ctx)) != occ:
                continue
        j = lb + 1 + int(np.argmax(lcp[lb + 1:rb + 1] == l))
        found.append((j, int(sa[lb]), l, occ, lb))
    found.sort()
    cols = [np.array([f[k] for f in found], np.uint32) for k in (1, 2, 3, 4)]
    return cols[0], cols[1], cols[2], cols[3], sa.astype(np.uint32)


def as_dict(t, pos, ln, occ, row, sa):
    """{repeat string: sorted occurrences}; asserts that no string is listed twice and that pos = sa[row]"""
    t = bytes(t)
    d = {}
    for p, l, o, r in zip(pos.tolist(), ln.tolist(), occ.tolist(), row.tolist()):
        w = t[p:p + l]
        assert len(w) == l and w not in d and int(sa[r]) == p
        d[w] = sorted(int(x) for x in sa[r:r + o])
    return d


def brute(t, kind=MAXIMAL, min_len=1, min_occ=2):
    """{repeat string: sorted occurrences}, from the definitions"""
    t = bytes(t)
    n = len(t)
    occs = {}
    for i in range(n):
        for l in range(1, n - i + 1):
            occs.setdefault(t[i:i + l], []).append(i)
    maximal = {}
    for w, ps in occs.items():
        if len(ps) < 2:
            continue
        l = len(w)
        right = [t[p + l] if p + l < n else ("end", p) for p in ps]     # the end differs from everything
        lft = [t[p - 1] if p else ("start", p) for p in ps]
        if len(set(right)) > 1 and len(set(lft)) > 1:
            maximal[w] = ps
    if kind == SUPERMAXIMAL:
        maximal = {w: ps for w, ps in maximal.items() if not any(w != v and w in v for v in maximal)}
    return {w: ps for w, ps in maximal.items() if len(w) >= min_len and len(ps) >= min_occ}


# ---- the texts of the tests
fibonacci, periodic, random_text = lz_ref.fibonacci, lz_ref.periodic, lz_ref.random_text


def many_left(doubled=None):
    """w = 01 02 03; w, then (c, w) for c = 0 .. 255: w occurs 257 times, all left contexts distinct (Nothing among them)
    and all right contexts distinct.  doubled = c: the byte in front of the last w is c instead of 255, so one left
    context occurs twice."""
    w = bytes([1, 2, 3])
    heads = list(range(256))
    if doubled is not None:
        heads[255] = doubled
    return w + b"".join(bytes([c]) + w for c in heads)
