"""CPU reference of the repeat-cover calls (tc_repeat_spans, tc_repeat_mask, tc_repeat_dedup, tc_cover_*_dev; include/textcomp.h has
the definitions), in plain Python and numpy:

  seeds(t, L, q, kind)       the seed positions, from a dictionary of the L-mers: the positions of every L-mer with at least q
                             of them, without the first for COVER_LATER;
  cover_of_len(len, L)       the general form: a boolean cover from any array of lengths, position i counting iff len[i] >= L and
                             covering [i, min(n, i + len[i])) -- a difference array, so it is linear on any contents;
  cover(t, L, q, kind)       the two together (a seed is a length L at its position);
  spans / mask / dedup       from a boolean cover;
  brute_cover(t, L, q, kind) straight from the equivalent definition over ALL substrings of length >= L, for short texts: every
                             occurrence (LATER: but the leftmost) of every substring that occurs at least q times is covered.

tests/test_cover_ref.py holds them together.  No oracle is involved: the reference has no such operation."""
import collections

import numpy as np

ALL, LATER = 0, 1
UPPER = np.arange(256, dtype=np.uint8)
UPPER[ord("a"):ord("z") + 1] -= 32          # the map of the header's examples


def seeds(t, L, q=2, kind=ALL):
    """the seed positions, increasing"""
    t = bytes(t)
    n = len(t)
    if L < 1 or L > n:
        return []
    where = collections.defaultdict(list)
    for i in range(n - L + 1):
        where[t[i:i + L]].append(i)
    out = []
    for pos in where.values():
        if len(pos) >= q:
            out.extend(pos[1:] if kind == LATER else pos)
    return sorted(out)


def cover_of_len(ln, L):
    """the general form -> a boolean array of len(ln) entries"""
    ln = np.asarray(ln).astype(np.int64)
    n = len(ln)
    i = np.nonzero(ln >= L)[0]
    d = np.zeros(n + 1, np.int64)
    np.add.at(d, i, 1)
    np.add.at(d, np.minimum(n, i + ln[i]), -1)
    return np.cumsum(d)[:n] > 0


def cover(t, L, q=2, kind=ALL):
    ln = np.zeros(len(bytes(t)), np.int64)
    ln[seeds(t, L, q, kind)] = L
    return cover_of_len(ln, L)


def spans(cov):
    """-> (start, len) as uint32 arrays, covered"""
    c = np.concatenate(([0], np.asarray(cov, np.int8), [0]))
    d = np.diff(c)
    s, e = np.nonzero(d == 1)[0], np.nonzero(d == -1)[0]
    return s.astype(np.uint32), (e - s).astype(np.uint32), int(np.count_nonzero(cov))


def mask(t, cov, map=None):
    """-> a uint8 array: map[t[p]] where covered, t[p] elsewhere; without a map the cover as 1 / 0"""
    if map is None:
        return np.asarray(cov).astype(np.uint8)
    a = np.frombuffer(bytes(t), np.uint8)
    return np.where(cov, np.asarray(map, np.uint8)[a], a).astype(np.uint8)


def dedup(t, cov):
    return np.frombuffer(bytes(t), np.uint8)[~np.asarray(cov, bool)].tobytes()


def brute_cover(t, L, q=2, kind=ALL):
    """every substring of length >= L is counted with all its (overlapping) occurrences"""
    t = bytes(t)
    n = len(t)
    cov = np.zeros(n, bool)
    where = collections.defaultdict(list)
    for l in range(max(L, 1), n + 1):
        for i in range(n - l + 1):
            where[t[i:i + l]].append(i)
    for w, pos in where.items():
        if len(pos) >= q:
            for i in (pos[1:] if kind == LATER else pos):
                cov[i:i + len(w)] = True
    return cov


def reference(t, L, q=2, kind=ALL, map=None):
    """-> (start, len), covered, mask, dedup"""
    cov = cover(t, L, q, kind)
    s, l, c = spans(cov)
    return (s, l), c, mask(t, cov, map), dedup(t, cov)
