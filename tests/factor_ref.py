"""Brute-force reference of FM-index factorize / unfactorize (numpy and Python bytes only; shares nothing with the code
under test).

The parse of a pattern p against a text t runs right to left and is greedy: with j = len(p), while j > 0, l is the largest
value such that p[j - l : j] occurs in t.  l >= 1 gives the match factor (pos, l), pos the 1-based position of the
occurrence whose text suffix is lexicographically smallest, the end of the text sorting first -- Python's bytes order puts
a proper prefix first, which is exactly that; l = 0 gives the literal factor (p[j - 1], 0).  Factors are listed in pattern
order, left to right."""
import numpy as np


def suffix_ranks(t):
    """rank[i] = the position of the suffix t[i:] among all suffixes of t, the empty one included (rank 0)"""
    t = bytes(t)
    n = len(t)
    rank = [0] * (n + 1)
    for r, i in enumerate(sorted(range(n + 1), key=lambda i: t[i:])):
        rank[i] = r
    return rank


def occurrences(t, w):
    out, i = [], t.find(w)
    while i >= 0:
        out.append(i)
        i = t.find(w, i + 1)
    return out


def factorize_one(t, rank, p):
    """[(pos, len)] of one pattern"""
    t, p = bytes(t), bytes(p)
    out = []
    j = len(p)
    while j > 0:
        l = 0
        while l < j and p[j - l - 1:j] in t:
            l += 1
        if l == 0:
            out.append((p[j - 1], 0))
            j -= 1
        else:
            i = min(occurrences(t, p[j - l:j]), key=lambda i: rank[i])
            out.append((i + 1, l))
            j -= l
    return out[::-1]


def factorize(t, pats, rank=None):
    """-> (fac_offs uint64 [npat + 1], fac_pos uint64 [total], fac_len uint32 [total])"""
    rank = suffix_ranks(t) if rank is None else rank
    offs, pos, ln = [0], [], []
    for p in pats:
        for a, l in factorize_one(t, rank, p):
            pos.append(a)
            ln.append(l)
        offs.append(len(pos))
    return np.array(offs, np.uint64), np.array(pos, np.uint64), np.array(ln, np.uint32)


def unfactorize(t, fac_offs, fac_pos, fac_len):
    """-> list of bytes, one per pattern"""
    t = bytes(t)
    out = []
    for i in range(len(fac_offs) - 1):
        b = b""
        for f in range(int(fac_offs[i]), int(fac_offs[i + 1])):
            a, l = int(fac_pos[f]), int(fac_len[f])
            b += bytes([a]) if l == 0 else t[a - 1:a - 1 + l]
        out.append(b)
    return out
