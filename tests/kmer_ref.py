"""CPU reference of the k-mers of a text (tc_kmers, tc_kmer_spectrum, tc_kmer_profile; include/textcomp.h has the
definitions), written twice:

  by_counter(t, k, ...)     collections.Counter over all substrings of length k, sorted: no suffix array is involved;
  by_esa(sa, lcp, k, ...)   the boundary definition applied to a suffix array and an LCP array -- those of a text (esa(t),
                            built naively) or any two arrays of N entries, which is what the _esa_dev entries promise to
                            follow on arrays that no text has.

tests/test_kmer_ref.py holds the two together.  No oracle is involved: the reference has no such operation."""
import collections

import numpy as np

import lz_ref

MASK64 = (1 << 64) - 1


def counter(t, k):
    t = bytes(t)
    return collections.Counter(t[i:i + k] for i in range(len(t) - k + 1)) if 1 <= k <= len(t) else collections.Counter()


def keep(occ, min_occ=1, max_occ=0):
    return occ >= min_occ and (max_occ == 0 or occ <= max_occ)


def by_counter(t, k, min_occ=1, max_occ=0):
    """[(k-mer, occ)] in lexicographic order, after the filters"""
    return [(w, c) for w, c in sorted(counter(t, k).items()) if keep(c, min_occ, max_occ)]


def esa(t):
    """-> (sa, lcp) as int64 arrays of n + 1 rows, naively"""
    t = bytes(t)
    sa = lz_ref.suffix_array(t)
    return sa, np.array(lz_ref.lcp_array(t, sa), np.int64)


def by_esa(sa, lcp, k, min_occ=1, max_occ=0):
    """-> (row, pos, occ) as lists: row q is a boundary iff lcp[q] < k (lcp[0] counts as 0, row N is one too); a k-mer is
    the interval [p, q) between two consecutive boundaries with sa[p] + k <= n"""
    N = len(lcp)
    n = N - 1
    bounds = [q for q in range(N) if q == 0 or int(lcp[q]) < k] + [N]
    out = ([], [], [])
    for p, q in zip(bounds, bounds[1:]):
        if int(sa[p]) + k <= n and keep(q - p, min_occ, max_occ):
            for col, v in zip(out, (p, int(sa[p]), q - p)):
                col.append(v)
    return out


def spectrum_of(occs, bins):
    """hist of `bins` entries from the k-mers' occurrence counts"""
    h = [0] * bins
    for c in occs:
        h[min(c, bins) - 1] += 1
    return h


def spectrum(t, k, bins):
    """-> (hist, distinct, total) from the Counter"""
    c = counter(t, k)
    return spectrum_of(c.values(), bins), len(c), max(0, len(bytes(t)) - k + 1)


def profile(t, kmax):
    """-> (distinct, unique), lists of kmax entries, from the Counter"""
    cs = [counter(t, k) for k in range(1, kmax + 1)]
    return [len(c) for c in cs], [sum(1 for v in c.values() if v == 1) for c in cs]


def profile_by_lcp(lcp, kmax):
    """the two formulas of the header on an LCP array (any N words), modulo 2^64 as the library computes them:
    distinct(k) = max(0, n-k+1) - #{r : lcp[r] >= k}, unique(k) = #{r in 1 .. n : max(lcp[r], lcp[r+1]) < k} - min(k-1, n)"""
    l = np.array(lcp, np.int64).copy()
    N = len(l)
    n = N - 1
    l[0] = 0
    nxt = np.concatenate([l[1:], [0]])
    m = np.maximum(l, nxt)[1:]
    d, u = [], []
    for k in range(1, kmax + 1):
        d.append((max(0, n - k + 1) - int((l >= k).sum())) & MASK64)
        u.append((int((m < k).sum()) - min(k - 1, n)) & MASK64)
    return d, u


# ---- the texts of the tests
fibonacci, periodic, random_text = lz_ref.fibonacci, lz_ref.periodic, lz_ref.random_text

# (text, k, [(row, pos, occ)]): the worked examples of include/textcomp.h
EXAMPLES = [
    (b"mississippi", 2, [(2, 7, 1), (3, 4, 2), (5, 0, 1), (6, 9, 1), (7, 8, 1), (8, 6, 2), (10, 5, 2)]),
    (b"aaabaab", 2, [(1, 0, 3), (4, 5, 2), (7, 3, 1)]),
    (b"aaabaab", 1, [(1, 0, 5), (6, 6, 2)]),
    (b"aaaaaa", 2, [(2, 4, 5)]),
]
EXAMPLE_ESA = {
    b"mississippi": ([11, 10, 7, 4, 1, 0, 9, 8, 6, 3, 5, 2], [0, 0, 1, 1, 4, 0, 0, 1, 0, 2, 1, 3]),
    b"aaabaab": ([7, 0, 4, 1, 5, 2, 6, 3], [0, 0, 2, 3, 1, 2, 0, 1]),
}
