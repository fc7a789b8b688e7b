"""Brute-force reference for the search with mismatches (tc_fm_count_mm / tc_fm_locate_mm): slide the pattern over the
text, count the differing bytes of every window, keep the windows within distance k.  numpy only; it shares nothing with
the code under test.  Exact for any text and pattern; cheap for the sizes the tests use (texts <= 8192 bytes, patterns
<= 32 bytes)."""
import numpy as np


def hits(text, pat, k):
    """-> (positions, distances): the 1-based positions i + 1, 0 <= i <= n - m, with Hamming(text[i : i + m], pat) <= k, in
    ascending order, and their distances.  An empty pattern or one longer than the text has none."""
    t = np.frombuffer(bytes(text), np.uint8)
    p = np.frombuffer(bytes(pat), np.uint8)
    n, m = len(t), len(p)
    if m == 0 or m > n:
        return np.empty(0, np.uint64), np.empty(0, np.uint8)
    dist = np.zeros(n - m + 1, np.int64)
    for j in range(m):
        dist += t[j:n - m + 1 + j] != p[j]
    pos = np.nonzero(dist <= k)[0]
    return (pos + 1).astype(np.uint64), dist[pos].astype(np.uint8)


def count(text, pat, k):
    return len(hits(text, pat, k)[0])


def sorted_pairs(positions, distances):
    """a device answer (enumeration order) in the reference's order: sorted by position"""
    positions = np.asarray(positions, np.uint64)
    distances = np.asarray(distances, np.uint8)
    o = np.argsort(positions, kind="stable")
    return positions[o], distances[o]
