"""CPU reference of the cross-document matches on a kept enhanced suffix array (tc_esa_doc_match, tc_esa_doc_shared;
include/textcomp.h has the definitions), in numpy, on top of tests/esa_docs_ref.py -- the row formulation:

  XRef(t, doc_start).neighbours(kind)  -> (a, b): for every row r >= 1 the nearest row >= 1 above and below whose document
                                       qualifies (OTHER: another document, from the run heads of da by two accumulates; EARLIER: a
                                       smaller document, by a stack over the rows), 0 and N where there is none;
  XRef.match(kind, clamp)              -> (xl, src, xdoc) in text order: La = min lcp(a, r], Lb = min lcp(r, b], the better of the
                                       two (a on a tie), NO_POS / NO_DOC where the match is empty, the clamp on i's own side;
  XRef.shared(kind, min_len)           -> (shared, longest): the cover of the clamped xl by tests/cover_ref.py summed per document,
                                       and the per-document maximum;
  XRef.cover(kind, min_len)            the boolean cover of the clamped xl.

tests/test_doc_match_ref.py holds all of it to loops over the bytes (brute_* below).  No oracle is involved: the reference has no
such operation."""
import numpy as np

import cover_ref
import esa_docs_ref

OTHER, EARLIER = 0, 1
NO_POS = 0xffffffff
NO_DOC = esa_docs_ref.NO_DOC


class XRef(esa_docs_ref.DocRef):
    def neighbours(self, kind):
        N, da = self.N, self.da
        rows = np.arange(N, dtype=np.int64)
        if kind == OTHER:
            bnd = np.zeros(N, bool)
            bnd[1:] = da[1:] != da[:-1]
            head = np.maximum.accumulate(np.where(bnd, rows, 0))
            a = np.maximum(head - 1, 0)
            nxt = np.where(bnd, rows, N)
            b = np.full(N, N, np.int64)
            b[:-1] = np.minimum.accumulate(nxt[::-1])[::-1][1:]
            return a, b
        a, b = np.zeros(N, np.int64), np.full(N, N, np.int64)
        dal = da.tolist()
        for out, order, none in ((a, range(1, N), 0), (b, range(N - 1, 0, -1), N)):
            stack = []                                  # rows with increasing documents
            for r in order:
                while stack and dal[stack[-1]] >= dal[r]:
                    stack.pop()
                out[r] = stack[-1] if stack else none
                stack.append(r)
        return a, b

    def match(self, kind=OTHER, clamp=True):
        n, N = self.n, self.N
        xl, src, xdoc = np.zeros(n, np.int64), np.full(n, NO_POS, np.int64), np.full(n, NO_DOC, np.int64)
        if n == 0:
            return xl, src, xdoc
        a, b = self.neighbours(kind)
        r = np.arange(1, N, dtype=np.int64)
        a, b = a[1:], b[1:]
        la = np.where(a > 0, self._lcp.query(np.minimum(a + 1, r), r), -1)
        lb = np.where(b < N, self._lcp.query(np.minimum(r + 1, N - 1), np.minimum(b, N - 1)), -1)
        L = np.maximum(la, lb)
        p = np.where(la >= lb, a, np.minimum(b, N - 1))
        i = self.sa[r]
        hit = L > 0
        xl[i[hit]] = L[hit]
        src[i[hit]] = self.sa[p[hit]]
        xdoc[i[hit]] = self.da[p[hit]]
        if clamp:
            xl = np.minimum(xl, self.doc_end() - np.arange(n))
        return xl, src, xdoc

    def doc_end(self):
        """doc_start[d(i) + 1] of every position i"""
        return self.doc_start[np.searchsorted(self.doc_start[1:], np.arange(self.n), side="right") + 1]

    def cover(self, kind, min_len):
        return cover_ref.cover_of_len(self.match(kind, True)[0], min_len)

    def shared(self, kind=OTHER, min_len=1):
        xl = self.match(kind, True)[0]
        c = np.concatenate(([0], np.cumsum(cover_ref.cover_of_len(xl, min_len))))
        ds = self.doc_start
        longest = np.array([xl[ds[d]:ds[d + 1]].max() if ds[d] < ds[d + 1] else 0 for d in range(self.ndocs)], np.uint32)
        return (c[ds[1:]] - c[ds[:-1]]).astype(np.uint64), longest


# ---- straight from the definitions, by loops over the bytes: what tests/test_doc_match_ref.py holds the above to
def _common(t, i, j):
    k = 0
    while i + k < len(t) and j + k < len(t) and t[i + k] == t[j + k]:
        k += 1
    return k


def brute_match(t, doc_start, kind, clamp):
    """(xl, src, xdoc) as lists: sort the suffixes, walk to the nearest qualifying neighbour on each side, compare byte by byte"""
    t = bytes(t)
    n = len(t)
    sufs = esa_docs_ref._sorted_suffixes(t)
    doc = [esa_docs_ref.brute_doc_of(doc_start, i) for i in range(n)]
    xl, src, xdoc = [0] * n, [NO_POS] * n, [NO_DOC] * n
    for r, i in enumerate(sufs):
        if i == n:
            continue
        ok = (lambda j: doc[j] != doc[i]) if kind == OTHER else (lambda j: doc[j] < doc[i])
        best, partner = -1, None
        for step in (-1, 1):                            # the predecessor first: it wins a tie
            x = r + step
            while 0 <= x < len(sufs) and (sufs[x] == n or not ok(sufs[x])):
                x += step
            if 0 <= x < len(sufs):
                l = _common(t, i, sufs[x])
                if l > best:
                    best, partner = l, sufs[x]
        if best > 0:
            xl[i], src[i], xdoc[i] = best, partner, doc[partner]
            if clamp:
                xl[i] = min(best, doc_start[doc[i] + 1] - i)
    return xl, src, xdoc


def brute_shared(t, doc_start, kind, min_len):
    """(shared, longest) as lists, from brute_match's clamped xl by a loop over the bytes of every document"""
    xl = brute_match(t, doc_start, kind, True)[0]
    shared, longest = [], []
    for d in range(len(doc_start) - 1):
        s, e = int(doc_start[d]), int(doc_start[d + 1])
        shared.append(sum(1 for p in range(s, e) if any(xl[i] >= min_len and p < i + xl[i] for i in range(s, p + 1))))
        longest.append(max(xl[s:e], default=0))
    return shared, longest
