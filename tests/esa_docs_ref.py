"""CPU reference of the document queries on a kept enhanced suffix array (tc_esa_build_docs, tc_esa_doc_count, tc_esa_doc_list;
include/textcomp.h has the definitions), in numpy, on top of tests/esa_ref.py:

  DocRef(t, doc_start).da, .pv        the document of every row and the previous row of that document (+ 1; 0: none), as the handle
                                      keeps them: da by a searchsorted of sa in doc_start, pv from a stable sort of the rows by da;
  DocRef.count(start, length, limit)  -> (df, occ): the rows x of the substring's interval [lo, hi) with pv[x] <= lo, one per
                                      distinct document, counted and cut at limit;
  DocRef.list(start, length, limit)   -> (list_offs, docs, hit_pos): those rows in increasing order, da and sa of each;
  DocRef.kmer_docs(k, min_df, max_df) -> (pos, occ, df, row): the k-mers of tc_kmers_esa_dev with df = the flagged rows of each group,
                                      a row being flagged when pv[r] <= the head of its group, by one cumulative sum;
  DocRef.kmer_doc_spectrum(k)         -> (hist of ndocs + 1 bins, distinct).

An occurrence belongs to the document that holds its first byte.  tests/test_esa_docs_ref.py holds all of it to loops over the bytes
(brute_* below).  No oracle is involved: the reference has no such operation."""
import functools

import numpy as np

import esa_ref

NO_DOC = 0xffffffff


def concat(docs):
    """a list of bytes -> (text, doc_start)"""
    ds = np.zeros(len(docs) + 1, np.int64)
    ds[1:] = np.cumsum([len(d) for d in docs])
    return b"".join(bytes(d) for d in docs), ds


def split_evenly(n, ndocs):
    """doc_start of ndocs documents of (almost) equal size over n bytes (empty ones where ndocs > n)"""
    return (np.arange(ndocs + 1, dtype=np.int64) * n) // ndocs


class DocRef(esa_ref.Ref):
    def __init__(self, t, doc_start):
        super().__init__(t)
        ds = np.asarray(doc_start, np.int64)
        assert len(ds) >= 2 and ds[0] == 0 and ds[-1] == self.n and (np.diff(ds) >= 0).all()
        self.doc_start = ds
        self.ndocs = len(ds) - 1
        # the d with ds[d] <= p < ds[d + 1]: the number of boundaries ds[1 ..] at or below p
        self.da = np.searchsorted(ds[1:], self.sa, side="right")
        self.da[self.sa >= self.n] = NO_DOC
        order = np.argsort(self.da, kind="stable")          # the rows in (document, row) order; NO_DOC (row 0) last
        self.pv = np.zeros(self.N, np.int64)
        same = self.da[order[1:]] == self.da[order[:-1]]
        self.pv[order[1:][same]] = order[:-1][same] + 1
        self.pv[self.da == NO_DOC] = NO_DOC
        self._whole = np.nonzero(self.pv[1:] <= 1)[0] + 1       # the answer of the empty string: every document's first row

    def _interval(self, start, length):
        lo, occ, _ = self.find(start, length)
        lo, occ = lo.astype(np.int64), occ.astype(np.int64)
        hi = lo + occ
        lo[np.asarray(length, np.int64) == 0] = 1           # the empty string: every row but the empty suffix
        return lo, hi, occ

    def _firsts(self, lo, hi, limit):
        if lo == 1 and hi == self.N:
            rows = self._whole
        else:
            rows = np.nonzero(self.pv[lo:hi] <= lo)[0] + lo
        return rows[:limit] if limit else rows

    def count(self, start, length, limit=0):
        lo, hi, occ = self._interval(start, length)
        df = np.array([len(self._firsts(a, b, limit)) for a, b in zip(lo.tolist(), hi.tolist())], np.uint32)
        return df.reshape(-1), occ.astype(np.uint32)

    def list(self, start, length, limit=0):
        lo, hi, _ = self._interval(start, length)
        firsts = [self._firsts(a, b, limit) for a, b in zip(lo.tolist(), hi.tolist())]
        offs = np.zeros(len(firsts) + 1, np.uint64)
        offs[1:] = np.cumsum([len(f) for f in firsts])
        rows = np.concatenate(firsts) if firsts else np.zeros(0, np.int64)
        rows = rows.astype(np.int64)
        return offs, self.da[rows].astype(np.uint32), self.sa[rows].astype(np.uint32)


    def kmer_docs(self, k, min_df=1, max_df=0):
        b = self.lcp < k
        b[0] = True
        p = np.nonzero(b)[0]                                # the heads: every boundary row
        q = np.append(p[1:], self.N)
        head = p[np.cumsum(b) - 1]
        flag = (self.pv <= head) & (np.arange(self.N) >= 1)
        F = np.concatenate(([0], np.cumsum(flag)))
        df = F[q] - F[p]
        keep = (self.sa[p] + k <= self.n) & (df >= min_df) & ((max_df == 0) | (df <= max_df))
        return tuple(x[keep].astype(np.uint32) for x in (self.sa[p], q - p, df, p))

    def kmer_doc_spectrum(self, k):
        df = self.kmer_docs(k)[2]
        return np.bincount(df.astype(np.int64), minlength=self.ndocs + 1).astype(np.uint64), len(df)


# ---- straight from the definitions, by loops over the bytes: what tests/test_esa_docs_ref.py holds the above to
def brute_kmer_docs(t, doc_start, k):
    """[(pos, occ, df, row)] of every distinct k-mer in lexicographic order: pos and row those of its first sorted suffix"""
    n = len(t)
    sufs = _sorted_suffixes(bytes(t))
    out, seen = [], {}
    for r, i in enumerate(sufs):
        if i + k > n:
            continue
        w = t[i:i + k]
        if w not in seen:
            seen[w] = len(out)
            out.append([i, 0, set(), r])
        out[seen[w]][1] += 1
        out[seen[w]][2].add(brute_doc_of(doc_start, i))
    return [(a, b, len(c), d) for a, b, c, d in out]


@functools.lru_cache(maxsize=64)
def _sorted_suffixes(t):
    """the suffixes of t in sorted order, the empty one first, by comparing them as byte strings (kept: one text is asked many times)"""
    return sorted(range(len(t) + 1), key=lambda i: t[i:])


def brute_doc_of(doc_start, p):
    for d in range(len(doc_start) - 1):
        if doc_start[d] <= p < doc_start[d + 1]:
            return d
    return NO_DOC


def brute_arrays(t, doc_start):
    """(da, pv) over the sorted suffixes, the empty one first"""
    sufs = _sorted_suffixes(bytes(t))
    da = [brute_doc_of(doc_start, i) for i in sufs]
    pv = []
    for r in range(len(sufs)):
        if da[r] == NO_DOC:
            pv.append(NO_DOC)
            continue
        before = [x for x in range(r) if da[x] == da[r]]
        pv.append(before[-1] + 1 if before else 0)
    return da, pv


def brute_list(t, doc_start, s, l, limit=0):
    """(docs, hit_pos, occ): the documents of the occurrences of t[s : s + l] in the order of their first row among the sorted
    suffixes, one occurrence (that row's suffix) in each, and the number of occurrences as tc_esa_find counts them"""
    n = len(t)
    w = t[s:s + l]
    sufs = _sorted_suffixes(bytes(t))
    docs, hits, occ = [], [], 0
    for i in sufs:
        if i + l > n or t[i:i + l] != w:
            continue
        occ += 1
        d = brute_doc_of(doc_start, i)
        if d != NO_DOC and d not in docs and (not limit or len(docs) < limit):
            docs.append(d)
            hits.append(i)
    return docs, hits, occ
