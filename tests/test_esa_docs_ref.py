"""CPU-only: the numpy reference of the document queries (tests/esa_docs_ref.py) is held to loops over the bytes -- da and pv, the
count with and without a limit, the list with its order and its hit positions -- on every text over {a, b} of up to 7 bytes with every
split into at most 3 documents, on random, Fibonacci, periodic and unary texts of up to 200 bytes with 1, 2, 7 and n documents, and on
the worked example of include/textcomp.h, banana . bandana . ananas, whose values are pinned literally."""
import itertools

import numpy as np
import pytest

import esa_docs_ref as R
import esa_ref


def _check_text(t, ds, queries):
    ref = R.DocRef(t, ds)
    da, pv = R.brute_arrays(t, list(ds))
    assert ref.da.tolist() == da and ref.pv.tolist() == pv
    for k in (1, 2, 3, 5):
        want = R.brute_kmer_docs(t, list(ds), k)
        got = ref.kmer_docs(k)
        assert [tuple(int(x[i]) for x in got) for i in range(len(got[0]))] == want, (t, list(ds), k)
        hist, distinct = ref.kmer_doc_spectrum(k)
        assert distinct == len(want) and hist.sum() == distinct and len(hist) == ref.ndocs + 1
        assert hist.tolist() == [sum(1 for w in want if w[2] == d) for d in range(ref.ndocs + 1)]
        for lo, hi in ((1, 1), (2, 0), (ref.ndocs, 0), (2, 3)):
            got = ref.kmer_docs(k, lo, hi)
            assert [int(x) for x in got[3]] == [w[3] for w in want if w[2] >= lo and (hi == 0 or w[2] <= hi)]
    s = [q[0] for q in queries]
    l = [q[1] for q in queries]
    for limit in (0, 1, 2):
        df, occ = ref.count(s, l, limit)
        offs, docs, hits = ref.list(s, l, limit)
        assert offs[0] == 0 and np.array_equal(np.diff(offs.astype(np.int64)), df)
        for k, (a, b) in enumerate(queries):
            wd, wh, wo = R.brute_list(t, list(ds), a, b, limit)
            assert (int(df[k]), int(occ[k])) == (len(wd), wo if b else len(t) + 1), (t, list(ds), a, b, limit)
            assert docs[int(offs[k]):int(offs[k + 1])].tolist() == wd and hits[int(offs[k]):int(offs[k + 1])].tolist() == wh


def _all_substrings(n):
    return [(s, l) for s in range(n + 1) for l in range(n - s + 1)]


@pytest.mark.parametrize("n", range(8))
def test_every_short_text_with_every_split(n):
    """every text over {a, b} of n bytes, every split into 1, 2 and 3 documents (empty ones included), every substring"""
    for t in itertools.product(b"ab", repeat=n):
        t = bytes(t)
        splits = {(0, n)} | {(0, a, n) for a in range(n + 1)} | {(0, a, b, n) for a in range(n + 1) for b in range(a, n + 1)}
        for ds in sorted(splits):
            _check_text(t, ds, _all_substrings(n))


def _texts():
    rng = np.random.default_rng(0xD0C5)
    yield "random2", bytes(rng.integers(97, 99, 200).astype(np.uint8))
    yield "random4", bytes(rng.integers(97, 101, 150).astype(np.uint8))
    yield "fibonacci", esa_ref.fibonacci(144)
    yield "period3", (b"abc" * 40)[:100]
    yield "period7", (b"abcabca" * 20)[:90]
    yield "unary", b"a" * 60


@pytest.mark.parametrize("name,t", list(_texts()), ids=[x[0] for x in _texts()])
def test_longer_texts(name, t):
    n = len(t)
    rng = np.random.default_rng(n)
    for ndocs in (1, 2, 7, n):
        ds = R.split_evenly(n, ndocs)
        if ndocs == 7:                                  # empty documents first, last and adjacent
            ds = np.array([0, 0, n // 5, n // 5, n // 5, n // 2, n, n])
        q = [(int(s), int(min(l, n - s))) for s, l in zip(rng.integers(0, n + 1, 60), rng.integers(0, 9, 60))]
        q += [(0, 0), (n, 0), (0, n), (n - 1, 1), (0, 1)]
        _check_text(t, ds, q)


def test_the_headers_example_pinned():
    t, ds = R.concat([b"banana", b"bandana", b"ananas"])
    assert t == b"bananabandanaananas" and ds.tolist() == [0, 6, 13, 19]
    ref = R.DocRef(t, ds)
    row, occ, _ = ref.find([1], [3])
    assert (int(row[0]), int(occ[0])) == (3, 5)                                     # "ana": rows [3, 8)
    offs, docs, hits = ref.list([1, 0, 2, 9, 3, 0], [3, 3, 3, 1, 4, 0])
    got = [docs[int(a):int(b)].tolist() for a, b in zip(offs[:-1], offs[1:])]
    assert got == [[1, 0, 2], [0, 1], [0, 2], [1], [0], [1, 0, 2]]
    assert hits[:3].tolist() == [10, 3, 13] and [t[h:h + 3] for h in (10, 3, 13)] == [b"ana"] * 3     # (text[7 : 10] is "and")
    df, occ = ref.count([1, 0, 2, 9, 3, 0], [3, 3, 3, 1, 4, 0])
    assert df.tolist() == [3, 2, 2, 1, 1, 3] and occ.tolist()[:5] == [5, 2, 2, 1, 1]
    assert ref.count([1, 0, 9], [3, 3, 1], limit=2)[0].tolist() == [2, 2, 1]
    assert ref.count([1, 0, 9], [3, 3, 1], limit=1)[0].tolist() == [1, 1, 1]
    assert int(ref.da[0]) == R.NO_DOC and int(ref.pv[0]) == R.NO_DOC
    pos, occ, df, row = ref.kmer_docs(3)
    assert len(pos) == 11 and sorted(df.tolist()) == [1] * 8 + [2, 2, 3]
    assert sorted(t[p:p + 3] for p, d in zip(pos.tolist(), df.tolist()) if d == 2) == [b"ban", b"nan"]
    assert [(t[p:p + 3], o) for p, o, d in zip(pos.tolist(), occ.tolist(), df.tolist()) if d == 3] == [(b"ana", 5)]
    hist, distinct = ref.kmer_doc_spectrum(3)
    assert hist.tolist() == [0, 8, 2, 1] and distinct == 11
