"""CPU-only: the numpy reference of the cross-document matches (tests/doc_match_ref.py) is held to loops over the bytes -- sort the
suffixes, walk to the nearest qualifying neighbour, compare byte by byte -- on every text over {a, b} of up to 7 bytes with every split
into at most 3 documents, on random, Fibonacci, period-7 and unary texts of up to 200 bytes in 1, 2, 7 and n documents, both kinds, both
clamps; the unclamped lengths are held to the document counts and lists of tests/esa_docs_ref.py (xl[i] >= L iff the substring (i, L)
occurs in two documents / in an earlier one); and the four worked examples of include/textcomp.h are pinned literally."""
import itertools

import numpy as np
import pytest

import cover_ref
import doc_match_ref as X
import esa_ref

KINDS = (X.OTHER, X.EARLIER)


def _check(t, ds, min_lens=(1, 2, 3)):
    ref = X.XRef(t, ds)
    for kind in KINDS:
        for clamp in (False, True):
            got = ref.match(kind, clamp)
            want = X.brute_match(t, list(ds), kind, clamp)
            assert [g.tolist() for g in got] == [list(w) for w in want], (t, list(ds), kind, clamp)
        for L in min_lens:
            shared, longest = ref.shared(kind, L)
            ws, wl = X.brute_shared(t, list(ds), kind, L)
            assert shared.tolist() == ws and longest.tolist() == wl, (t, list(ds), kind, L)
    return ref


def _check_property(ref):
    """with clamp = 0: OTHER xl[i] >= L iff doc_count(i, L, limit 2) = 2; EARLIER iff the document list of (i, L) holds one below d(i)"""
    n = ref.n
    pairs = [(i, L) for i in range(n) for L in range(1, n - i + 1)]
    if not pairs:
        return 0
    s, l = [p[0] for p in pairs], [p[1] for p in pairs]
    xo, xe = ref.match(X.OTHER, False)[0], ref.match(X.EARLIER, False)[0]
    df, _ = ref.count(s, l, 2)
    offs, docs, _ = ref.list(s, l, 0)
    doc_of = np.searchsorted(ref.doc_start[1:], np.arange(n), side="right")
    for k, (i, L) in enumerate(pairs):
        assert (xo[i] >= L) == (df[k] == 2), (ref.t, ref.doc_start.tolist(), i, L)
        earlier = bool((docs[int(offs[k]):int(offs[k + 1])].astype(np.int64) < doc_of[i]).any())
        assert (xe[i] >= L) == earlier, (ref.t, ref.doc_start.tolist(), i, L)
    return len(pairs)


@pytest.mark.parametrize("n", range(8))
def test_every_short_text_with_every_split(n):
    for t in itertools.product(b"ab", repeat=n):
        t = bytes(t)
        splits = {(0, n)} | {(0, a, n) for a in range(n + 1)} | {(0, a, b, n) for a in range(n + 1) for b in range(a, n + 1)}
        for ds in sorted(splits):
            _check(t, ds)


def _texts():
    rng = np.random.default_rng(0xD0C6)
    yield "random2", bytes(rng.integers(97, 99, 200).astype(np.uint8))
    yield "random4", bytes(rng.integers(97, 101, 150).astype(np.uint8))
    yield "fibonacci", esa_ref.fibonacci(144)
    yield "period7", (b"abcabca" * 20)[:90]
    yield "unary", b"a" * 60


@pytest.mark.parametrize("name,t", list(_texts()), ids=[x[0] for x in _texts()])
def test_longer_texts(name, t):
    n = len(t)
    for ndocs in (1, 2, 7, n):
        ds = X.esa_docs_ref.split_evenly(n, ndocs)
        if ndocs == 7:                                  # empty documents first, last and adjacent
            ds = np.array([0, 0, n // 5, n // 5, n // 5, n // 2, n, n])
        ref = _check(t, ds, (1, 2, 3, 20))
        if ndocs == 1:
            assert not ref.match(X.OTHER, True)[0].any() and not ref.shared(X.EARLIER, 1)[0].any()


def test_the_property_against_the_document_counts_and_lists():
    rng = np.random.default_rng(0xD0C7)
    pairs = 0
    for _ in range(60):
        n = int(rng.integers(1, 26))
        t = bytes(rng.integers(97, 99, n).astype(np.uint8))
        ndocs = int(rng.integers(1, 6))
        ds = np.concatenate(([0], np.sort(rng.integers(0, n + 1, ndocs - 1)), [n])).astype(np.int64)
        pairs += _check_property(X.XRef(t, ds))
    assert pairs > 5000


def _row(s):
    return [X.NO_POS if x == "-" else int(x) for x in s.split()]


def test_the_headers_examples_pinned():
    t, ds = X.esa_docs_ref.concat([b"banana", b"bandana", b"ananas"])
    ref = X.XRef(t, ds)
    for clamp in (False, True):                         # example 1: the clamp changes nothing here
        xl, src, xdoc = ref.match(X.OTHER, clamp)
        assert xl.tolist() == _row("3 5 4 3 2 1 3 2 1 0 3 2 1 5 4 3 2 1 0")
        assert src.tolist() == _row("6 13 14 10 11 12 0 15 16 - 3 4 5 1 2 1 2 7 -")
        assert xdoc.tolist() == _row("1 2 2 1 1 1 0 2 2 - 0 0 0 0 0 0 0 1 -")
    for L, want in ((1, [6, 6, 5]), (2, [6, 6, 5]), (3, [6, 6, 5])):
        shared, longest = ref.shared(X.OTHER, L)
        assert shared.tolist() == want and longest.tolist() == [5, 3, 5]
    xl, src, _ = ref.match(X.EARLIER, True)             # example 2
    assert xl.tolist() == _row("0 0 0 0 0 0 3 2 1 0 3 2 1 5 4 3 2 1 0")
    assert src.tolist() == _row("- - - - - - 0 1 2 - 3 4 5 1 2 1 2 7 -")
    shared, longest = ref.shared(X.EARLIER, 1)
    assert shared.tolist() == [0, 6, 5] and longest.tolist() == [0, 3, 5]

    t, ds = X.esa_docs_ref.concat([b"ab", b"cab", b"abc"])
    ref = X.XRef(t, ds)
    assert ds.tolist() == [0, 2, 5, 8]
    assert ref.match(X.OTHER, False)[0].tolist() == _row("3 2 1 2 1 3 2 1")      # example 3
    xl, src, xdoc = ref.match(X.OTHER, True)
    assert xl.tolist() == _row("2 1 1 2 1 3 2 1")
    assert src.tolist() == _row("5 6 7 5 6 0 1 2") and xdoc.tolist() == _row("2 2 2 2 2 0 0 1")
    cov = ref.cover(X.OTHER, 2)
    assert cov.astype(int).tolist() == _row("1 1 0 1 1 1 1 1")
    s, l, _ = cover_ref.spans(cov)
    assert list(zip(s.tolist(), l.tolist())) == [(0, 2), (3, 5)] and bytes(cover_ref.dedup(t, cov)) == b"c"
    for L, want in ((1, [2, 3, 3]), (2, [2, 2, 3]), (3, [0, 0, 3])):
        shared, longest = ref.shared(X.OTHER, L)
        assert shared.tolist() == want and longest.tolist() == [2, 2, 3]
    xl, src, xdoc = ref.match(X.EARLIER, True)          # example 4
    assert xl.tolist() == _row("0 0 0 2 1 3 2 1")
    assert src.tolist() == _row("- - - 0 1 0 1 2") and xdoc.tolist() == _row("- - - 0 0 0 0 1")
    cov = ref.cover(X.EARLIER, 2)
    assert cov.astype(int).tolist() == _row("0 0 0 1 1 1 1 1") and bytes(cover_ref.dedup(t, cov)) == b"abc"
