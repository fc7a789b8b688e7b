"""CPU-only: the reference of the repeat-cover tests (tests/cover_ref.py) against itself -- the seed definition against brute force
over all substrings, on every text over {a, b} up to 10 bytes and on 3000 random ones up to 40 bytes over at most 4 letters, for
both kinds; the four equivalent forms of include/textcomp.h against the references of the LPF array, the shortest unique prefixes
and the k-mers; the spans' two structural facts; and the eleven worked examples of the header, literally."""
import itertools

import numpy as np

import cover_ref as R
import kmer_ref
import lz_ref
import sus_ref

# text, L, q, kind -> spans, covered, mask (upper case = covered), dedup
EXAMPLES = [
    (b"mississippi", 2, 2, R.ALL, [(1, 7)], 7, b"mISSISSIppi", b"mppi"),
    (b"mississippi", 2, 2, R.LATER, [(4, 4)], 4, b"missISSIppi", b"missppi"),
    (b"mississippi", 1, 4, R.ALL, [(1, 7), (10, 1)], 8, b"mISSISSIppI", b"mpp"),
    (b"mississippi", 1, 4, R.LATER, [(3, 5), (10, 1)], 6, b"misSISSIppI", b"mispp"),
    (b"abcabcabc", 3, 3, R.ALL, [(0, 9)], 9, b"ABCABCABC", b""),
    (b"abcabcabc", 3, 2, R.LATER, [(3, 6)], 6, b"abcABCABC", b"abc"),
    (b"banana", 2, 2, R.LATER, [(3, 3)], 3, b"banANA", b"ban"),
    (b"aaaa", 2, 2, R.LATER, [(1, 3)], 3, b"aAAA", b"a"),
    (b"abcdabxcd", 2, 2, R.ALL, [(0, 6), (7, 2)], 8, b"ABCDABxCD", b"x"),
    (b"abcdabxcd", 2, 2, R.LATER, [(4, 2), (7, 2)], 4, b"abcdABxCD", b"abcdx"),
    (b"the cat sat; the cat ran", 4, 2, R.LATER, [(13, 8)], 8, b"the cat sat; THE CAT ran", b"the cat sat; ran"),
]


def _check(t, L, q, kind):
    cov = R.cover(t, L, q, kind)
    assert np.array_equal(cov, R.brute_cover(t, L, q, kind)), (t, L, q, kind)
    s, l, c = R.spans(cov)
    assert c == int(l.sum()) == int(cov.sum())
    assert all(int(x) >= L for x in l), (t, L, q, kind)
    assert len(s) <= (len(t) + 1) // (L + 1), (t, L, q, kind)
    assert all(int(a) + int(b) < int(c2) for a, b, c2 in zip(s, l, s[1:])), (t, L, q, kind)       # at least one byte apart
    assert len(R.dedup(t, cov)) == len(t) - c
    return cov


def test_worked_examples():
    assert len(EXAMPLES) == 11
    for t, L, q, kind, sp, covered, msk, dd in EXAMPLES:
        (s, l), c, m, d = R.reference(t, L, q, kind, R.UPPER)
        assert (list(zip(s.tolist(), l.tolist())), c, m.tobytes(), d) == (sp, covered, msk, dd), (t, L, q, kind)
        assert np.array_equal(R.brute_cover(t, L, q, kind), R.cover(t, L, q, kind))
        want01 = [0] * len(t)
        for s0, l0 in sp:
            want01[s0:s0 + l0] = [1] * l0
        assert R.mask(t, R.cover(t, L, q, kind)).tolist() == want01
    (s, l), c, m, d = R.reference(b"", 1)
    assert (len(s), len(l), c, len(m), d) == (0, 0, 0, 0, b"")
    (s, l), c, m, d = R.reference(b"abab", 5, 2, R.ALL, R.UPPER)        # min_len > n: nothing is covered
    assert (len(s), c, m.tobytes(), d) == (0, 0, b"abab", b"abab")


def test_every_binary_text_up_to_10():
    for n in range(0, 11):
        for t in itertools.product(b"ab", repeat=n):
            for L in (1, 2, 3, 4):
                for q in (2, 3):
                    for kind in (R.ALL, R.LATER):
                        _check(bytes(t), L, q, kind)


def test_random_texts_up_to_40():
    rng = np.random.default_rng(0xC0BE)
    for _ in range(3000):
        n = int(rng.integers(1, 41))
        sigma = int(rng.integers(1, 5))
        t = bytes(b"acgt"[int(c)] for c in rng.integers(0, sigma, n))
        _check(t, int(rng.integers(1, 7)), int(rng.integers(2, 5)), int(rng.integers(0, 2)))


def _texts():
    rng = np.random.default_rng(0xC0BF)
    for _ in range(300):
        n = int(rng.integers(1, 61))
        yield bytes(b"acgt"[int(c)] for c in rng.integers(0, int(rng.integers(1, 5)), n))
    yield from (sus_ref.fibonacci(55), b"ab" * 20, b"abc" * 13 + b"a", b"a" * 30, b"acgtacga" * 3)


def test_later_at_two_is_the_union_of_the_lpf_stretches():
    for t in _texts():
        lpf = lz_ref.lpf_src(t)[0]
        for L in (1, 2, 3, 5):
            assert np.array_equal(R.cover(t, L, 2, R.LATER), R.cover_of_len(lpf, L)), (t, L)


def test_all_at_two_seeds_are_read_off_the_unique_prefixes():
    for t in _texts():
        up = sus_ref.reference(t)[0].astype(np.int64)
        n = len(t)
        for L in (1, 2, 3, 5):
            want = [i for i in range(n) if i + L <= n and (up[i] == 0 or up[i] > L)]
            assert R.seeds(t, L, 2, R.ALL) == want, (t, L)


def test_all_seeds_are_the_positions_of_the_frequent_kmers():
    for t in _texts():
        sa, lcp = kmer_ref.esa(t)
        for L in (1, 2, 4):
            for q in (2, 3, 5):
                row, pos, occ = kmer_ref.by_esa(sa, lcp, L, q, 0)
                want = sorted(int(sa[r + j]) for r, o in zip(row, occ) for j in range(o))
                assert R.seeds(t, L, q, R.ALL) == want, (t, L, q)


def test_general_form_clamps_and_ignores_short_entries():
    ln = np.array([0, 3, 0, 0, 0, 2, 0xffffffff, 0, 0], np.uint32)
    assert R.cover_of_len(ln, 3).tolist() == [False, True, True, True, False, False, True, True, True]
    assert R.cover_of_len(ln, 2).tolist() == [False, True, True, True, False, True, True, True, True]
    assert R.cover_of_len(np.zeros(5, np.uint32), 1).tolist() == [False] * 5
    assert R.spans(R.cover_of_len(ln, 3))[:2][0].tolist() == [1, 6]
