"""CPU-only: the reference of the unique-substring tests (tests/sus_ref.py) against itself -- the row rule, the MUS rule and the
three-candidate point answer against brute force over all substrings, on every text over {a, b} up to 10 bytes and on a few
thousand random ones up to 40 bytes over at most 4 letters -- with the worked examples of include/textcomp.h, literally, and the
two structural facts: MUS ends increase strictly, and neighbouring point answers differ in length by at most one."""
import itertools

import numpy as np

import sus_ref as S

EXAMPLES = {
    b"mississippi": ([1, 5, 4, 3, 5, 4, 3, 2, 2, 2, 0], [(0, 1), (3, 3), (7, 2), (8, 2), (9, 2)],
                     [(0, 1), (0, 2), (0, 3), (3, 3), (3, 3), (3, 3), (6, 3), (7, 2), (7, 2), (8, 2), (9, 2)]),
    b"abaab": ([3, 2, 2, 0, 0], [(1, 2), (2, 2)], [(0, 3), (1, 2), (1, 2), (2, 2), (2, 3)]),
    b"banana": ([1, 4, 3, 0, 0, 0], [(0, 1), (2, 3)], [(0, 1), (0, 2), (0, 3), (2, 3), (2, 3), (2, 4)]),
    b"abcabc": ([4, 3, 2, 0, 0, 0], [(2, 2)], [(0, 4), (1, 3), (2, 2), (2, 2), (2, 3), (2, 4)]),
    b"aaaa": ([4, 0, 0, 0], [(0, 4)], [(0, 4)] * 4),
    b"a": ([1], [(0, 1)], [(0, 1)]),
}


def _ref(t):
    up, (ms, ml), (ss, sl) = S.reference(t)
    return up.tolist(), list(zip(ms.tolist(), ml.tolist())), list(zip(ss.tolist(), sl.tolist()))


def _check(t):
    up, mus, point = _ref(t)
    assert (up, mus, point) == S.brute(t), t
    ends = [s + l - 1 for s, l in mus]
    assert all(a < b for a, b in zip(ends, ends[1:])), t
    assert all(abs(a[1] - b[1]) <= 1 for a, b in zip(point, point[1:])), t
    assert len(mus) >= (1 if t else 0) and len(mus) <= len(t)


def test_worked_examples():
    for t, want in EXAMPLES.items():
        assert _ref(t) == want, t
        assert S.brute(t) == want, t
    assert _ref(b"") == ([], [], [])


def test_every_binary_text_up_to_10():
    for n in range(0, 11):
        for t in itertools.product(b"ab", repeat=n):
            _check(bytes(t))


def test_random_texts_up_to_40():
    rng = np.random.default_rng(0x5051)
    for _ in range(3000):
        n = int(rng.integers(1, 41))
        sigma = int(rng.integers(1, 5))
        _check(bytes(b"acgt"[int(c)] for c in rng.integers(0, sigma, n)))
    for t in (S.fibonacci(34), b"ab" * 15, b"abc" * 9 + b"a", b"acgtacga" * 2):
        _check(t)


def test_windows_keep_the_order():
    rng = np.random.default_rng(0x5052)
    for _ in range(200):
        t = bytes(b"acgt"[int(c)] for c in rng.integers(0, 3, int(rng.integers(1, 41))))
        up = S.reference(t)[0]
        ms, ml = S.mus_from_up(up)
        for lo, hi in ((1, 0), (2, 0), (1, 1), (3, 5), (50, 0)):
            keep = (ml >= lo) & ((ml <= hi) if hi else True)
            fs, fl = S.mus_from_up(up, lo, hi)
            assert (fs.tolist(), fl.tolist()) == (ms[keep].tolist(), ml[keep].tolist())


def test_staircase_has_its_properties():
    """the figures the GPU test's staircase case relies on, from the reference alone"""
    t = S.staircase()
    up, (ms, ml), (ss, sl) = S.reference(t)
    assert len(t) == 47993
    me = ms.astype(np.int64) + ml - 1
    cover = np.zeros(len(t) + 1, np.int64)
    np.add.at(cover, ms, 1)
    np.add.at(cover, me + 1, -1)
    assert int(np.cumsum(cover).max()) >= 65
