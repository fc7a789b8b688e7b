"""CPU-only: the two references of tests/pal_ref.py agree -- the definition of a palindrome with mismatches taken literally
(brute: all substrings, the pairs counted, the outermost pair matching, the longest per centre) and the numpy method
(palindromes) that the device tests compare tc_palindromes with -- on every string over ab up to length 10, on random strings
over 1 to 5 letters up to length 40, under the identity and the DNA complement, for the budgets 0 .. 3 and 16 and several
min_len, and on the worked examples of include/textcomp.h."""
import itertools

import numpy as np

import pal_ref as R

BUDGETS = (0, 1, 2, 3, 16)


def _pals(t, *a):
    return R.as_triples(*R.palindromes(t, *a))


def test_header_examples():
    assert R.brute(b"mississippi", None, 0, 3) == [(1, 4, 0), (1, 7, 0), (4, 4, 0), (7, 4, 0)]
    assert R.brute(b"ACGT", R.DNA) == [(0, 4, 0)]
    assert R.brute(b"ACAGT", R.DNA) == []
    assert R.brute(b"ACAGT", R.DNA, 1) == [(0, 5, 1), (2, 3, 1)]
    for t, comp, m, min_len in ((b"mississippi", None, 0, 3), (b"mississippi", None, 0, 1), (b"ACGT", R.DNA, 0, 1),
                                (b"ACAGT", R.DNA, 0, 1), (b"ACAGT", R.DNA, 1, 1)):
        assert _pals(t, comp, m, min_len) == R.brute(t, comp, m, min_len)
    assert R.longest(b"mississippi") == (1, 7, 0) and R.longest(b"ACAC", R.DNA) == (0, 0, 0) and R.longest(b"") == (0, 0, 0)
    assert R.longest(b"abab") == (0, 3, 0)          # aba and bab: the smaller centre


def test_every_text_over_ab_up_to_10_bytes():
    swap = R.IDENTITY.copy()
    swap[ord("a")], swap[ord("b")] = ord("b"), ord("a")
    for n in range(0, 11):
        for bits in itertools.product(b"ab", repeat=n):
            t = bytes(bits)
            for comp in (None, swap):
                for m in (0, 1, 3) if n > 7 else BUDGETS:
                    got = _pals(t, comp, m)
                    assert got == R.brute(t, comp, m), (t, m)
                    assert len(got) < max(2 * n, 1)
                    centres = [2 * s + l - 1 for s, l, _ in got]
                    assert centres == sorted(set(centres))      # one per centre, in increasing centre


def test_random_texts_over_1_to_5_letters():
    rng = np.random.RandomState(0x9a1)
    letters = np.frombuffer(b"ACGTN", np.uint8)
    for it in range(400):
        n = int(rng.randint(0, 41))
        t = letters[rng.randint(0, 1 + it % 5, n)]
        for comp in (None, R.DNA):
            m = BUDGETS[it % len(BUDGETS)]
            for min_len in (1, 2, 5):
                assert _pals(t, comp, m, min_len) == R.brute(t, comp, m, min_len), (bytes(t), m, min_len)
            s, ln, mm = R.palindromes(t, comp, m)
            want = (0, 0, 0)
            if len(ln):
                k = min(range(len(ln)), key=lambda j: (-int(ln[j]), 2 * int(s[j]) + int(ln[j])))
                want = (int(s[k]), int(ln[k]), int(mm[k]))
            assert R.longest(t, comp, m) == want


def test_unary_closed_form_and_planted_texts():
    for n in range(1, 30):
        for ch in (b"a", b"A"):
            for comp in (None, R.DNA):
                for m in (0, 2):
                    assert _pals(ch * n, comp, m) == R.brute(ch * n, comp, m), (ch, n, m)
    rng = np.random.default_rng(7)
    for comp in (None, R.DNA):
        t = R.planted(rng, 60, comp)
        for m in (0, 1, 3):
            assert _pals(t, comp, m, 4) == R.brute(t, comp, m, 4)
        assert R.longest(R.planted(rng, 3000, comp), comp, 3)[1] >= 20
