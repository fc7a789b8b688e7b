"""CPU-only: the reference of the repeats tests (tests/rep_ref.py) against itself -- the suffix-array rule with its
representative rows against brute force over all substrings, on texts of at most 30 bytes, both kinds, with filters -- and
the worked examples of include/textcomp.h, literally."""
import numpy as np
import pytest

import rep_ref as R


def _named(t, kind, **kw):
    pos, ln, occ, row, sa = R.repeats(t, kind, **kw)
    return {w.decode(): len(ps) for w, ps in R.as_dict(t, pos, ln, occ, row, sa).items()}


def test_worked_examples():
    assert _named(b"mississippi", R.MAXIMAL) == {"i": 4, "issi": 2, "p": 2, "s": 4}
    assert _named(b"mississippi", R.SUPERMAXIMAL) == {"issi": 2, "p": 2}
    assert _named(b"a" * 8, R.MAXIMAL) == {"a" * k: 9 - k for k in range(1, 8)}
    assert _named(b"a" * 8, R.SUPERMAXIMAL) == {"a" * 7: 2}
    assert _named(b"abcabcabc", R.MAXIMAL) == {"abc": 3, "abcabc": 2}
    assert _named(b"abcabcabc", R.SUPERMAXIMAL) == {"abcabc": 2}
    for t in (b"", b"a", b"ab"):
        assert _named(t, R.MAXIMAL) == {} and _named(t, R.SUPERMAXIMAL) == {}
    assert _named(b"aa", R.MAXIMAL) == {"a": 2} and _named(b"aa", R.SUPERMAXIMAL) == {"a": 2}


def test_order_is_by_representative_row_not_by_first_row():
    """the example of the header: for equal first rows the longer repeat first; first rows do not ascend"""
    pos, ln, occ, row, sa = R.repeats(b"abcabcabc", R.MAXIMAL)
    assert (row.tolist(), ln.tolist(), occ.tolist()) == ([1, 2], [3, 6], [3, 2])
    pos, ln, occ, row, sa = R.repeats(b"aaabaab", R.MAXIMAL)    # "aa" [1, 3], "aab" [2, 3], "a" [1, 5]
    assert sa.tolist() == [7, 0, 4, 1, 5, 2, 6, 3]
    assert (row.tolist(), ln.tolist(), occ.tolist(), pos.tolist()) == ([1, 2, 1], [2, 3, 1], [3, 2, 5], [0, 4, 0])


def _texts():
    rng = np.random.default_rng(0x5e9)
    out = [b"", b"a", b"aa", b"ab", b"mississippi", b"a" * 8, b"abcabcabc", b"abracadabra", b"a" * 28, b"ab" * 14, b"abc" * 9 + b"a"]
    for sigma in (1, 2, 3, 4):
        for _ in range(40):
            n = int(rng.integers(0, 31))
            out.append(bytes(b"acgt"[int(c)] for c in rng.integers(0, sigma, n)))
    for p in (2, 3, 5, 7):
        for n in (9, 20, 30):
            unit = bytes(b"acgt"[int(c)] for c in rng.integers(0, 3, p))
            out.append((unit * 30)[:n])
    out.append(R.fibonacci(30))
    return out


@pytest.mark.parametrize("kind", [R.MAXIMAL, R.SUPERMAXIMAL])
def test_esa_rule_against_brute_force(kind):
    for t in _texts():
        for kw in ({}, {"min_len": 2}, {"min_occ": 3}, {"min_len": 3, "min_occ": 3}, {"min_len": 40}):
            pos, ln, occ, row, sa = R.repeats(t, kind, **kw)
            got = R.as_dict(t, pos, ln, occ, row, sa)
            assert got == R.brute(t, kind, **kw), (t, kind, kw)
            assert (occ.astype(np.int64) == [len(got[t[p:p + l]]) for p, l in zip(pos.tolist(), ln.tolist())]).all()
            assert len(pos) < max(len(t), 1)            # fewer than n maximal repeats: capacity n is always enough


def test_many_left_contexts():
    """the 257-occurrence text: w = 01 02 03 is supermaximal with all 257 left contexts distinct; with one left context
    doubled it is not"""
    w = bytes([1, 2, 3])
    t = R.many_left()
    assert len(t) == 3 + 256 * 4
    d = R.as_dict(t, *R.repeats(t, R.SUPERMAXIMAL))
    assert len(d[w]) == 257
    assert all(len(ps) <= 257 for ps in d.values())
    assert len(R.as_dict(t, *R.repeats(t, R.MAXIMAL))[w]) == 257
    t2 = R.many_left(doubled=7)
    assert w not in R.as_dict(t2, *R.repeats(t2, R.SUPERMAXIMAL))
    assert len(R.as_dict(t2, *R.repeats(t2, R.MAXIMAL))[w]) == 257
