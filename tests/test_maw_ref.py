"""CPU-only: the reference of the absent-word tests (tests/maw_ref.py) against itself -- the row rule with its order against
brute force over all substrings, on texts of at most 16 bytes over 1, 2, 3, 4 and 6 letters and over all 256 byte values,
periodic and doubled texts among them -- and the worked examples of include/textcomp.h, literally."""
import numpy as np
import pytest

import maw_ref as M


def _triples(t, **kw):
    a, p, l = M.absent_words(t, **kw)
    return list(zip(bytes(a).decode("latin-1"), p.tolist(), l.tolist()))


def _words(t, **kw):
    return [w.decode("latin-1") for w in M.words(t, *M.absent_words(t, **kw))]


def test_worked_examples():
    assert _triples(b"abaab") == [("a", 2, 3), ("b", 3, 3), ("a", 0, 4), ("b", 4, 2)]
    assert _words(b"abaab") == ["aaa", "bab", "aaba", "bb"]
    assert _triples(b"aaabaab") == [("a", 0, 4), ("b", 0, 4), ("b", 1, 5), ("b", 5, 3), ("b", 6, 2)]
    assert _words(b"aaabaab") == ["aaaa", "baaa", "baaba", "bab", "bb"]
    assert _words(b"mississippi") == "ii mip pip pis missip sissis im mm pm sm mp sp ipi ppp ms ps isi sss".split()
    assert _words(b"") == []


def test_unary_texts_have_their_one_longer_power():
    """a^n occurs and a^(n + 1) does not, and its two factors of length n are a^n: by the definition that is a minimal absent
    word, the only one; so a text of one byte has the word of two"""
    for n in range(1, 17):
        assert _triples(b"a" * n) == [("a", 0, n + 1)]
        assert M.brute(b"a" * n) == {b"a" * (n + 1)}


def test_all_bytes_once():
    t = M.all_bytes()
    a, p, l = M.absent_words(t)
    assert len(a) == 65281 and (l == 2).all()
    pairs = {bytes(t[i:i + 2]) for i in range(255)}
    got = set(M.words(t, a, p, l))
    assert len(got) == 65281 and not (got & pairs) and len(got | pairs) == 65536
    hist, total = M.profile(t, 4)
    assert hist.tolist() == [0, 0, 65281, 0, 0] and total == 65281


def _texts():
    rng = np.random.default_rng(0x3a7)
    out = [b"", b"a", b"aa", b"ab", b"ba", b"abaab", b"aaabaab", b"mississippi", b"abracadabra", b"a" * 16, b"ab" * 8, b"abc" * 5 + b"a"]
    for sigma in (1, 2, 3, 4, 6):
        for _ in range(60):
            n = int(rng.integers(0, 17))
            out.append(bytes(b"acgtnx"[int(c)] for c in rng.integers(0, sigma, n)))
    for _ in range(40):                             # 256-valued bytes
        out.append(rng.integers(0, 256, int(rng.integers(0, 17)), dtype=np.uint8).tobytes())
    for p in (2, 3, 5, 7):                          # periodic
        for n in (9, 13, 16):
            unit = bytes(b"acgt"[int(c)] for c in rng.integers(0, 3, p))
            out.append((unit * 16)[:n])
    for _ in range(20):                             # a text followed by its copy
        half = bytes(b"acgt"[int(c)] for c in rng.integers(0, int(rng.integers(1, 5)), int(rng.integers(1, 9))))
        out.append(half + half)
    out.append(M.fibonacci(16))
    return out


def test_row_rule_against_brute_force():
    for t in _texts():
        a, p, l = M.absent_words(t)
        w = M.words(t, a, p, l)
        assert len(set(w)) == len(w), t             # every word once
        assert set(w) == M.brute(t), t
        assert (l >= 2).all()
        for lo, hi in ((2, 2), (3, 0), (3, 5), (2, 16), (20, 0)):
            keep = (l >= lo) & ((l <= hi) if hi else True)
            fa, fp, fl = M.absent_words(t, lo, hi)  # a window keeps the order
            assert (fa.tolist(), fp.tolist(), fl.tolist()) == (a[keep].tolist(), p[keep].tolist(), l[keep].tolist()), (t, lo, hi)


@pytest.mark.parametrize("kmax", [2, 5, 40])
def test_profile_is_the_histogram_of_the_list(kmax):
    for t in _texts():
        _, _, l = M.absent_words(t)
        hist, total = M.profile(t, kmax)
        assert len(hist) == kmax + 1 and hist[0] == 0 and hist[1] == 0 and total == len(l)
        assert hist.tolist() == [int((l == k).sum()) for k in range(kmax + 1)]
