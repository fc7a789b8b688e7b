"""CPU-only: the reference of the LZ77 device tests (tests/lz_ref.py) against itself.  The brute force over all j < i and
the suffix-array restatement (nearest rows above and below with sa < i, the minimum of lcp over the rows between) agree on
unary, periodic, Fibonacci and random texts over 1 to 4 letters; the neighbour rule that defines src attains the maximum
that defines lpf; the parse is a valid phrase list whose unparse is the text."""
import numpy as np

import lz_ref as R


def _texts():
    out = [b"", b"a", b"aa", b"ab", b"a" * 64, b"abracadabra"]
    for n in (1, 2, 3, 7, 30, 65):
        out.append(b"a" * n)
        for p in (2, 3, 7):
            out.append(R.periodic(n, p))
        out.append(R.fibonacci(n))
    for sigma in (1, 2, 3, 4):
        for k, n in enumerate((1, 2, 5, 17, 33, 40, 64, 90)):
            out.append(R.random_text(0x1200 + 16 * sigma + k, n, sigma))
    out.append(R.random_text(0x12ff, 50, 256))
    return out


def test_brute_force_and_suffix_array_restatement_agree():
    texts = _texts()
    assert len(texts) >= 60
    for t in texts:
        lpf, src, best = R.brute(t)
        assert lpf == best, t                               # the neighbour rule attains the maximum
        for i in range(len(t)):
            if lpf[i]:
                assert src[i] < i and t[src[i]:src[i] + lpf[i]] == t[i:i + lpf[i]]
                assert i + lpf[i] == len(t) or src[i] + lpf[i] == len(t) or t[src[i] + lpf[i]] != t[i + lpf[i]]
            else:
                assert src[i] == 0 and t[i] not in t[:i]
        assert (lpf, src) == R.by_esa(t), t


def test_suffix_array_and_lcp_of_the_reference():
    for t in _texts():
        sa = R.suffix_array(t).tolist()
        assert sa == sorted(range(len(t) + 1), key=lambda j: t[j:]), t
        lcp = R.lcp_array(t, np.array(sa, np.int64))
        assert lcp[0] == 0 and all(lcp[j] == R._lcp(t, sa[j - 1], sa[j]) for j in range(1, len(sa)))


def test_parse_examples_and_round_trip():
    ps, pl = R.parse(b"a" * 64)
    assert ps.tolist() == [97, 0] and pl.tolist() == [0, 63]
    ps, pl = R.parse(b"")
    assert len(ps) == 0 and len(pl) == 0
    ps, pl = R.parse(b"abab")
    assert ps.tolist() == [97, 98, 0] and pl.tolist() == [0, 0, 2]
    for t in _texts():
        ps, pl = R.parse(t)
        assert ps.dtype == np.uint32 and pl.dtype == np.uint32
        assert R.valid(ps, pl) and R.unparse(ps, pl) == t
        assert sum(max(int(l), 1) for l in pl) == len(t)


def test_valid_refuses_what_unparse_refuses():
    assert R.valid([97, 0], [0, 63])
    assert not R.valid([0], [1])                            # a copy at position 0
    assert not R.valid([97, 1], [0, 3])                     # src = start
    assert not R.valid([97, 2], [0, 3])                     # src > start
    assert not R.valid([256], [0])                          # a literal above 255
    assert R.unparse([97, 98, 0, 1], [0, 0, 1, 5]) == b"abababab"[:8]
