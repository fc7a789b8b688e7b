"""CPU-only: the reference of the two-text device tests (tests/textmatch_ref.py) against itself.  Plain brute force
(bytes.find and counting) and the definitions on a naive enhanced suffix array of Q T -- the nearest T rows, the range
minima between, the clamp to Q's end, the T rows of the LCP interval -- agree on the three examples of include/textcomp.h
and on random pairs over 1, 2, 4 and 256 letters with a, b <= 40; the MEM rule and the LCS follow from the arrays."""
import numpy as np

import textmatch_ref as R


def _pairs():
    out = [(b"", b""), (b"", b"a"), (b"a", b""), (b"a", b"a"), (b"a", b"b"), (b"ab", b"ba"), (b"abab", b"ab"),
           (b"ab" * 5, b"ab" * 3), (b"ab" * 3, b"ab" * 5), (b"a" * 12, b"baaa"), (b"baaa", b"a" * 12)]
    rng = np.random.default_rng(0x7e47)
    for sigma in (1, 2, 4, 256):
        for k in range(24):
            a, b = int(rng.integers(0, 41)), int(rng.integers(0, 41))
            out.append((R.random_text(0x4100 + 64 * sigma + k, a, sigma), R.random_text(0x4900 + 64 * sigma + k, b, sigma)))
    return out


def test_the_examples_of_the_header():
    for q, t, ms_len, ms_pos, ms_occ, mems in R.EXAMPLES:
        assert R.brute(q, t) == (ms_len, ms_pos, ms_occ), (q, t)
        assert R.by_esa(q, t) == (ms_len, ms_pos, ms_occ), (q, t)
        start, pos, ln = R.mems_of(ms_len, ms_pos, 1)
        assert list(zip(start.tolist(), pos.tolist(), ln.tolist())) == mems
    assert R.lcs_of(*R.EXAMPLES[0][2:4]) == (5, 1, 0, 15)
    assert R.lcs_of(*R.EXAMPLES[1][2:4]) == (2, 0, 2, 3)
    assert R.lcs_of(*R.EXAMPLES[2][2:4]) == (3, 0, 0, 12)
    assert R.lcs_of([], []) == (0, 0, 0, 0) and R.lcs_of([0, 0], [0, 0]) == (0, 0, 0, 0)


def test_brute_force_and_suffix_array_restatement_agree():
    pairs = _pairs()
    assert len(pairs) >= 100
    clamped = 0
    for q, t in pairs:
        ms_len, ms_pos, ms_occ = R.brute(q, t)
        assert (ms_len, ms_pos, ms_occ) == R.by_esa(q, t), (q, t)
        for i, l in enumerate(ms_len):
            if l:
                assert q[i:i + l] == t[ms_pos[i]:ms_pos[i] + l] and ms_occ[i] >= 1
                assert i + l == len(q) or q[i:i + l + 1] not in t
                clamped += i + l == len(q) and (q + t)[i:i + l + 1] in t
            else:
                assert ms_pos[i] == 0 and ms_occ[i] == 0 and q[i:i + 1] not in t
            assert i == 0 or ms_len[i - 1] <= l + 1
    assert clamped >= 20        # matches that would run over q's end into t's head: the clamp of by_esa is exercised


def test_same_text_on_both_sides():
    for t in (b"abracadabra", b"aaaa", R.random_text(0x51, 33, 2)):
        ms_len, ms_pos, _ = R.by_esa(t, t)
        assert ms_len == [len(t) - i for i in range(len(t))]
        assert R.brute(t, t)[0] == ms_len
        assert R.lcs_of(ms_len, ms_pos)[:2] == (len(t), 0)


def test_mem_rule_on_arrays_no_text_produces():
    ln = np.array([3, 3, 2, 0x80000001, 0x80000000, 5, 0, 0, 1], np.uint32)
    ps = np.arange(len(ln), dtype=np.uint32) + 100
    start, pos, out = R.mems_of(ln, ps, 1)
    assert start.tolist() == [0, 1, 3, 8] and pos.tolist() == [100, 101, 103, 108]
    assert out.tolist() == [3, 3, 0x80000001, 1]
    assert R.mems_of(ln, ps, 4)[0].tolist() == [3]
    assert R.mems_of(ln.view(np.int32), ps.view(np.int32), 4)[0].tolist() == [3]    # signed views of the same words
