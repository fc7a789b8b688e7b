"""CPU-only: the two references of tests/kmer_ref.py -- collections.Counter over the text, and the boundary definition on a
naive suffix array and LCP array -- are held to each other, to the worked examples of include/textcomp.h, to the sum of the
occurrence counts and to both profile formulas, on random texts of up to 60 bytes over 1, 2, 3, 4 and 256 letters at every
k up to n + 2.  The same file keeps KM_TILE of tests/test_gpu_kmers.py equal to csrc/tc_kmer.hpp."""
import os
import re

import numpy as np
import pytest

import kmer_ref as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILTERS = [(1, 0), (1, 1), (2, 0), (3, 5), (2, 2)]


def _texts():
    rng = np.random.default_rng(0x6b6d6572)
    out = [b"", b"a", b"ab", b"aa"]
    for sigma in (1, 2, 3, 4, 256):
        for _ in range(14):
            n = int(rng.integers(0, 61))
            out.append(bytes(rng.integers(0, sigma, n, dtype=np.uint8) if sigma == 256
                             else rng.integers(97, 97 + sigma, n, dtype=np.uint8)))
    return out


def test_worked_examples():
    for t, k, want in K.EXAMPLES:
        sa, lcp = K.esa(t)
        if t in K.EXAMPLE_ESA:
            assert (sa.tolist(), lcp.tolist()) == K.EXAMPLE_ESA[t]
        row, pos, occ = K.by_esa(sa, lcp, k)
        assert list(zip(row, pos, occ)) == want, (t, k)
        assert [(t[p:p + k], o) for _, p, o in want] == K.by_counter(t, k)
    assert [w for w, _ in K.by_counter(b"mississippi", 2)] == [b"ip", b"is", b"mi", b"pi", b"pp", b"si", b"ss"]


@pytest.mark.parametrize("part", range(4))
def test_the_two_references_agree(part):
    for t in _texts()[part::4]:
        n = len(t)
        sa, lcp = K.esa(t)
        for k in range(1, n + 3):
            for mn, mx in FILTERS:
                row, pos, occ = K.by_esa(sa, lcp, k, mn, mx)
                assert [(t[p:p + k], o) for p, o in zip(pos, occ)] == K.by_counter(t, k, mn, mx), (t, k, mn, mx)      # the list and its order
                assert all(int(sa[r]) == p for r, p in zip(row, pos))
                for r, p, o in zip(row, pos, occ):                                                                   # all occurrences
                    assert sorted(int(x) for x in sa[r:r + o]) == [i for i in range(n - k + 1) if t[i:i + k] == t[p:p + k]]
            _, _, occ = K.by_esa(sa, lcp, k)
            assert sum(occ) == max(0, n - k + 1)
            assert sum(o for _, o in K.by_counter(t, k)) == max(0, n - k + 1)
            for bins in (1, 2, 7):
                hist, distinct, total = K.spectrum(t, k, bins)
                assert hist == K.spectrum_of(occ, bins) and sum(hist) == distinct == len(occ) and total == max(0, n - k + 1)
        kmax = n + 2
        assert K.profile_by_lcp(lcp, kmax) == K.profile(t, kmax), t


def test_km_tile_of_the_gpu_test_is_the_kernels():
    src = open(os.path.join(ROOT, "text-compression_amd", "csrc", "tc_kmer.hpp")).read()
    tile = int(re.search(r"#define KM_TILE (\d+)", src).group(1))
    assert tile == int(re.search(r"#define KM_NT (\d+)", src).group(1)) * int(re.search(r"#define KM_ROWS (\d+)", src).group(1))
    gpu = open(os.path.join(ROOT, "tests", "test_gpu_kmers.py")).read()
    assert int(re.search(r"^KM_TILE = (\d+)", gpu, flags=re.M).group(1)) == tile
