"""Reference for the suffix array + LCP array tests: pure Python / numpy, independent of the code under test.

  esa_direct(text)   suffixes sorted directly (the empty suffix first), neighbours compared byte by byte: n <= ~4000
  kasai(text, sa)    the LCP array of a given suffix array (Kasai et al. 2001): larger texts, over a suffix array the
                     existing suite pins (tc_suffix_array)
  unary_lcp(n), periodic_lcp(text, p)   closed forms, a second opinion at the larger sizes
  planted_pair(rng, m, ending)          a text with one irreducible comparison of exactly m bytes, stopping at the end of
                                        the text or at a differing byte
  long_items(text, sa, cap)             the values a short cap sends on to the long-compare kernel (csrc/tc_lcp.hpp step 3):
                                        what a test asserts about its own input before it trusts it

Conventions of include/textcomp.h: sa has n + 1 rows, 0-based starts, row 0 the empty suffix (sa[0] = n); lcp[0] = 0,
lcp[j] = longest common prefix of the suffixes at sa[j - 1] and sa[j]; the end of the text matches nothing."""
import numpy as np


def esa_direct(text):
    t = bytes(text)
    n = len(t)
    sa = sorted(range(n + 1), key=lambda i: t[i:])
    lcp = [0] * (n + 1)
    for j in range(1, n + 1):
        a, b = t[sa[j - 1]:], t[sa[j]:]
        l = 0
        while l < len(a) and l < len(b) and a[l] == b[l]:
            l += 1
        lcp[j] = l
    return np.array(sa, np.uint32), np.array(lcp, np.uint32)


def _match_len(t, a, b, n):
    """longest common prefix of t[a:] and t[b:], by doubling blocks (numpy compares the blocks)"""
    l, step = 0, 64
    while True:
        k = min(step, n - a - l, n - b - l)
        if k <= 0:
            return l
        x, y = t[a + l:a + l + k], t[b + l:b + l + k]
        d = np.flatnonzero(x != y)
        if len(d):
            return l + int(d[0])
        l += k
        step *= 2


def kasai(text, sa):
    """LCP array of suffix array sa (n + 1 rows, row 0 the empty suffix) in text order, h decreasing by at most one a
    step; the byte comparisons go through numpy blocks, so that a long repeat costs no Python loop per byte"""
    t = np.frombuffer(bytes(text), np.uint8) if not isinstance(text, np.ndarray) else text
    n = len(t)
    sa = np.asarray(sa, np.int64)
    rank = np.empty(n + 1, np.int64)
    rank[sa] = np.arange(n + 1)
    lcp = np.zeros(n + 1, np.uint32)
    sal, rankl = sa.tolist(), rank.tolist()
    tb = t.tobytes()
    out = [0] * (n + 1)
    h = 0
    for i in range(n):
        j = sal[rankl[i] - 1]     # rank[i] >= 1: row 0 is the empty suffix
        m = n - max(i, j)
        while h < m and tb[i + h] == tb[j + h]:
            h += 1
            if h & 63 == 0 and h < m:      # a long match: leave the byte loop
                h += _match_len(t, i + h, j + h, n)
                break
        out[rankl[i]] = h
        if h:
            h -= 1
    lcp[:] = out
    return lcp


def unary_lcp(n):
    """text = one byte n times: sa = n, n - 1, .., 0 and lcp[j] = j - 1 (lcp[0] = 0)"""
    lcp = np.arange(-1, n, dtype=np.int64)
    lcp[0] = 0
    return np.arange(n, -1, -1).astype(np.uint32), lcp.astype(np.uint32)


def periodic_lcp_of_rows(sa, n, p):
    """text of period p whose first p bytes are pairwise distinct as ROTATIONS (e.g. a random block: every suffix pair
    at a distance that is a multiple of p agrees to the end of the shorter one): for neighbouring rows whose starts
    differ by a multiple of p, lcp = n - max of the two starts.  -> (mask of such rows, their lcp)"""
    sa = np.asarray(sa, np.int64)
    a, b = sa[:-1], sa[1:]
    mask = np.zeros(len(sa), bool)
    val = np.zeros(len(sa), np.uint32)
    same = ((a - b) % p == 0) & (a < n) & (b < n)
    mask[1:] = same
    val[1:][same] = (n - np.maximum(a, b))[same]
    return mask, val


LETTERS = np.frombuffer(b"ACGTNBDEFHIJKLMO", np.uint8)      # the alphabets of planted_pair; separators lie outside


def planted_pair(rng, m, ending, sigma=4, seps=b"#$", tail=5):
    """A text with exactly one irreducible comparison of m bytes: a random block B of m bytes over sigma letters, twice.
      ending "end"       B + seps[0] + B                        the second copy runs to the end of the text: the
                                                                comparison stops there (lim == m)
      ending "mismatch"  B + seps[0] + B + seps[1] + tail       it stops at a differing byte, text left on both sides
    (tail: that many random letters).  The two copies start behind different bytes, so the later one in suffix order is
    irreducible.  Several "mismatch" pairs may follow one another in one text when their separators differ.  -> bytes"""
    assert ending in ("end", "mismatch") and 2 <= sigma <= len(LETTERS) and len(seps) >= 2 and seps[0] != seps[1]
    assert not set(seps) & set(LETTERS[:sigma].tobytes())
    block = LETTERS[rng.integers(0, sigma, m)].tobytes()
    text = block + seps[0:1] + block
    if ending == "mismatch":
        text += seps[1:2] + LETTERS[rng.integers(0, sigma, tail)].tobytes()
    return text


def long_items(text, sa, cap, lcp=None):
    """What lcp_irreducible_kernel hands to lcp_long_kernel at short cap `cap`, from phi, the Kasai LCP array and the
    byte in front: the positions i with a predecessor phi[i] in suffix order that are irreducible (i == 0, phi[i] == 0
    or T[i - 1] != T[phi[i] - 1]), whose PLCP[i] = lcp(i, phi[i]) reaches the cap, with text left behind the cap
    (lim = n - max(i, phi[i]) > cap).  -> (PLCP values of those that stop at a differing byte, PLCP < lim;
    PLCP values of those that stop at the end of the text, PLCP == lim), each sorted.  lcp: kasai(text, sa) if at hand."""
    t = np.frombuffer(bytes(text), np.uint8) if not isinstance(text, np.ndarray) else text
    n = len(t)
    sa = np.asarray(sa, np.int64)
    if lcp is None:
        lcp = kasai(t, sa)
    i, phi = sa[1:], sa[:-1]                     # row j >= 1: position sa[j], its predecessor sa[j - 1]
    plcp = np.asarray(lcp, np.int64)[1:]
    lim = n - np.maximum(i, phi)
    front = (i > 0) & (phi > 0)
    tp = np.concatenate([t, t[:1] if n else np.zeros(1, np.uint8)])     # index -1 reads a byte that `front` masks
    reducible = front & (tp[i - 1] == tp[phi - 1])
    is_long = ~reducible & (plcp >= cap) & (lim > cap)
    return np.sort(plcp[is_long & (plcp < lim)]), np.sort(plcp[is_long & (plcp == lim)])
