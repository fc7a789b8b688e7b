"""CPU reference of the minimal absent words of a text (tc_absent_words; include/textcomp.h has the definitions), written
twice:

  brute(t)            straight from the definition, for short texts: every word x = u . b, u an occurring substring and b a byte of
                      the text, that does not occur while x without its first byte does (x without its last byte is u);
  absent_words(t ..)  the row rule: a naive sort and Kasai's loop (tests/lz_ref.py), then one lane per row k >= 1 with l = lcp[k]:
                      lb / rb / q / the representative test are the previous / next smaller (or smaller-or-equal) values of the LCP
                      array, found for all rows at once by monotonic stacks, the left-byte sets of a row range come from prefix
                      counts per byte, and the words come out in the order include/textcomp.h documents: increasing k, the first
                      child's words before the k-child's, increasing left byte inside a child.

tests/test_maw_ref.py holds the two together.  No oracle is involved: the reference has no such operation."""
import numpy as np

import lz_ref
import rep_ref


def _prev_below(v, strict):
    """p[k] = the last row j < k with v[j] < v[k] (strict) or v[j] <= v[k]; row 0 (v[0] = 0) ends every search"""
    N = len(v)
    p = [0] * N
    st = []
    for k in range(N):
        x = v[k]
        if strict:
            while st and v[st[-1]] >= x:
                st.pop()
        else:
            while st and v[st[-1]] > x:
                st.pop()
        p[k] = st[-1] if st else 0
        st.append(k)
    return p


def _next_below(v, strict):
    """q[k] = the first row j > k with v[j] < v[k] (strict) or v[j] <= v[k], N when there is none"""
    N = len(v)
    q = [N] * N
    st = []
    for k in range(N - 1, -1, -1):
        x = v[k]
        if strict:
            while st and v[st[-1]] >= x:
                st.pop()
        else:
            while st and v[st[-1]] > x:
                st.pop()
        q[k] = st[-1] if st else N
        st.append(k)
    return q


def absent_words(t, min_len=2, max_len=0):
    """-> (left uint8, pos uint32, len uint32), in the order tc_absent_words writes them"""
    t = bytes(t)
    n = len(t)
    assert min_len >= 2 and (max_len == 0 or max_len >= min_len)
    out_a, out_p, out_l = [], [], []
    if n >= 1:
        sa, lcp, left = rep_ref.esa(t)
        N = n + 1
        left = left.copy()
        left[0] = t[n - 1]                          # row 0, the empty suffix: the text's last byte stands before it
        alpha = sorted(set(t))
        col = {b: i for i, b in enumerate(alpha)}
        onehot = np.zeros((N + 1, len(alpha)), np.int32)
        rows = np.nonzero(left >= 0)[0]
        onehot[rows + 1, [col[int(b)] for b in left[rows]]] = 1
        pref = np.cumsum(onehot, axis=0)            # pref[r] = the left bytes of the rows below r, counted
        abytes = np.array(alpha, np.int64)

        def lset(lo, hi):                           # the set of left bytes of the rows lo .. hi, as a boolean row
            return (pref[hi + 1] - pref[lo]) > 0

        v = lcp.tolist()
        v[0] = 0
        psv, pse = _prev_below(v, True), _prev_below(v, False)
        nsv, nse = _next_below(v, True), _next_below(v, False)
        sal = sa.tolist()
        for k in range(1, N):
            l = v[k]
            if l + 2 < min_len or (max_len and l + 2 > max_len):
                continue
            if l == 0:
                lb, rb = 0, N - 1
            else:
                lb, rb = psv[k], nsv[k] - 1
            q = nse[k]
            lw = lset(lb, rb)
            kids = []
            if pse[k] == lb and sal[lb] + l < n:
                kids.append((lb, k - 1))
            kids.append((k, q - 1))
            for cl, cr in kids:
                for a in abytes[lw & ~lset(cl, cr)].tolist():
                    out_a.append(a)
                    out_p.append(sal[cl])
                    out_l.append(l + 2)
    return np.array(out_a, np.uint8), np.array(out_p, np.uint32), np.array(out_l, np.uint32)


def words(t, left, pos, ln):
    """the words as bytes, in list order: the byte left, then text[pos .. pos + len - 1)"""
    t = bytes(t)
    out = []
    for a, p, l in zip(np.asarray(left).tolist(), np.asarray(pos).tolist(), np.asarray(ln).tolist()):
        w = bytes([a]) + t[p:p + l - 1]
        assert len(w) == l, (a, p, l)
        out.append(w)
    return out


def profile(t, kmax):
    """-> (hist of kmax + 1 entries indexed by word length, total over every length)"""
    _, _, ln = absent_words(t)
    hist = np.bincount(ln[ln <= kmax].astype(np.int64), minlength=kmax + 1).astype(np.uint64)
    return hist, len(ln)


def brute(t):
    """the set of minimal absent words, from the definition"""
    t = bytes(t)
    n = len(t)
    subs = {t[i:j] for i in range(n) for j in range(i + 1, n + 1)}
    alpha = sorted(set(t))
    out = set()
    for u in subs:
        for b in alpha:
            x = u + bytes([b])
            if x not in subs and x[1:] in subs:
                out.add(x)
    return out


# ---- the texts of the tests
fibonacci, periodic, random_text = lz_ref.fibonacci, lz_ref.periodic, lz_ref.random_text


def all_bytes():
    """each of the 256 byte values once, in a fixed scrambled order: 65 536 - 255 = 65 281 words of length 2 and nothing longer"""
    return bytes(np.random.default_rng(0x3a7).permutation(256).astype(np.uint8))
