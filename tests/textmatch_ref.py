"""CPU reference of the comparison of two texts (tc_text_match_stats, tc_text_mems, tc_text_lcs; include/textcomp.h has the
definitions), written twice:

  brute(q, t)    straight from the definitions, by bytes.find and counting: ms_len[i] = the longest prefix of q[i:] that
                 occurs in t, ms_pos[i] = the start of the smallest suffix of t with that prefix, ms_occ[i] = its
                 occurrences, overlapping ones included;
  by_esa(q, t)   the definitions on a naive enhanced suffix array of q + t (tests/lz_ref.py: prefix doubling, Kasai): the
                 nearest T rows above and below a Q row, the minimum of lcp over the rows between, the clamp to q's end,
                 then the LCP interval at that depth and the T rows in it.

tests/test_textmatch_ref.py holds the two to each other.  Python compares bytes the way the suffix array does: a proper
prefix -- the end of the text -- sorts first."""
import numpy as np

import lz_ref


def brute(q, t):
    """-> (ms_len, ms_pos, ms_occ) as lists"""
    q, t = bytes(q), bytes(t)
    a = len(q)
    ms_len, ms_pos, ms_occ = [0] * a, [0] * a, [0] * a
    for i in range(a):
        l = 0
        while i + l < a and t.find(q[i:i + l + 1]) >= 0:
            l += 1
        if l == 0:
            continue
        w, occ, j = q[i:i + l], [], t.find(q[i:i + l])
        while j >= 0:
            occ.append(j)
            j = t.find(w, j + 1)
        ms_len[i], ms_occ[i] = l, len(occ)
        ms_pos[i] = min(occ, key=lambda j: t[j:])
    return ms_len, ms_pos, ms_occ


def by_esa(q, t):
    """-> (ms_len, ms_pos, ms_occ) as lists, from the enhanced suffix array of q + t"""
    q, t = bytes(q), bytes(t)
    a, b = len(q), len(t)
    ms_len, ms_pos, ms_occ = [0] * a, [0] * a, [0] * a
    if a == 0 or b == 0:
        return ms_len, ms_pos, ms_occ
    x = q + t
    n = a + b
    N = n + 1
    sa = lz_ref.suffix_array(x)
    lcp = np.array(lz_ref.lcp_array(x, sa), np.int64)
    is_t = (sa >= a) & (sa < n)
    cnt = np.concatenate([[0], np.cumsum(is_t)])            # cnt[r] = the T rows below r, r in 0 .. N
    trow = np.nonzero(is_t)[0]
    sa_l = sa.tolist()
    for r in range(1, N):
        i = sa_l[r]
        if i >= a:
            continue
        c = int(cnt[r])
        m = 0
        if c >= 1:
            m = int(lcp[trow[c - 1] + 1:r + 1].min())
        if c < b:
            m = max(m, int(lcp[r + 1:trow[c] + 1].min()))
        l = min(m, a - i)                                   # the clamp: the match may run over q's end into t's head
        if l == 0:
            continue
        lo = int(np.nonzero(lcp[:r + 1] < l)[0][-1])        # the largest row <= r with lcp < l
        after = np.nonzero(lcp[r + 1:] < l)[0]
        hi1 = r + 1 + int(after[0]) if len(after) else N    # the smallest row > r with lcp < l, or N
        ms_len[i] = l
        ms_occ[i] = int(cnt[hi1] - cnt[lo])
        ms_pos[i] = sa_l[int(trow[int(cnt[lo])])] - a
    return ms_len, ms_pos, ms_occ


def stats(q, t):
    """(ms_len, ms_pos, ms_occ) as uint32 arrays: brute force where it is affordable, the suffix-array restatement
    otherwise"""
    out = brute(q, t) if len(q) * max(len(t), 1) <= 4096 else by_esa(q, t)
    return tuple(np.array(v, np.uint32) for v in out)


def mems_of(ms_len, ms_pos, min_len):
    """the rule of tc_text_mems on any two arrays (compared as unsigned 32-bit words) -> (start, pos, len) as uint32 arrays"""
    ln = np.asarray(ms_len).astype(np.uint32)
    ps = np.asarray(ms_pos).astype(np.uint32)
    if len(ln) == 0:
        return tuple(np.empty(0, np.uint32) for _ in range(3))
    prev = np.concatenate([[0], ln[:-1]]).astype(np.uint32)
    keep = (ln >= np.uint32(min_len)) & (prev <= ln)        # (prev = 0 at i = 0: always <=)
    start = np.nonzero(keep)[0].astype(np.uint32)
    return start, ps[keep], ln[keep]


def lcs_of(ms_len, ms_pos):
    """-> (len, qpos, tpos, sum)"""
    ln = [int(v) for v in ms_len]
    best = max(ln, default=0)
    if best == 0:
        return 0, 0, 0, 0
    at = ln.index(best)
    return best, at, int(ms_pos[at]), sum(ln)


# the three pairs of include/textcomp.h: (q, t, ms_len, ms_pos, ms_occ, the MEMs at min_len 1)
EXAMPLES = [
    (b"banana", b"ananas", [0, 5, 4, 3, 2, 1], [0, 0, 1, 0, 1, 0], [0, 1, 1, 2, 2, 3], [(1, 0, 5)]),
    (b"ab", b"abab", [2, 1], [2, 3], [2, 2], [(0, 2, 2)]),
    (b"aaaaa", b"aaa", [3, 3, 3, 2, 1], [0, 0, 0, 1, 2], [1, 1, 1, 2, 3], [(0, 0, 3), (1, 0, 3), (2, 0, 3)]),
]


def random_text(seed, n, sigma):
    return lz_ref.random_text(seed, n, sigma)
