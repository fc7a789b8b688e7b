"""CPU reference of the LPF array, the LZ77 parse of a text against itself and its inverse (tc_lpf_array, tc_lz_parse,
tc_lz_unparse; include/textcomp.h has the definitions), written twice:

  brute(t)     straight from the definitions, for n <= 256: lpf[i] = the maximum of lcp(i, j) over all j < i; src[i] by
               the neighbour rule -- the suffixes that start before i sorted directly, suffix i's two neighbours among
               them, the one with the longer shared prefix, on a tie the smaller one;
  by_esa(t)    the suffix-array restatement for larger texts: a naive sort (prefix doubling in numpy), the LCP array by
               Kasai's loop, the nearest rows above and below with sa < i by a stack, the minimum of lcp over the rows
               between from a sparse table.

tests/test_lz_ref.py checks that the two agree and that the neighbour rule attains the maximum.  Python compares bytes
the way the suffix array does: a proper prefix -- the end of the text -- sorts first."""
import numpy as np


def _lcp(t, i, j):
    n, l = len(t), 0
    while i + l < n and j + l < n and t[i + l] == t[j + l]:
        l += 1
    return l


def brute(t):
    """-> (lpf, src, best): best[i] = max over j < i of lcp(i, j), by trying every j; lpf / src by the neighbour rule"""
    t = bytes(t)
    n = len(t)
    assert n <= 256
    lpf, src, best = [0] * n, [0] * n, [0] * n
    for i in range(n):
        best[i] = max([_lcp(t, i, j) for j in range(i)], default=0)
        me = t[i:]
        smaller = [j for j in range(i) if t[j:] < me]
        larger = [j for j in range(i) if t[j:] > me]
        lo = max(smaller, key=lambda j: t[j:]) if smaller else None
        hi = min(larger, key=lambda j: t[j:]) if larger else None
        llo = _lcp(t, i, lo) if lo is not None else 0
        lhi = _lcp(t, i, hi) if hi is not None else 0
        if llo >= lhi:
            lpf[i], src[i] = llo, (lo if llo else 0)
        else:
            lpf[i], src[i] = lhi, hi
    return lpf, src, best


def suffix_array(t):
    """the n + 1 suffixes of t in order, the empty one first, by prefix doubling"""
    a = np.frombuffer(bytes(t), np.uint8).astype(np.int64) + 1
    n = len(a)
    rank = np.concatenate([a, [0]])
    N = n + 1
    k = 1
    while True:
        second = np.zeros(N, np.int64)
        if k < N:
            second[:N - k] = rank[k:]
        order = np.lexsort((second, rank))
        key = rank[order] * (max(N, 257) + 2) + second[order]   # (ranks are byte values + 1 in the first round, < N later)
        new = np.empty(N, np.int64)
        new[order] = np.concatenate([[0], np.cumsum(key[1:] != key[:-1])])
        rank = new
        if int(rank.max()) == N - 1:
            return order.astype(np.int64)
        k *= 2


def lcp_array(t, sa):
    """Kasai: lcp[0] = 0, lcp[j] = the longest common prefix of the suffixes at sa[j - 1] and sa[j]"""
    t = bytes(t)
    n = len(t)
    N = n + 1
    isa = np.empty(N, np.int64)
    isa[sa] = np.arange(N)
    sa_l, isa_l = sa.tolist(), isa.tolist()
    lcp = [0] * N
    h = 0
    for i in range(n):
        r = isa_l[i]
        j = sa_l[r - 1]         # (r >= 1: row 0 is the empty suffix)
        while i + h < n and j + h < n and t[i + h] == t[j + h]:
            h += 1
        lcp[r] = h
        if h:
            h -= 1
    return lcp


def by_esa(t):
    """-> (lpf, src) as lists, from the suffix array, the LCP array, nearest smaller rows and range minima"""
    t = bytes(t)
    n = len(t)
    if n == 0:
        return [], []
    N = n + 1
    sa = suffix_array(t)
    lcp = np.array(lcp_array(t, sa), np.int64)
    sa_l = sa.tolist()
    prev, nxt = [-1] * N, [N] * N       # nearest rows above / below with a smaller sa
    stack = []
    for r in range(N):
        while stack and sa_l[stack[-1]] > sa_l[r]:
            stack.pop()
        prev[r] = stack[-1] if stack else -1
        stack.append(r)
    stack = []
    for r in range(N - 1, -1, -1):
        while stack and sa_l[stack[-1]] > sa_l[r]:
            stack.pop()
        nxt[r] = stack[-1] if stack else N
        stack.append(r)
    table = [lcp]                       # table[k][j] = min lcp[j .. j + 2^k)
    k = 1
    while 2 * k <= N:
        p = table[-1]
        table.append(np.minimum(p[:len(p) - k], p[k:]))
        k *= 2

    def range_min(lo, hi):              # min lcp[lo .. hi], lo <= hi
        k = (hi - lo + 1).bit_length() - 1
        return int(min(table[k][lo], table[k][hi - (1 << k) + 1]))

    lpf, src = [0] * n, [0] * n
    for r in range(1, N):
        i = sa_l[r]
        p, q = prev[r], nxt[r]
        lp = range_min(p + 1, r) if p >= 0 else 0
        lq = range_min(r + 1, q) if q < N else 0
        if lp >= lq:
            lpf[i], src[i] = lp, (sa_l[p] if lp else 0)
        else:
            lpf[i], src[i] = lq, sa_l[q]
    return lpf, src


def lpf_src(t):
    """(lpf, src) as uint32 arrays: brute force where it is affordable, the suffix-array restatement otherwise"""
    lpf, src = brute(t)[:2] if len(t) <= 64 else by_esa(t)
    return np.array(lpf, np.uint32), np.array(src, np.uint32)


def parse_of(t, lpf, src):
    """the greedy parse from the two arrays -> (ph_src, ph_len) as uint32 arrays"""
    t = bytes(t)
    ps, pl, i = [], [], 0
    while i < len(t):
        if lpf[i] == 0:
            ps.append(t[i])
            pl.append(0)
            i += 1
        else:
            ps.append(int(src[i]))
            pl.append(int(lpf[i]))
            i += int(lpf[i])
    return np.array(ps, np.uint32), np.array(pl, np.uint32)


def parse(t):
    return parse_of(t, *lpf_src(t))


def valid(ph_src, ph_len):
    """is the list one tc_lz_unparse accepts (the total's bound aside)"""
    s = 0
    for a, l in zip(ph_src, ph_len):
        a, l = int(a), int(l)
        if (a >= s) if l else (a > 255):
            return False
        s += max(l, 1)
    return True


def unparse(ph_src, ph_len):
    """phrases back to bytes, one byte after the other"""
    out = bytearray()
    for a, l in zip(ph_src, ph_len):
        a, l = int(a), int(l)
        if l == 0:
            out.append(a)
        else:
            assert a < len(out)
            for k in range(l):
                out.append(out[a + k])
    return bytes(out)


# ---- the texts of the tests
def fibonacci(n, a=b"a", b=b"b"):
    x, y = b, a
    while len(y) < n:
        x, y = y, y + x
    return y[:n]


def periodic(n, p):
    return (bytes(b"abcdefg"[:p]) * (n // p + 1))[:n]


def random_text(seed, n, sigma):
    rng = np.random.default_rng(seed)
    if sigma == 256:
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    return np.frombuffer(b"acgt"[:sigma], np.uint8)[rng.integers(0, sigma, n)].tobytes()
