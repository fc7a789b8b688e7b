"""The k-mers of a text -- list, abundance spectrum, all-k profile -- against collections.Counter over the text
(tests/kmer_ref.py; tests/test_kmer_ref.py holds it to the boundary definition).  Everything is compared exactly, through
the host, the _dev and the _esa_dev entries, on the smallest shapes at which the kernels can go wrong: texts of at most
3 KM_TILE + 5 bytes, one group over more than three tiles with boundaries in the first and last rows of a tile, groups that
straddle every tile edge, k on both sides of log_sigma n, filters that cut none, some and all, the capacity and error
protocol, and arrays that are no enhanced suffix array.  The lists are checked without trusting the library's order: the
(k-mer, occ) pairs are the sorted Counter items, sa[row] = pos, the row intervals do not overlap, and sa[row : row + occ]
holds the k-mer's occurrences."""
import collections
import ctypes as C

import numpy as np
import pytest

import kmer_ref as K

pytestmark = pytest.mark.gpu

KM_TILE = 4096      # rows per tile of the passes: csrc/tc_kmer.hpp (tests/test_kmer_ref.py keeps the two equal)
TC_ERR_ARG, TC_ERR_CAPACITY = -1, -2
TC_MAX_N = 0x7ffffff0
KBIG = 2 ** 32 - 1
FILTERS = [(1, 0), (1, 1), (2, 0), (3, 5)]


@pytest.fixture(scope="module")
def ctx():
    import textcomp
    c = textcomp.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ helpers
_OCCS, _DEV = {}, {}


def _occs(t, k):
    """{k-mer: its positions, increasing}, computed once"""
    key = (t, k)
    if key not in _OCCS:
        d = collections.defaultdict(list)
        if 1 <= k <= len(t):
            for i in range(len(t) - k + 1):
                d[t[i:i + k]].append(i)
        _OCCS[key] = d
    return _OCCS[key]


def _want(t, k, mn, mx):
    return [(w, len(ps)) for w, ps in sorted(_occs(t, k).items()) if K.keep(len(ps), mn, mx)]


def _np32(x):
    return x.cpu().numpy().view(np.uint32)


def _dev(ctx, t):
    """(d_text, d_sa, d_lcp) of a text, built once"""
    import torch
    if t not in _DEV:
        d_text = torch.from_numpy(np.frombuffer(t, np.uint8).copy()).cuda()
        d_sa = ctx.suffix_array_dev(d_text)
        _DEV[t] = (d_text, d_sa, ctx.lcp_array_dev(d_text, d_sa))
    return _DEV[t]


def _check_list(t, k, mn, mx, pos, occ, row, sa, what):
    n = len(t)
    assert pos.dtype == occ.dtype == row.dtype == np.uint32 and len(pos) == len(occ) == len(row), what
    got = [(t[p:p + k], o) for p, o in zip(pos.tolist(), occ.tolist())]
    assert got == _want(t, k, mn, mx), what
    assert len(sa) == n + 1 and sorted(sa.tolist()) == list(range(n + 1)), what
    assert np.array_equal(sa[row], pos), what
    assert (row[1:].astype(np.int64) >= row[:-1].astype(np.int64) + occ[:-1]).all(), what
    occs = _occs(t, k)
    for p, o, r in zip(pos.tolist(), occ.tolist(), row.tolist()):
        assert sorted(sa[r:r + o].tolist()) == occs[t[p:p + k]], (what, p, o, r)


def _every_way(ctx, t, k, filters=FILTERS, what=""):
    """the list through the three entry kinds: the same arrays, and right"""
    t = bytes(t)
    d_text, d_sa, d_lcp = _dev(ctx, t)
    for mn, mx in filters:
        tag = "%s n=%d k=%d filters=(%d, %d)" % (what, len(t), k, mn, mx)
        pos, occ, row, sa = ctx.kmers(t, k, mn, mx, with_sa=True)
        _check_list(t, k, mn, mx, pos, occ, row, sa, tag + " host")
        assert ctx.kmer_count(t, k, mn, mx) == len(pos), tag
        dev = ctx.kmers_dev(d_text, k, mn, mx, with_sa=True)
        esa = ctx.kmers_esa_dev(d_sa, d_lcp, k, mn, mx)
        for name, h, d, e in zip(("pos", "occ", "row"), (pos, occ, row), dev, esa):
            assert np.array_equal(_np32(d), h), (tag, "dev", name)
            assert np.array_equal(_np32(e), h), (tag, "esa_dev", name)
        assert np.array_equal(_np32(dev[3]), sa) and np.array_equal(_np32(d_sa), sa), tag


def _check_spectrum(ctx, t, k, bins):
    t = bytes(t)
    want = K.spectrum_of([len(ps) for ps in _occs(t, k).values()], bins)
    distinct, total = len(_occs(t, k)), max(0, len(t) - k + 1)
    hist, d, tot = ctx.kmer_spectrum(t, k, bins)
    assert hist.dtype == np.uint64 and hist.tolist() == want and (d, tot) == (distinct, total), (len(t), k, bins, "host")
    _, d_sa, d_lcp = _dev(ctx, t)
    d_hist, d, tot = ctx.kmer_spectrum_esa_dev(d_sa, d_lcp, k, bins)
    assert d_hist.cpu().tolist() == want and (d, tot) == (distinct, total), (len(t), k, bins, "esa_dev")


# ------------------------------------------------------------------------------------------------ the list
def test_tiny_texts(ctx):
    for t in (b"", b"a", b"aa", b"ab"):
        for k in (1, 2, 3, KBIG):
            _every_way(ctx, t, k, what=repr(t))
    pos, occ, row, sa = ctx.kmers(b"", 1, with_sa=True)
    assert len(pos) == len(occ) == len(row) == 0 and sa.tolist() == [0]
    assert ctx.kmer_spectrum(b"", 1, 4)[0].tolist() == [0, 0, 0, 0] and ctx.kmer_spectrum(b"", 1, 4)[1:] == (0, 0)
    d, u = ctx.kmer_profile(b"", 5)
    assert d.tolist() == u.tolist() == [0] * 5


def test_worked_examples(ctx):
    for t, k, want in K.EXAMPLES:
        pos, occ, row, sa = ctx.kmers(t, k, with_sa=True)
        assert list(zip(row.tolist(), pos.tolist(), occ.tolist())) == want, (t, k)
        if t in K.EXAMPLE_ESA:
            assert sa.tolist() == K.EXAMPLE_ESA[t][0]
        _every_way(ctx, t, k, what=repr(t))
    assert [b"mississippi"[p:p + 2] for p in ctx.kmers(b"mississippi", 2)[0]] == [b"ip", b"is", b"mi", b"pi", b"pp", b"si", b"ss"]


def test_k_at_the_ends(ctx):
    t = K.random_text(1, 300, 4)
    for k in (1, len(t), len(t) + 1, KBIG):
        _every_way(ctx, t, k, what="random")
    assert ctx.kmer_count(t, len(t)) == 1 and ctx.kmer_count(t, len(t) + 1) == 0


@pytest.mark.parametrize("n", [KM_TILE - 2, KM_TILE - 1, KM_TILE, KM_TILE + 1, 3 * KM_TILE + 5])
def test_unary_one_group_over_the_tiles(ctx, n):
    """one k-mer over all rows but the first k: its group ends at the virtual row N, in the last row of a tile, the first
    row of the next, or three tiles on; no lane may walk it"""
    t = b"a" * n
    for k in (1, 2):
        _every_way(ctx, t, k, [(1, 0), (2, 0), (n + 1 - k, n + 1 - k), (n + 2 - k, 0)], "unary")
        assert ctx.kmers(t, k)[1].tolist() == [n + 1 - k]


def test_groups_straddle_every_tile_edge(ctx):
    """period 3 at k = 2: three k-mers, each a third of the rows, so a group lies across each tile edge"""
    t = K.periodic(3 * KM_TILE + 5, 3)
    _every_way(ctx, t, 2, what="period 3")
    assert len(ctx.kmers(t, 2)[0]) == 3
    _every_way(ctx, K.periodic(2 * KM_TILE + 1, 7), 5, what="period 7")


@pytest.mark.parametrize("sigma,ks", [(2, (6, 13, 20)), (4, (3, 6, 7, 10)), (256, (1, 2, 3))])
@pytest.mark.parametrize("N", [2 * KM_TILE - 1, 2 * KM_TILE + 1])
def test_random_texts_around_log_sigma_n(ctx, sigma, ks, N):
    t = K.random_text(sigma + N, N - 1, sigma)
    for k in ks:
        _every_way(ctx, t, k, what="sigma %d" % sigma)


def test_filters_cut_none_some_and_all(ctx):
    t = K.random_text(7, 1000, 2)
    n = len(t)
    for k in (1, 3, 8):
        _every_way(ctx, t, k, FILTERS + [(n, 0), (1, n), (n, n)], "filters")
    assert ctx.kmer_count(t, 3, n, 0) == 0 and ctx.kmer_count(t, 3, 1, 0) == 8
    assert 0 < ctx.kmer_count(t, 8, 3, 5) < ctx.kmer_count(t, 8, 1, 0)
    assert ctx.kmer_count(b"a" * 50, 1, 50, 0) == 1                 # min_occ = n keeps the one k-mer that has it


# ------------------------------------------------------------------------------------------------ the protocol
def _raw(ctx, t, k, mn, mx, cap, sa=False, pos=True, occ=True, row=True):
    """tc_kmers with buffers of `cap` slots filled with a canary -> (rc, nk, pos, occ, row)"""
    a = np.frombuffer(bytes(t), np.uint8)
    bufs = [np.full(max(cap, 1), 0xdeadbeef, np.uint32) for _ in range(3)]
    sa_buf = np.zeros(len(t) + 1, np.uint32)
    nk = C.c_uint64(cap)
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)
    rc = ctx.lib.tc_kmers(ctx.handle, ptr(a) if len(a) else None, len(a), k, mn, mx, ptr(sa_buf) if sa else None,
                          ptr(bufs[0]) if pos else None, ptr(bufs[1]) if occ else None, ptr(bufs[2]) if row else None, C.byref(nk))
    return (rc, int(nk.value)) + tuple(bufs)


def test_capacity_protocol(ctx):
    t = b"mississippi"
    rc, nk, pos, occ, row = _raw(ctx, t, 2, 1, 0, 0, pos=False, occ=False, row=False)       # sizes only
    assert (rc, nk) == (0, 7)
    rc, nk, pos, occ, row = _raw(ctx, t, 2, 1, 0, 6)                                        # one slot short
    assert (rc, nk) == (TC_ERR_CAPACITY, 7)
    assert (pos == 0xdeadbeef).all() and (occ == 0xdeadbeef).all() and (row == 0xdeadbeef).all()
    rc, nk, pos, occ, row = _raw(ctx, t, 2, 1, 0, len(t))                                   # capacity n always suffices
    assert (rc, nk) == (0, 7) and pos[:7].tolist() == [7, 4, 0, 9, 8, 6, 5] and (pos[7:] == 0xdeadbeef).all()
    rc, nk, pos, occ, row = _raw(ctx, t, 2, 1, 0, 7, row=False)                             # no kmer_row, no sa
    assert (rc, nk) == (0, 7) and occ[:7].tolist() == [1, 2, 1, 1, 1, 2, 2] and (row == 0xdeadbeef).all()
    rc, nk, *_ = _raw(ctx, t, 1, 1, 0, len(t))                                              # every byte distinct at most: n slots
    assert (rc, nk) == (0, 4)
    # the device forms
    d_text, d_sa, d_lcp = _dev(ctx, t)
    for cap in (1, 7, 100):
        got = ctx.kmers_esa_dev(d_sa, d_lcp, 2, cap=cap)
        assert _np32(got[0]).tolist() == [7, 4, 0, 9, 8, 6, 5]
        got = ctx.kmers_dev(d_text, 2, cap=cap)
        assert _np32(got[2]).tolist() == [2, 3, 5, 6, 7, 8, 10]


def test_argument_errors(ctx):
    import torch
    lib, h = ctx.lib, ctx.handle
    t = b"mississippi"
    for k, mn, mx in ((0, 1, 0), (2, 0, 0), (2, 3, 2), (2, 2, 1)):
        assert _raw(ctx, t, k, mn, mx, 11)[0] == TC_ERR_ARG, (k, mn, mx)
    assert _raw(ctx, t, 2, 1, 0, 11, pos=False)[0] == TC_ERR_ARG
    assert _raw(ctx, t, 2, 1, 0, 11, occ=False)[0] == TC_ERR_ARG
    assert _raw(ctx, t, 2, 1, 0, 11, pos=False, occ=False)[0] == TC_ERR_ARG     # a capacity, and nowhere to write
    a = np.frombuffer(t, np.uint8)
    buf = np.zeros(16, np.uint32)
    u64s = np.zeros(16, np.uint64)
    ptr = lambda x: C.c_void_p(x.ctypes.data)
    nk = C.c_uint64(11)
    assert lib.tc_kmers(h, ptr(a), 11, 2, 1, 0, None, ptr(buf), ptr(buf), None, None) == TC_ERR_ARG             # no capacity word
    assert lib.tc_kmers(h, None, 11, 2, 1, 0, None, ptr(buf), ptr(buf), None, C.byref(nk)) == TC_ERR_ARG        # no text
    assert lib.tc_kmers(h, ptr(a), TC_MAX_N + 1, 2, 1, 0, None, None, None, None, C.byref(C.c_uint64(0))) == TC_ERR_ARG
    assert lib.tc_kmers_dev(h, None, TC_MAX_N + 1, 2, 1, 0, None, None, None, None, C.byref(C.c_uint64(0))) == TC_ERR_ARG
    d_text, d_sa, d_lcp = _dev(ctx, t)
    psa, pl = C.c_void_p(d_sa.data_ptr()), C.c_void_p(d_lcp.data_ptr())
    z = lambda: C.byref(C.c_uint64(0))
    assert lib.tc_kmers_esa_dev(h, None, pl, 12, 2, 1, 0, None, None, None, z()) == TC_ERR_ARG
    assert lib.tc_kmers_esa_dev(h, psa, None, 12, 2, 1, 0, None, None, None, z()) == TC_ERR_ARG
    assert lib.tc_kmers_esa_dev(h, psa, pl, 0, 2, 1, 0, None, None, None, z()) == TC_ERR_ARG
    assert lib.tc_kmers_esa_dev(h, psa, pl, TC_MAX_N + 2, 2, 1, 0, None, None, None, z()) == TC_ERR_ARG
    assert lib.tc_kmers_esa_dev(h, psa, pl, 12, 0, 1, 0, None, None, None, z()) == TC_ERR_ARG
    assert lib.tc_kmers_esa_dev(h, psa, pl, 12, 2, 1, 0, None, None, None, None) == TC_ERR_ARG
    assert lib.tc_kmers_esa_dev(h, psa, pl, 12, 2, 1, 0, None, None, None, z()) == 0
    d_hist = torch.zeros(8, dtype=torch.int64, device="cuda")
    ph = C.c_void_p(d_hist.data_ptr())
    d, tot = C.c_uint64(), C.c_uint64()
    for k, bins in ((0, 4), (2, 0), (2, 65537)):
        assert lib.tc_kmer_spectrum(h, ptr(a), 11, k, bins, ptr(u64s), C.byref(d), C.byref(tot)) == TC_ERR_ARG
        assert lib.tc_kmer_spectrum_esa_dev(h, psa, pl, 12, k, bins, ph, C.byref(d), C.byref(tot)) == TC_ERR_ARG
    assert lib.tc_kmer_spectrum(h, ptr(a), 11, 2, 4, None, C.byref(d), C.byref(tot)) == TC_ERR_ARG
    assert lib.tc_kmer_spectrum(h, ptr(a), 11, 2, 4, ptr(u64s), None, C.byref(tot)) == TC_ERR_ARG
    assert lib.tc_kmer_spectrum(h, ptr(a), 11, 2, 4, ptr(u64s), C.byref(d), None) == TC_ERR_ARG
    assert lib.tc_kmer_spectrum(h, None, 11, 2, 4, ptr(u64s), C.byref(d), C.byref(tot)) == TC_ERR_ARG
    assert lib.tc_kmer_spectrum(h, ptr(a), TC_MAX_N + 1, 2, 4, ptr(u64s), C.byref(d), C.byref(tot)) == TC_ERR_ARG
    assert lib.tc_kmer_spectrum_esa_dev(h, psa, pl, 12, 2, 4, None, C.byref(d), C.byref(tot)) == TC_ERR_ARG
    assert lib.tc_kmer_spectrum_esa_dev(h, None, pl, 12, 2, 4, ph, C.byref(d), C.byref(tot)) == TC_ERR_ARG
    assert lib.tc_kmer_spectrum_esa_dev(h, psa, pl, 0, 2, 4, ph, C.byref(d), C.byref(tot)) == TC_ERR_ARG
    assert lib.tc_kmer_spectrum_esa_dev(h, psa, pl, TC_MAX_N + 2, 2, 4, ph, C.byref(d), C.byref(tot)) == TC_ERR_ARG
    for kmax in (0, 4097):
        assert lib.tc_kmer_profile(h, ptr(a), 11, kmax, ptr(u64s), None) == TC_ERR_ARG
        assert lib.tc_kmer_profile_esa_dev(h, pl, 12, kmax, ptr(u64s), None) == TC_ERR_ARG
    assert lib.tc_kmer_profile(h, ptr(a), 11, 4, None, ptr(u64s)) == TC_ERR_ARG
    assert lib.tc_kmer_profile(h, None, 11, 4, ptr(u64s), None) == TC_ERR_ARG
    assert lib.tc_kmer_profile(h, ptr(a), TC_MAX_N + 1, 4, ptr(u64s), None) == TC_ERR_ARG
    assert lib.tc_kmer_profile_esa_dev(h, None, 12, 4, ptr(u64s), None) == TC_ERR_ARG
    assert lib.tc_kmer_profile_esa_dev(h, pl, 0, 4, ptr(u64s), None) == TC_ERR_ARG
    assert lib.tc_kmer_profile_esa_dev(h, pl, TC_MAX_N + 2, 4, ptr(u64s), None) == TC_ERR_ARG
    assert lib.tc_kmer_profile_esa_dev(h, pl, 12, 4, None, None) == TC_ERR_ARG
    assert ctx.kmers(t, 2)[0].tolist() == [7, 4, 0, 9, 8, 6, 5]        # the context still works


# ------------------------------------------------------------------------------------------------ spectrum and profile
@pytest.mark.parametrize("bins", [1, 2, 256, 65536])
def test_spectrum(ctx, bins):
    _check_spectrum(ctx, b"mississippi", 2, bins)
    _check_spectrum(ctx, b"mississippi", 12, bins)
    t = K.random_text(3, 2 * KM_TILE, 4)
    for k in (1, 4, 7, 12):
        _check_spectrum(ctx, t, k, bins)
    _check_spectrum(ctx, K.periodic(3 * KM_TILE + 5, 3), 2, bins)
    for k in (1, 2):            # one k-mer, above the counters kept in LDS: it adds to global memory itself
        _check_spectrum(ctx, b"a" * (KM_TILE + 904), k, bins)


_PROFILE_TEXTS = {"random": K.random_text(5, 2 * KM_TILE, 4), "unary": b"a" * (KM_TILE + 904), "period 7": K.periodic(KM_TILE + 904, 7),
                  "short": b"aaabaab"}


@pytest.mark.parametrize("kmax", [1, 7, 4096])
@pytest.mark.parametrize("name", sorted(_PROFILE_TEXTS))
def test_profile(ctx, name, kmax):
    t = _PROFILE_TEXTS[name]
    d, u = ctx.kmer_profile(t, kmax)
    assert d.dtype == u.dtype == np.uint64 and len(d) == len(u) == kmax
    for k in sorted({1, 2, 3, 5, 7, 8, 13, 64, 500, 4095, 4096} & set(range(1, kmax + 1))):       # against the Counter ...
        c = K.counter(t, k)
        assert (int(d[k - 1]), int(u[k - 1])) == (len(c), sum(1 for v in c.values() if v == 1)), (name, k)
    _, lcp = K.esa(t) if len(t) < 100 else (None, _np32(_dev(ctx, t)[2]))
    wd, wu = K.profile_by_lcp(lcp, kmax)                                   # ... and every k against the two formulas
    assert d.tolist() == wd and u.tolist() == wu, name
    d_lcp = _dev(ctx, t)[2]
    d2, u2 = ctx.kmer_profile_esa_dev(d_lcp, kmax)
    assert d2.tolist() == wd and u2.tolist() == wu, name
    d3, u3 = ctx.kmer_profile_esa_dev(d_lcp, kmax, unique=False)           # unique = NULL
    assert d3.tolist() == wd and u3 is None
    assert ctx.kmer_profile(t, kmax, unique=False)[0].tolist() == wd


# ------------------------------------------------------------------------------------------------ arrays that are no ESA
@pytest.mark.parametrize("kind", ["shuffled sa", "small lcp words", "random words", "lcp[0] != 0"])
def test_esa_dev_on_arrays_no_text_has(ctx, kind):
    """TC_OK, and what the boundary definition gives on those arrays: boundaries from the lcp values alone, sa copied and
    compared, never an index"""
    import torch
    rng = np.random.default_rng(len(kind))
    N = 2 * KM_TILE + 1
    t = K.random_text(9, N - 1, 2)
    sa = _np32(_dev(ctx, t)[1]).copy()
    lcp = _np32(_dev(ctx, t)[2]).copy()
    if kind == "shuffled sa":
        rng.shuffle(sa)
    elif kind == "small lcp words":
        lcp = rng.integers(0, 6, N).astype(np.uint32)
        sa = rng.integers(0, 2 * N, N).astype(np.uint32)
    elif kind == "random words":
        lcp = rng.integers(0, 2 ** 32, N, dtype=np.uint64).astype(np.uint32)
        sa = rng.integers(0, 2 ** 32, N, dtype=np.uint64).astype(np.uint32)
    else:
        lcp[0] = 77
    d_sa = torch.from_numpy(sa.view(np.int32)).cuda()
    d_lcp = torch.from_numpy(lcp.view(np.int32)).cuda()
    for k in (1, 2, 4, 13, 2 ** 31, KBIG):
        for mn, mx in ((1, 0), (2, 0), (3, 5)):
            row, pos, occ = K.by_esa(sa, lcp, k, mn, mx)
            got = ctx.kmers_esa_dev(d_sa, d_lcp, k, mn, mx)
            assert [_np32(g).tolist() for g in got] == [pos, occ, row], (kind, k, mn, mx)
        _, _, occ = K.by_esa(sa, lcp, k)
        for bins in (2, 65536):
            d_hist, distinct, total = ctx.kmer_spectrum_esa_dev(d_sa, d_lcp, k, bins)
            assert d_hist.cpu().tolist() == K.spectrum_of(occ, bins) and (distinct, total) == (len(occ), max(0, N - 1 - k + 1)), (kind, k, bins)
    for kmax in (7, 4096):
        d, u = ctx.kmer_profile_esa_dev(d_lcp, kmax)
        wd, wu = K.profile_by_lcp(lcp, kmax)
        assert d.tolist() == wd and u.tolist() == wu, (kind, kmax)


def test_unaligned_arrays(ctx):
    """an LCP array that does not start on a 16-byte boundary is read word by word"""
    import torch
    t = K.random_text(11, KM_TILE + 100, 4)
    _, d_sa, d_lcp = _dev(ctx, t)
    off = torch.empty(d_lcp.numel() + 1, dtype=torch.int32, device="cuda")
    off[1:] = d_lcp
    view = off[1:]
    assert view.data_ptr() % 16 == 4
    for k in (3, 6):
        want = ctx.kmers_esa_dev(d_sa, d_lcp, k)
        got = ctx.kmers_esa_dev(d_sa, view, k)
        assert all(torch.equal(a, b) for a, b in zip(got, want))
        assert torch.equal(ctx.kmer_spectrum_esa_dev(d_sa, view, k)[0], ctx.kmer_spectrum_esa_dev(d_sa, d_lcp, k)[0])
    assert ctx.kmer_profile_esa_dev(view, 64)[0].tolist() == ctx.kmer_profile_esa_dev(d_lcp, 64)[0].tolist()


# ------------------------------------------------------------------------------------------------ contexts
def test_two_contexts_interleaved(ctx):
    import textcomp
    ta, tb = K.random_text(21, KM_TILE + 7, 4), K.periodic(2 * KM_TILE + 3, 3)
    with textcomp.Context(0) as other:
        for k in (2, 5):
            a1 = ctx.kmers(ta, k, with_sa=True)
            b1 = other.kmers(tb, k, with_sa=True)
            a2 = ctx.kmer_spectrum(ta, k, 16)
            b2 = other.kmer_profile(tb, 9)
            a3 = ctx.kmers(ta, k, 2, 0)
            _check_list(ta, k, 1, 0, *a1, "first context")
            _check_list(tb, k, 1, 0, *b1, "second context")
            assert a2[0].tolist() == K.spectrum(ta, k, 16)[0]
            assert (b2[0].tolist(), b2[1].tolist()) == K.profile(tb, 9)
            assert [(ta[p:p + k], o) for p, o in zip(a3[0].tolist(), a3[1].tolist())] == _want(ta, k, 2, 0)
