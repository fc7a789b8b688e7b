"""Document collections on the kept enhanced suffix array (tc_esa_build_docs, tc_esa_doc_count, tc_esa_doc_list, tc_esa_kmer_docs,
tc_esa_kmer_doc_spectrum) against the
reference of tests/esa_docs_ref.py (numpy; tests/test_esa_docs_ref.py holds it to loops over the bytes).  Everything is compared
exactly.  Every batch goes through the host entry of the C ABI, through ESAHandle's host methods and through its _dev methods, on the
smallest shapes at which the kernels can go wrong: texts of 0, 1 and 2 bytes; 1, 2, 255, 256, 257 documents (the one-pass / two-pass
edge of the build's sort) and 65535 documents of 0 to 5 bytes; empty documents at both ends; row counts one below, at and one above
one and two tiles of the sort (ESD_TILE = 4096 rows); every substring of 120-byte texts of six shapes in 1, 3 and 40 documents at
limits 0, 1 and 2; batches on both sides of one workgroup of queries; a fan-out-4 tree of eight levels; the document frequency of
the k-mers and its histogram at k = 1, 2, 3, 8, 21 on unary, period-7 and random text over more than two tiles of the k-mer passes,
with and without a df filter, equal to tc_kmers_esa_dev in set, order, pos, occ and row; the capacity protocols; each
combination of NULL outputs; a plain handle refused; the older queries on a handle with documents; two contexts on one handle; the
error protocol; and one text of 300 001 bytes in 300 documents."""
import ctypes as C
import functools

import numpy as np
import pytest

import esa_docs_ref as R
import test_gpu_esa as E
from test_gpu_esa import _dbg, _dev, _np, _p, _same, _shape, _text, _u32

pytestmark = pytest.mark.gpu

TC_ERR_ARG, TC_ERR_CAPACITY = -1, -2
ESD_TILE = 4096
LIMITS = (0, 1, 2)


@pytest.fixture(scope="module")
def ctx():
    import textcomp
    c = textcomp.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _ref_of(t, ds):
    return R.DocRef(t, np.array(ds, np.int64))


def _ref(t, ds):
    return _ref_of(t, tuple(int(x) for x in ds))


def _split(n, ndocs, seed):
    """ndocs documents over n bytes: equal sizes, every inner boundary moved by -1, 0 or 1 (so some documents are empty)"""
    ds = R.split_evenly(n, ndocs)
    if ndocs > 1:
        ds[1:-1] += np.random.default_rng(seed).integers(-1, 2, ndocs - 1)
    return np.clip(np.maximum.accumulate(ds), 0, n)


def _dptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def _docs(ctx, h, ref, s, l, limits=LIMITS, what=""):
    """one batch of substrings through count and list, in the three forms, at every limit"""
    import torch
    s, l = _u32(s), _u32(l)
    nq = len(s)
    d_s, d_l = _dev(s), _dev(l)
    lib, cx = ctx.lib, ctx.handle
    first = None
    for limit in limits:
        tag = "%s docs n=%d ndocs=%d nq=%d limit=%d" % (what, ref.n, ref.ndocs, nq, limit)
        wdf, wocc = ref.count(s, l, limit)
        woffs, wdocs, whits = ref.list(s, l, limit)
        first = wdf if first is None else first
        # ---- count
        df, occ = np.full(nq, 0xabababab, np.uint32), np.full(nq, 0xabababab, np.uint32)
        assert lib.tc_esa_doc_count(cx, h._h, _p(s), _p(l), nq, limit, _p(df), _p(occ)) == 0, tag
        _same(df, wdf, tag + " abi df")
        _same(occ, wocc, tag + " abi occ")
        _same(h.doc_count(s, l, limit, ctx=ctx), wdf, tag + " host df, no occ")
        got = h.doc_count(s, l, limit, occ=True, ctx=ctx)
        _same(got[0], wdf, tag + " host df")
        _same(got[1], wocc, tag + " host occ")
        _same(h.doc_count_dev(d_s, d_l, limit, ctx=ctx), wdf, tag + " dev df, no occ")
        got = h.doc_count_dev(d_s, d_l, limit, occ=True, ctx=ctx)
        _same(got[0], wdf, tag + " dev df")
        _same(got[1], wocc, tag + " dev occ")
        # ---- list: sizes first, then the exact capacity
        total = int(woffs[-1])
        offs = np.full(nq + 1, 0xabababab, np.uint64)
        cap = C.c_uint64(0)
        rc = lib.tc_esa_doc_list(cx, h._h, _p(s), _p(l), nq, limit, _p(offs), None, None, C.byref(cap))
        assert rc == (TC_ERR_CAPACITY if total else 0) and cap.value == total, tag
        docs, hits = np.full(total, 0xabababab, np.uint32), np.full(total, 0xabababab, np.uint32)
        assert lib.tc_esa_doc_list(cx, h._h, _p(s), _p(l), nq, limit, _p(offs), _p(docs), _p(hits), C.byref(cap)) == 0 and cap.value == total, tag
        _same(offs, woffs, tag + " abi list_offs")
        _same(docs, wdocs, tag + " abi docs")
        _same(hits, whits, tag + " abi hit_pos")
        got = h.doc_list(s, l, limit, hit_pos=True, ctx=ctx)
        for g, w, name in zip(got, (woffs, wdocs, whits), ("list_offs", "docs", "hit_pos")):
            _same(g, w, tag + " host " + name)
        _same(h.doc_list(s, l, limit, ctx=ctx)[1], wdocs, tag + " host docs, no hit_pos")
        got = h.doc_list_dev(d_s, d_l, limit, hit_pos=True, ctx=ctx)
        assert got[0].dtype == torch.int64
        _same(got[0].cpu().numpy().astype(np.uint64), woffs, tag + " dev list_offs")
        _same(got[1], wdocs, tag + " dev docs")
        _same(got[2], whits, tag + " dev hit_pos")
        _same(h.doc_list_dev(d_s, d_l, limit, ctx=ctx)[1], wdocs, tag + " dev docs, no hit_pos")
    return first                                        # df at the first of the limits


def _all_substrings(n):
    s = np.concatenate([np.full(n - i + 1, i) for i in range(n + 1)])
    l = np.concatenate([np.arange(n - i + 1) for i in range(n + 1)])
    return s, l


def _check_arrays(h, ref, what=""):
    _same(h.read("da"), ref.da.astype(np.uint32), what + " da")
    _same(h.read("pv"), ref.pv.astype(np.uint32), what + " pv")
    _same(h.read("doc_start"), ref.doc_start.astype(np.uint32), what + " doc_start")
    assert h.ndocs == ref.ndocs


def _kmer_docs(ctx, h, ref, k, filters=((1, 0),), what=""):
    """the document frequency of the k-mers through the three forms, at every filter, and its histogram"""
    import torch
    lib, cx = ctx.lib, ctx.handle
    tag = "%s kmer_docs n=%d ndocs=%d k=%d" % (what, ref.n, ref.ndocs, k)
    want = ref.kmer_docs(k)
    plain = h.kmers(k, ctx=ctx)                             # no df filter: the k-mers of tc_kmers_esa_dev, in set, order, pos, occ, row
    for g, w, name in zip(plain, (want[0], want[1], want[3]), ("pos", "occ", "row")):
        _same(g, w, tag + " kmers " + name)
    for lo, hi in filters:
        want = ref.kmer_docs(k, lo, hi)
        need = len(want[0])
        ftag = tag + " df %d..%d" % (lo, hi)
        nk = C.c_uint64(0)
        assert lib.tc_esa_kmer_docs(cx, h._h, k, lo, hi, None, None, None, None, C.byref(nk)) == 0 and nk.value == need, ftag
        assert h.kmer_doc_count(k, lo, hi, ctx=ctx) == need, ftag
        out = [np.full(need + 3, 0xabababab, np.uint32) for _ in range(4)]
        nk = C.c_uint64(need)
        assert lib.tc_esa_kmer_docs(cx, h._h, k, lo, hi, *(_p(o) for o in out), C.byref(nk)) == 0 and nk.value == need, ftag
        host, dev = h.kmer_docs(k, lo, hi, ctx=ctx), h.kmer_docs_dev(k, lo, hi, ctx=ctx)
        for i, name in enumerate(("pos", "occ", "df", "row")):
            _same(out[i][:need], want[i], ftag + " abi " + name)
            assert (out[i][need:] == 0xabababab).all()
            _same(host[i], want[i], ftag + " host " + name)
            _same(dev[i], want[i], ftag + " dev " + name)
        assert dev[0].dtype == torch.int32
    whist, wdistinct = ref.kmer_doc_spectrum(k)
    hist, distinct = h.kmer_doc_spectrum(k, ctx=ctx)
    _same(hist, whist, tag + " spectrum")
    d_hist, d_distinct = h.kmer_doc_spectrum_dev(k, ctx=ctx)
    _same(d_hist.cpu().numpy().astype(np.uint64), whist, tag + " spectrum, dev")
    assert distinct == d_distinct == wdistinct == int(hist.sum()) and hist[0] == 0
    return want


def _collection(ctx, t, ds, nq, seed, limits=LIMITS, what=""):
    ref = _ref(t, ds)
    with ctx.esa_build_docs(t, ds) as h:
        _check_arrays(h, ref, what)
        _, (s, l), _ = E._sampled(t, nq, seed)
        _docs(ctx, h, ref, s, l, limits=limits, what=what)
        _kmer_docs(ctx, h, ref, 3, ((1, 0), (2, 0)), what=what)


# ------------------------------------------------------------------------------------------------ the cases
def test_tiny_texts_and_the_worked_example(ctx):
    import textcomp
    for t in (b"", b"a", b"ab", b"aa"):
        n = len(t)
        for ds in ([0, n], [0, 0, n], [0, n, n], [0, n // 2, n], [0, 0, n // 2, n, n]):
            ref = _ref(t, ds)
            with ctx.esa_build_docs(t, ds) as h:
                assert (h.n, h.ndocs) == (n, len(ds) - 1)
                _check_arrays(h, ref, "tiny")
                _docs(ctx, h, ref, *_all_substrings(n), what="tiny")
    text, ds = textcomp.concat_docs([b"banana", b"bandana", b"ananas"])
    assert text.tobytes() == b"bananabandanaananas" and ds.tolist() == [0, 6, 13, 19] and ds.dtype == np.uint32
    with ctx.esa_build_docs(text, ds) as h:
        offs, docs, hits = h.doc_list([1, 0, 2, 9, 3, 0], [3, 3, 3, 1, 4, 0], hit_pos=True)
        assert [docs[int(a):int(b)].tolist() for a, b in zip(offs[:-1], offs[1:])] == [[1, 0, 2], [0, 1], [0, 2], [1], [0], [1, 0, 2]]
        assert hits[:3].tolist() == [10, 3, 13]
        df, occ = h.doc_count([1, 0, 2, 9, 3], [3, 3, 3, 1, 4], occ=True)
        assert df.tolist() == [3, 2, 2, 1, 1] and occ.tolist() == [5, 2, 2, 1, 1]
        assert h.doc_count([1, 0, 9], [3, 3, 1], limit=2).tolist() == [2, 2, 1]
        assert h.read("da")[0] == 0xffffffff and h.read("pv")[0] == 0xffffffff
        hist, distinct = h.kmer_doc_spectrum(3)
        assert hist.tolist() == [0, 8, 2, 1] and distinct == 11
        pos, occ, df, row = h.kmer_docs(3, 2)
        assert [(text.tobytes()[p:p + 3], o, d) for p, o, d in zip(pos.tolist(), occ.tolist(), df.tolist())] == [(b"ana", 5, 3), (b"ban", 2, 2), (b"nan", 2, 2)]


@pytest.mark.parametrize("ndocs", (1, 2, 255, 256, 257))
def test_document_counts_around_one_pass_of_the_sort(ctx, ndocs):
    t = _text(0xD0C + ndocs, 2500, 4) + (b"abc" * 200) + b"a" * 300
    _collection(ctx, t, _split(len(t), ndocs, ndocs), 700, ndocs, what="ndocs %d" % ndocs)


def test_65535_documents_of_0_to_5_bytes(ctx):
    import torch
    t = _text(0xFFFF, 150000, 4)
    ds = _split(len(t), 65535, 5)
    sizes = np.diff(ds)
    assert sizes.min() == 0 and sizes.max() <= 5
    ref = _ref(t, ds)
    d_text = torch.from_numpy(np.frombuffer(t, np.uint8).copy()).cuda()
    with ctx.esa_build_docs_dev(d_text, ds) as h:          # (the table of doc_start no longer fits in LDS)
        _check_arrays(h, ref, "65535")
        rng = np.random.default_rng(65535)
        s = rng.integers(0, len(t) - 12, 3000)
        l = rng.integers(0, 12, 3000)
        s[0], l[0] = 0, 0                                   # every non-empty document
        df = _docs(ctx, h, ref, s, l, what="65535")
        assert df[0] == (sizes > 0).sum() and df.max() > 1000
        for k in (1, 8):                                    # k = 1: document frequencies above the bins the spectrum keeps in LDS
            _kmer_docs(ctx, h, ref, k, ((1, 0), (1, 1), (5000, 0)), what="65535")
        assert ref.kmer_docs(1)[2].max() > 4096
    hh = C.c_void_p(1)
    big = np.zeros(65537, np.uint32)
    assert ctx.lib.tc_esa_build_docs(ctx.handle, None, 0, _p(big), 65536, C.byref(hh)) == TC_ERR_ARG and hh.value is None


def test_empty_documents_at_both_ends(ctx):
    t = _shape("fibonacci", 900)
    n = len(t)
    for ds in ([0, 0, 0, 300, 300, 900, 900, 900], [0, 0, n], [0, n, n], [0] * 40 + [n] * 40):
        _collection(ctx, t, ds, 400, len(ds), what="empty ends")


@pytest.mark.parametrize("rows", (ESD_TILE - 1, ESD_TILE, ESD_TILE + 1, 2 * ESD_TILE - 1, 2 * ESD_TILE, 2 * ESD_TILE + 1))
def test_row_counts_around_the_tiles_of_the_sort(ctx, rows):
    n = rows - 1
    for shape, ndocs in (("random4", 300), ("unary", 3), ("period3", 256)):
        _collection(ctx, _shape(shape, n), _split(n, ndocs, rows), 500, rows, limits=(0, 2), what="%s rows %d" % (shape, rows))


@pytest.mark.parametrize("shape", E.SHAPES)
def test_every_substring_of_a_short_text(ctx, shape):
    t = _shape(shape, 120)
    s, l = _all_substrings(len(t))
    for ndocs in (1, 3, 40):
        ds = _split(len(t), ndocs, ndocs)
        ref = _ref(t, ds)
        with ctx.esa_build_docs(t, ds) as h:
            _check_arrays(h, ref, shape)
            df = _docs(ctx, h, ref, s, l, what="%s %d docs" % (shape, ndocs))
            assert df.max() == (np.diff(ds) > 0).sum()


@pytest.mark.parametrize("nq", (1, 255, 256, 257))
def test_batch_sizes_around_a_workgroup(ctx, nq):
    t = _text(0xBA7D, 1500, 2) + b"ab" * 300 + b"a" * 200
    _collection(ctx, t, _split(len(t), 17, nq), nq, nq, limits=(0, 2), what="batch")


def test_fan_out_4_tree_of_eight_levels(ctx):
    t = _text(0xF4, 20000, 4) + (b"abc" * 7000)[:20000] + b"a" * 25537
    assert len(t) == 65537
    ds = np.array([0, 5, 10000, 19000, 30000, 30001, 45000, 60000, 65000, 65536, 65537])
    assert _dbg(ctx, "tc_dbg_fm_set_lcp_fanout", 4) == 0
    try:
        h = ctx.esa_build_docs(t, ds)
    finally:
        assert _dbg(ctx, "tc_dbg_fm_set_lcp_fanout", 64) == 0
    with h:
        ref = _ref(t, ds)
        _check_arrays(h, ref, "fan-out 4")
        assert h.device_bytes(7) == h.device_bytes(4)      # pv and its tree have the shape of lcp and its tree
        _, (s, l), _ = E._sampled(t, 2000, 4)
        _docs(ctx, h, ref, s, l, what="fan-out 4")
        rng = np.random.default_rng(44)
        i = rng.integers(40000, 65537, 1000)                # inside the unary stretch: wide intervals, first rows far apart
        _docs(ctx, h, ref, i, np.minimum(65537 - i, rng.integers(1, 30, 1000)), what="fan-out 4 wide intervals")


KM_TILE = 4096          # rows per tile of the k-mer passes (csrc/tc_kmer.hpp)


@pytest.mark.parametrize("shape", ("unary", "period7", "random4"))
def test_kmer_document_frequency(ctx, shape):
    n = 2 * KM_TILE + 700
    t = (b"abcabca" * (n // 7 + 1))[:n] if shape == "period7" else _shape(shape, n)
    for ndocs in (1, 7):
        ds = _split(n, ndocs, ndocs)
        ref = _ref(t, ds)
        with ctx.esa_build_docs(t, ds) as h:
            for k in (1, 2, 3, 8, 21):
                _kmer_docs(ctx, h, ref, k, ((1, 0), (1, 1), (ndocs, 0), (ndocs, ndocs), (2, 5), (0, 0)), what=shape)
            # k = 0 is refused, k > n gives no k-mer, max_df below min_df is refused
            nk = C.c_uint64(0)
            assert ctx.lib.tc_esa_kmer_docs(ctx.handle, h._h, 0, 1, 0, None, None, None, None, C.byref(nk)) == TC_ERR_ARG
            assert ctx.lib.tc_esa_kmer_docs_dev(ctx.handle, h._h, 3, 3, 2, None, None, None, None, C.byref(nk)) == TC_ERR_ARG
            assert h.kmer_doc_count(n + 1) == 0 and h.kmer_doc_count(n) == 1 and len(h.kmer_docs(n + 1)[0]) == 0
            hist, distinct = h.kmer_doc_spectrum(n + 1)
            assert distinct == 0 and not hist.any()
            hist = np.zeros(ndocs + 1, np.uint64)
            assert ctx.lib.tc_esa_kmer_doc_spectrum(ctx.handle, h._h, 0, _p(hist), C.byref(nk)) == TC_ERR_ARG


def test_kmer_docs_capacity_protocol_and_null_outputs(ctx):
    import torch
    t = _text(0xC0DE, 6000, 4) + b"acgt" * 300
    ds = _split(len(t), 11, 11)
    ref = _ref(t, ds)
    want = ref.kmer_docs(5, 2, 0)
    need = len(want[0])
    assert need > 10
    lib, cx = ctx.lib, ctx.handle
    with ctx.esa_build(t) as plain, ctx.esa_build_docs(t, ds) as h:
        for dev in (False, True):
            fn = lib.tc_esa_kmer_docs_dev if dev else lib.tc_esa_kmer_docs

            def arrays(k):
                return torch.full((k,), 0x2b2b2b2b, dtype=torch.int32).cuda() if dev else np.full(k, 0x2b2b2b2b, np.uint32)

            def ptr(a):
                return C.c_void_p(a.data_ptr()) if dev else _p(a)

            for cap_in in (need - 1, need, need + 5):
                for mask in (15, 1, 2, 4, 8, 5, 10):        # which of pos, occ, df, row are asked for
                    out = [arrays(cap_in) for _ in range(4)]
                    torch.cuda.synchronize()
                    nk = C.c_uint64(cap_in)
                    rc = fn(cx, h._h, 5, 2, 0, *(ptr(o) if mask >> i & 1 else None for i, o in enumerate(out)), C.byref(nk))
                    assert nk.value == need and rc == (TC_ERR_CAPACITY if cap_in < need else 0), (dev, cap_in, mask)
                    for i in range(4):
                        if cap_in >= need and mask >> i & 1:
                            _same(_np(out[i])[:need], want[i], "output %d" % i)
                            assert (_np(out[i])[need:] == 0x2b2b2b2b).all()
                        else:
                            assert (_np(out[i]) == 0x2b2b2b2b).all()
            nk = C.c_uint64(7)                              # a capacity without any array
            assert fn(cx, h._h, 5, 2, 0, None, None, None, None, C.byref(nk)) == TC_ERR_ARG
            assert fn(cx, h._h, 5, 2, 0, None, None, None, None, None) == TC_ERR_ARG
            nk = C.c_uint64(0)
            assert fn(cx, plain._h, 5, 2, 0, None, None, None, None, C.byref(nk)) == TC_ERR_ARG
        hist = np.zeros(12, np.uint64)
        nk = C.c_uint64(0)
        assert lib.tc_esa_kmer_doc_spectrum(cx, plain._h, 5, _p(hist), C.byref(nk)) == TC_ERR_ARG
        assert lib.tc_esa_kmer_doc_spectrum(cx, h._h, 5, None, C.byref(nk)) == TC_ERR_ARG
        assert lib.tc_esa_kmer_doc_spectrum(cx, h._h, 5, _p(hist), None) == TC_ERR_ARG
        assert lib.tc_esa_kmer_doc_spectrum(cx, h._h, 5, _p(hist), C.byref(nk)) == 0 and nk.value == int(hist.sum())
        a, b = h.kmer_docs_dev(5, 2), h.kmer_docs_dev(5, 2)        # two calls give identical output
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_capacity_protocol_and_null_outputs(ctx):
    import torch
    t = _shape("fibonacci", 700)
    ds = _split(len(t), 9, 9)
    ref = _ref(t, ds)
    _, (s, l), _ = E._sampled(t, 600, 9)
    s, l = _u32(s), _u32(l)
    nq = len(s)
    d_s, d_l = _dev(s), _dev(l)
    woffs, wdocs, whits = ref.list(s, l)
    wdf, wocc = ref.count(s, l)
    total = int(woffs[-1])
    lib, cx = ctx.lib, ctx.handle
    with ctx.esa_build_docs(t, ds) as h:
        for dev in (False, True):
            fn = lib.tc_esa_doc_list_dev if dev else lib.tc_esa_doc_list
            qs, ql = (_dptr(d_s), _dptr(d_l)) if dev else (_p(s), _p(l))

            def arrays(k, sentinel):
                if dev:
                    return torch.full((k,), sentinel, dtype=torch.int32).cuda()
                return np.full(k, sentinel, np.uint32)

            def ptr(a):
                return None if a is None else (C.c_void_p(a.data_ptr()) if dev else _p(a))

            offs = torch.zeros(nq + 1, dtype=torch.int64).cuda() if dev else np.zeros(nq + 1, np.uint64)
            torch.cuda.synchronize()
            for cap_in, with_hits in ((0, False), (total - 1, True), (total, True), (total, False), (total + 7, True)):
                docs, hits = arrays(max(cap_in, 1), 0x2b2b2b2b), arrays(max(cap_in, 1), 0x2b2b2b2b)
                torch.cuda.synchronize()
                cap = C.c_uint64(cap_in)
                rc = fn(cx, h._h, qs, ql, nq, 0, ptr(offs), ptr(docs) if cap_in else None, ptr(hits) if with_hits and cap_in else None, C.byref(cap))
                assert cap.value == total, (dev, cap_in)
                if cap_in < total:                          # sizes only, or one short: the total is set, nothing written
                    assert rc == TC_ERR_CAPACITY
                    assert (_np(docs) == 0x2b2b2b2b).all() and (_np(hits) == 0x2b2b2b2b).all()
                    continue
                assert rc == 0
                _same(_np(offs).astype(np.uint64), woffs, "list_offs")
                _same(_np(docs)[:total], wdocs, "docs")
                assert (_np(docs)[total:] == 0x2b2b2b2b).all()
                if with_hits:
                    _same(_np(hits)[:total], whits, "hit_pos")
                else:
                    assert (_np(hits) == 0x2b2b2b2b).all()
            # two calls give identical output
            a = h.doc_list_dev(d_s, d_l, hit_pos=True) if dev else h.doc_list(s, l, hit_pos=True)
            b = h.doc_list_dev(d_s, d_l, hit_pos=True) if dev else h.doc_list(s, l, hit_pos=True)
            assert all(np.array_equal(_np(x), _np(y)) for x, y in zip(a, b))
            # count: occ may be null, df may not
            cnt = lib.tc_esa_doc_count_dev if dev else lib.tc_esa_doc_count
            df, occ = arrays(nq, 0x2b2b2b2b), arrays(nq, 0x2b2b2b2b)
            torch.cuda.synchronize()
            assert cnt(cx, h._h, qs, ql, nq, 0, ptr(df), None) == 0
            _same(_np(df), wdf, "df alone")
            assert (_np(occ) == 0x2b2b2b2b).all()
            assert cnt(cx, h._h, qs, ql, nq, 0, None, ptr(occ)) == TC_ERR_ARG
        # nq = 0: TC_OK with nothing touched, whatever the pointers
        cap = C.c_uint64(5)
        assert lib.tc_esa_doc_count(cx, h._h, None, None, 0, 0, None, None) == 0
        assert lib.tc_esa_doc_list_dev(cx, h._h, None, None, 0, 0, None, None, None, C.byref(cap)) == 0 and cap.value == 0
        assert len(h.doc_count([], [])) == 0 and len(h.doc_list([], [])[1]) == 0


def test_host_list_stages_only_what_it_lists(ctx):
    """the host form carves the staging of its lists behind the sizes pass: on a context whose workspace is still small the second
    plan grows it, the sizes pass runs again on the new block, and a generous capacity reserves nothing"""
    import textcomp
    t = _shape("unary", 3000)
    ds = _split(len(t), 1500, 15)
    ref = _ref(t, ds)
    s, l = _u32(np.arange(400) % 7), _u32(np.zeros(400))         # len = 0: every non-empty document, 400 times
    woffs, wdocs, whits = ref.list(s, l)
    total = int(woffs[-1])
    assert total * 8 > 4 << 20                                  # more than the slack a reserve adds
    with ctx.esa_build_docs(t, ds) as h, textcomp.Context(0) as fresh:
        got = h.doc_list(s, l, hit_pos=True, ctx=fresh)
        for g, w, name in zip(got, (woffs, wdocs, whits), ("list_offs", "docs", "hit_pos")):
            _same(g, w, "fresh context " + name)
        offs = np.zeros(3, np.uint64)
        docs = np.full(8, 0xabababab, np.uint32)
        cap = C.c_uint64(1 << 40)                               # a capacity no workspace could stage: two documents are listed
        q = _u32([0, 1])
        assert fresh.lib.tc_esa_doc_list(fresh.handle, h._h, _p(q), _p(_u32([3000, 2999])), 2, 0, _p(offs), _p(docs), None, C.byref(cap)) == 0
        assert cap.value == 2 and offs.tolist() == [0, 1, 2] and (docs[2:] == 0xabababab).all()


def test_a_plain_handle_is_refused_and_a_docs_handle_answers_the_older_queries(ctx):
    import textcomp
    t = _text(0xA78, 3000, 4) + b"acgt" * 200
    n = len(t)
    ds = _split(n, 12, 12)
    good = np.zeros(4, np.uint32)
    lib, cx = ctx.lib, ctx.handle
    with ctx.esa_build(t) as plain, ctx.esa_build_docs(t, ds) as h:
        assert (plain.ndocs, h.ndocs) == (0, 12)
        cap = C.c_uint64(0)
        offs = np.zeros(5, np.uint64)
        assert lib.tc_esa_doc_count(cx, plain._h, _p(good), _p(good), 4, 0, _p(good), None) == TC_ERR_ARG
        assert lib.tc_esa_doc_list(cx, plain._h, _p(good), _p(good), 4, 0, _p(offs), None, None, C.byref(cap)) == TC_ERR_ARG
        assert lib.tc_esa_doc_arrays(plain._h, None, None, None) == TC_ERR_ARG and lib.tc_esa_doc_arrays(h._h, None, None, None) == 0
        assert lib.tc_esa_ndocs(None) == 0 and all(p for p in h.doc_arrays())
        with pytest.raises(textcomp.TcError):
            plain.doc_count([0], [1])
        for what in (5, 6, 7):
            assert lib.tc_esa_read(cx, plain._h, what, 0, 1, _p(good), 0) == TC_ERR_ARG
        assert lib.tc_esa_read(cx, h._h, 8, 0, 1, _p(good), 0) == TC_ERR_ARG
        assert lib.tc_esa_read(cx, h._h, 7, 0, 14, _p(np.zeros(16, np.uint32)), 0) == TC_ERR_ARG      # doc_start has ndocs + 1 entries
        _same(h.read_dev("doc_start", 1, 12), ds[1:].astype(np.uint32), "doc_start, dev")
        # the bytes: a plain handle as before; parts 1 .. 7 sum to part 0 on both
        pp, dp = [plain.device_bytes(p) for p in range(8)], [h.device_bytes(p) for p in range(8)]
        assert pp[0] == sum(pp[1:]) and dp[0] == sum(dp[1:]) and pp[1:6] == dp[1:6] and pp[6:] == [0, 0]
        assert dp[6] >= 4 * (n + 1) + 4 * 13 and dp[7] == dp[4] and 21 * n < dp[0] < 21.4 * n + 2048
        # every older query and analysis: the same answers as the plain handle gives
        E._all_queries(ctx, h, t, 600, 1)
        for x, y in zip(h.kmers(5, 2), plain.kmers(5, 2)):
            _same(x, _np(y), "kmers")
        for what in ("text", "sa", "isa", "lcp"):
            assert np.array_equal(h.read(what), plain.read(what))
        ref = _ref(t, ds)
        with textcomp.Context(0) as other:                  # another context on the handle's device queries it
            _, (s, l), _ = E._sampled(t, 300, 4)
            _docs(other, h, ref, s, l, limits=(0,), what="other context")
            _docs(ctx, h, ref, s, l, limits=(2,), what="first context")
            _docs(other, h, ref, s, l, limits=(1,), what="other context")


def test_errors_leave_the_handle_and_the_context_usable(ctx):
    import torch
    t = _text(0xE45, 999, 4)
    n = len(t)
    ds = _split(n, 5, 5)
    ref = _ref(t, ds)
    lib, cx = ctx.lib, ctx.handle
    with ctx.esa_build_docs(t, ds) as h:
        good = np.zeros(4, np.uint32)
        offs = np.zeros(5, np.uint64)

        def still_answers():
            _, (s, l), _ = E._sampled(t, 64, 3)
            _docs(ctx, h, ref, s, l, limits=(0,))

        for s, l in (([0, 0, n + 1, 0], [0, 0, 0, 0]), ([0, 0, 0, 0], [0, n + 1, 0, 0]), ([0, n, 0, 0], [0, 1, 0, 0]), ([5, 0, 0, 0], [0xfffffffe, 0, 0, 0])):
            s, l = _u32(s), _u32(l)
            cap = C.c_uint64(100)
            docs = np.zeros(100, np.uint32)
            assert lib.tc_esa_doc_count(cx, h._h, _p(s), _p(l), 4, 0, _p(good.copy()), None) == TC_ERR_ARG
            assert "leaves the text" in lib.tc_last_error(cx).decode()
            assert lib.tc_esa_doc_list(cx, h._h, _p(s), _p(l), 4, 0, _p(offs), _p(docs), None, C.byref(cap)) == TC_ERR_ARG
            d_s, d_l, d_o, d_docs = _dev(s), _dev(l), _dev(good), _dev(docs)
            d_offs = torch.zeros(5, dtype=torch.int64).cuda()
            torch.cuda.synchronize()
            assert lib.tc_esa_doc_count_dev(cx, h._h, _dptr(d_s), _dptr(d_l), 4, 2, _dptr(d_o), None) == TC_ERR_ARG
            cap = C.c_uint64(100)
            assert lib.tc_esa_doc_list_dev(cx, h._h, _dptr(d_s), _dptr(d_l), 4, 0, _dptr(d_offs), _dptr(d_docs), None, C.byref(cap)) == TC_ERR_ARG
            still_answers()
        # nulls
        cap = C.c_uint64(0)
        assert lib.tc_esa_doc_count(cx, None, _p(good), _p(good), 4, 0, _p(good), None) == TC_ERR_ARG
        assert lib.tc_esa_doc_count(cx, h._h, None, _p(good), 4, 0, _p(good), None) == TC_ERR_ARG
        assert lib.tc_esa_doc_count(cx, h._h, _p(good), None, 4, 0, _p(good), None) == TC_ERR_ARG
        assert lib.tc_esa_doc_list(cx, h._h, _p(good), _p(good), 4, 0, None, None, None, C.byref(cap)) == TC_ERR_ARG
        assert lib.tc_esa_doc_list(cx, h._h, _p(good), _p(good), 4, 0, _p(offs), None, None, None) == TC_ERR_ARG
        cap = C.c_uint64(3)
        assert lib.tc_esa_doc_list(cx, h._h, _p(good), _p(good), 4, 0, _p(offs), None, None, C.byref(cap)) == TC_ERR_ARG
        still_answers()
        # a doc_start that breaks the rules: TC_ERR_ARG, *out NULL
        tt = np.frombuffer(t, np.uint8)
        for bad in ([1, n], [0, n - 1], [0, 500, 400, n], [0, n + 1, n]):
            hh = C.c_void_p(1)
            b = _u32(bad)
            assert lib.tc_esa_build_docs(cx, _p(tt), n, _p(b), len(b) - 1, C.byref(hh)) == TC_ERR_ARG and hh.value is None, bad
        hh = C.c_void_p(1)
        assert lib.tc_esa_build_docs(cx, _p(tt), n, _p(_u32([0, n])), 0, C.byref(hh)) == TC_ERR_ARG and hh.value is None
        hh = C.c_void_p(1)
        assert lib.tc_esa_build_docs(cx, _p(tt), n, None, 1, C.byref(hh)) == TC_ERR_ARG and hh.value is None
        assert lib.tc_esa_build_docs_dev(cx, None, 0, _p(_u32([0, 0])), 1, None) == TC_ERR_ARG
        still_answers()


def test_one_larger_text(ctx):
    t = _text(0x300, 200000, 4) + _text(0x301, 50000, 4) * 2 + b"a" * 1
    assert len(t) == 300001
    ds = _split(len(t), 300, 300)
    ref = _ref(t, ds)
    with ctx.esa_build_docs(t, ds) as h:
        _check_arrays(h, ref, "300 001 bytes")
        rng = np.random.default_rng(0x300)
        s = rng.integers(0, len(t) - 40, 20000)
        l = np.where(np.arange(20000) % 4 == 0, rng.integers(0, 6, 20000), rng.integers(6, 40, 20000))
        s[:3], l[:3] = (0, len(t), 250000), (len(t), 0, 50001)
        df = _docs(ctx, h, ref, s, l, limits=(0, 2), what="300 001 bytes")
        assert df.max() == 300 and (df == 2).any()
        for k in (1, 21):
            want = _kmer_docs(ctx, h, ref, k, ((1, 0), (2, 2), (300, 0)), what="300 001 bytes")
        assert len(want[0]) == 0 and len(ref.kmer_docs(1, 300)[0]) == 4         # each of ACGT is in every document, no 21-mer is
