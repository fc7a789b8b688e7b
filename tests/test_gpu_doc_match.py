"""Cross-document matches on the kept enhanced suffix array (tc_esa_doc_match, tc_esa_doc_shared and the compositions
ESAHandle.shared_spans / shared_mask / shared_dedup) against the reference of tests/doc_match_ref.py (numpy; tests/test_doc_match_ref.py
holds it to loops over the bytes).  Everything is compared exactly.  Every case goes through the host entry of the C ABI, through
ESAHandle's host methods and through its _dev methods, both kinds and both clamps, on the smallest shapes at which the kernels can go
wrong: texts of 0, 1 and 2 bytes; 1 document (all zeros), 2, 3, 255, 256, 257 documents and 65535 documents on 150 000 bytes; empty
documents at both ends and adjacent; two identical documents; the four worked examples of include/textcomp.h; row counts one below, at
and one above one and two tiles of the scans (ESX_TILE = 2048 rows); a first document that owns more than three tiles of consecutive
rows, with heads in earlier tiles; the eight-level fan-out-4 tree on 65 537 bytes; all 256 byte values; 120-byte texts of six shapes in
1, 3 and 40 documents; each combination of NULL outputs; doc_shared at min_len 1, 2, 3, 20; a plain handle refused; the error protocol;
two contexts on one handle; the older queries unchanged afterwards; and on 300 001 bytes in 300 documents the unclamped lengths against
tc_esa_doc_count_dev at limit 2."""
import ctypes as C
import functools

import numpy as np
import pytest

import cover_ref
import doc_match_ref as X
import esa_docs_ref as R
import test_gpu_esa as E
from test_gpu_esa import _dbg, _dev, _np, _p, _same, _shape, _text, _u32

pytestmark = pytest.mark.gpu

TC_ERR_ARG = -1
ESX_TILE = 2048
KINDS = (X.OTHER, X.EARLIER)
MIN_LENS = (1, 2, 3, 20)
FILL = 0xabababab


@pytest.fixture(scope="module")
def ctx():
    import textcomp
    c = textcomp.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _ref_of(t, ds):
    return X.XRef(t, np.array(ds, np.int64))


def _ref(t, ds):
    return _ref_of(bytes(t), tuple(int(x) for x in ds))


def _split(n, ndocs, seed):
    """ndocs documents over n bytes: equal sizes, every inner boundary moved by -1, 0 or 1 (so some documents are empty)"""
    ds = R.split_evenly(n, ndocs)
    if ndocs > 1:
        ds[1:-1] += np.random.default_rng(seed).integers(-1, 2, ndocs - 1)
    return np.clip(np.maximum.accumulate(ds), 0, n)


def _dptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def _match(ctx, h, ref, what="", kinds=KINDS, clamps=(True, False), min_lens=MIN_LENS):
    """the per-position and the per-document answers through the three forms"""
    import torch
    lib, cx, n, nd = ctx.lib, ctx.handle, ref.n, ref.ndocs
    for kind in kinds:
        for clamp in clamps:
            tag = "%s match n=%d ndocs=%d kind=%d clamp=%d" % (what, n, nd, kind, clamp)
            want = [w.astype(np.uint32) for w in ref.match(kind, clamp)]
            out = [np.full(n, FILL, np.uint32) for _ in range(3)]
            assert lib.tc_esa_doc_match(cx, h._h, kind, int(clamp), *(_p(o) for o in out)) == 0, tag
            host = h.doc_match(kind, clamp, src=True, doc=True, ctx=ctx)
            dev = h.doc_match_dev(kind, clamp, src=True, doc=True, ctx=ctx)
            assert dev[0].dtype == torch.int32
            for i, name in enumerate(("xl", "src", "xdoc")):
                _same(out[i], want[i], tag + " abi " + name)
                _same(host[i], want[i], tag + " host " + name)
                _same(dev[i], want[i], tag + " dev " + name)
            _same(h.doc_match(kind, clamp, ctx=ctx), want[0], tag + " host xl alone")
            _same(h.doc_match_dev(kind, clamp, ctx=ctx), want[0], tag + " dev xl alone")
        for L in min_lens:
            tag = "%s shared n=%d ndocs=%d kind=%d min_len=%d" % (what, n, nd, kind, L)
            ws, wl = ref.shared(kind, L)
            shared, longest = np.full(nd, FILL, np.uint64), np.full(nd, FILL, np.uint32)
            assert lib.tc_esa_doc_shared(cx, h._h, kind, L, _p(shared), _p(longest)) == 0, tag
            _same(shared, ws, tag + " abi shared")
            _same(longest, wl, tag + " abi longest")
            got = h.doc_shared(L, kind, ctx=ctx)
            _same(got[0], ws, tag + " host shared")
            _same(got[1], wl, tag + " host longest")
            got = h.doc_shared_dev(L, kind, ctx=ctx)
            assert got[0].dtype == torch.int64
            _same(got[0].cpu().numpy().astype(np.uint64), ws, tag + " dev shared")
            _same(got[1], wl, tag + " dev longest")


def _collection(ctx, t, ds, what="", **kw):
    ref = _ref(t, ds)
    with ctx.esa_build_docs(t, ds) as h:
        _match(ctx, h, ref, what, **kw)
    return ref


def _row(s):
    return [X.NO_POS if x == "-" else int(x) for x in s.split()]


# ------------------------------------------------------------------------------------------------ the cases
def test_tiny_texts(ctx):
    for t in (b"", b"a", b"ab", b"aa"):
        n = len(t)
        for ds in ([0, n], [0, 0, n], [0, n, n], [0, n // 2, n], [0, 0, n // 2, n, n]):
            _collection(ctx, t, ds, "tiny")
    with ctx.esa_build_docs(b"", [0, 0, 0]) as h:           # n = 0: TC_OK, nothing touched for match; zeros for shared
        out = np.full(2, FILL, np.uint32)
        assert ctx.lib.tc_esa_doc_match(ctx.handle, h._h, 0, 1, _p(out), _p(out), _p(out)) == 0 and (out == FILL).all()
        assert ctx.lib.tc_esa_doc_match(ctx.handle, h._h, 0, 1, None, None, None) == 0
        assert ctx.lib.tc_esa_doc_match(ctx.handle, h._h, 2, 1, _p(out), None, None) == TC_ERR_ARG
        shared, longest = h.doc_shared(1)
        assert shared.tolist() == [0, 0] and longest.tolist() == [0, 0] and len(h.doc_match()) == 0


def test_the_headers_examples(ctx):
    import textcomp
    text, ds = textcomp.concat_docs([b"banana", b"bandana", b"ananas"])
    with ctx.esa_build_docs(text, ds) as h:
        for clamp in (True, False):
            xl, src, xdoc = h.doc_match(textcomp.DOC_OTHER, clamp, src=True, doc=True)
            assert xl.tolist() == _row("3 5 4 3 2 1 3 2 1 0 3 2 1 5 4 3 2 1 0")
            assert src.tolist() == _row("6 13 14 10 11 12 0 15 16 - 3 4 5 1 2 1 2 7 -")
            assert xdoc.tolist() == _row("1 2 2 1 1 1 0 2 2 - 0 0 0 0 0 0 0 1 -")
        for L in (1, 2, 3):
            shared, longest = h.doc_shared(L)
            assert shared.tolist() == [6, 6, 5] and longest.tolist() == [5, 3, 5]
        xl, src = h.doc_match(textcomp.DOC_EARLIER, src=True)
        assert xl.tolist() == _row("0 0 0 0 0 0 3 2 1 0 3 2 1 5 4 3 2 1 0")
        assert src.tolist() == _row("- - - - - - 0 1 2 - 3 4 5 1 2 1 2 7 -")
        shared, longest = h.doc_shared(1, textcomp.DOC_EARLIER)
        assert shared.tolist() == [0, 6, 5] and longest.tolist() == [0, 3, 5]
        _match(ctx, h, _ref(text.tobytes(), ds), "example 1")
    text, ds = textcomp.concat_docs([b"ab", b"cab", b"abc"])
    with ctx.esa_build_docs(text, ds) as h:
        assert h.doc_match(clamp=False).tolist() == _row("3 2 1 2 1 3 2 1")
        xl, src, xdoc = h.doc_match(src=True, doc=True)
        assert (xl.tolist(), src.tolist(), xdoc.tolist()) == (_row("2 1 1 2 1 3 2 1"), _row("5 6 7 5 6 0 1 2"), _row("2 2 2 2 2 0 0 1"))
        for L, want in ((1, [2, 3, 3]), (2, [2, 2, 3]), (3, [0, 0, 3])):
            shared, longest = h.doc_shared(L)
            assert shared.tolist() == want and longest.tolist() == [2, 2, 3]
        s, l, cov = h.shared_spans(2)
        assert list(zip(s.tolist(), l.tolist())) == [(0, 2), (3, 5)] and cov == 7
        assert h.shared_mask(2)[0].tolist() == _row("1 1 0 1 1 1 1 1") and h.shared_dedup(2)[0].tobytes() == b"c"
        xl, src, xdoc = h.doc_match(textcomp.DOC_EARLIER, src=True, doc=True)
        assert (xl.tolist(), src.tolist(), xdoc.tolist()) == (_row("0 0 0 2 1 3 2 1"), _row("- - - 0 1 0 1 2"), _row("- - - 0 0 0 0 1"))
        assert h.shared_mask(2, textcomp.DOC_EARLIER)[0].tolist() == _row("0 0 0 1 1 1 1 1")
        assert h.shared_dedup(2, textcomp.DOC_EARLIER)[0].tobytes() == b"abc"
        _match(ctx, h, _ref(text.tobytes(), ds), "example 3")


@pytest.mark.parametrize("ndocs", (1, 2, 3, 255, 256, 257))
def test_document_counts(ctx, ndocs):
    t = _text(0xD0C + ndocs, 2500, 4) + (b"abc" * 200) + b"a" * 300
    ref = _collection(ctx, t, _split(len(t), ndocs, ndocs), "ndocs %d" % ndocs)
    if ndocs == 1:                                          # one document: all-zero xl, no partner, nothing shared, both kinds
        for kind in KINDS:
            xl, src, xdoc = ref.match(kind, True)
            assert not xl.any() and (src == X.NO_POS).all() and (xdoc == X.NO_DOC).all() and not ref.shared(kind, 1)[0].any()


def test_65535_documents_on_150000_bytes(ctx):
    t = _text(0xFFFF, 150000, 4)
    ds = _split(len(t), 65535, 5)
    _collection(ctx, t, ds, "65535", clamps=(True,), min_lens=(1, 3))


def test_empty_documents_and_identical_documents(ctx):
    t = _shape("fibonacci", 900)
    n = len(t)
    for ds in ([0, 0, 0, 300, 300, 300, 900, 900, 900], [0, 0, n], [0, n, n], [0] * 40 + [n] * 40):
        _collection(ctx, t, ds, "empty ends", clamps=(True,))
    d = _text(0x1D, 700, 4)
    ref = _collection(ctx, d + d, [0, 700, 1400], "identical")
    xl = ref.match(X.OTHER, True)[0]
    assert xl.tolist() == list(range(700, 0, -1)) * 2       # the whole rest of the document, clamped
    assert ref.match(X.OTHER, False)[0][0] == 700 and ref.shared(X.EARLIER, 1)[0].tolist() == [0, 700]


@pytest.mark.parametrize("rows", (ESX_TILE - 1, ESX_TILE, ESX_TILE + 1, 2 * ESX_TILE - 1, 2 * ESX_TILE, 2 * ESX_TILE + 1))
def test_row_counts_around_the_tiles_of_the_scans(ctx, rows):
    n = rows - 1
    for shape, ndocs in (("random4", 300), ("unary", 3), ("period3", 7)):
        _collection(ctx, _shape(shape, n), _split(n, ndocs, rows), "%s rows %d" % (shape, rows), clamps=(True,), min_lens=(1, 20))


def test_a_run_over_more_than_three_tiles(ctx):
    t = b"a" * 10000 + b"aab"
    ref = _collection(ctx, t, [0, 10000, len(t)], "long run")
    a, b = ref.neighbours(X.OTHER)
    run = np.nonzero(ref.da[1:] != ref.da[:-1])[0] + 1      # the boundaries: one run of the first document spans more than three tiles,
    assert np.diff(run).max() > 3 * ESX_TILE                # and the head of most of its rows lies in an earlier tile
    assert ((np.arange(ref.N) // ESX_TILE) > (a + 1) // ESX_TILE).sum() > 2 * ESX_TILE
    _collection(ctx, t, [0, 5, ESX_TILE, ESX_TILE, 3 * ESX_TILE + 1, len(t)], "documents over tiles")


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
        assert h.device_bytes(5) * 3 > 4 * (len(t) + 1)     # a tree of fan-out 4: a third of its array
        _match(ctx, h, _ref(t, ds), "fan-out 4", min_lens=(1, 20))


@pytest.mark.parametrize("shape", E.SHAPES)
def test_short_texts_of_six_shapes(ctx, shape):
    t = _shape(shape, 120)
    if shape == "all256":
        every = _shape(shape, 256)
        assert len(set(every)) == 256
        _collection(ctx, every * 2 + every[::-1] * 2 + every[:100], _split(1124, 5, 256), "all 256 byte values", clamps=(True,))
    for ndocs in (1, 3, 40):
        _collection(ctx, t, _split(len(t), ndocs, ndocs), "%s %d docs" % (shape, ndocs))


def test_null_outputs(ctx):
    import torch
    t = _text(0x0A11, 1500, 2) + b"ab" * 300
    n = len(t)
    ds = _split(n, 9, 9)
    ref = _ref(t, ds)
    lib, cx = ctx.lib, ctx.handle
    with ctx.esa_build_docs(t, ds) as h:
        for kind in KINDS:
            want = [w.astype(np.uint32) for w in ref.match(kind, True)]
            ws, wl = ref.shared(kind, 2)
            for mask in range(8):
                out = [np.full(n, FILL, np.uint32) if mask >> i & 1 else None for i in range(3)]
                d_out = [_dev(np.full(n, FILL, np.uint32)) if mask >> i & 1 else None for i in range(3)]
                torch.cuda.synchronize()
                rc = lib.tc_esa_doc_match(cx, h._h, kind, 1, *(_p(o) for o in out))
                rd = lib.tc_esa_doc_match_dev(cx, h._h, kind, 1, *(_dptr(o) for o in d_out))
                assert rc == rd == (0 if mask else TC_ERR_ARG), (kind, mask)
                for i in range(3):
                    if mask >> i & 1:
                        _same(out[i], want[i], "null outputs abi %d/%d" % (mask, i))
                        _same(d_out[i], want[i], "null outputs dev %d/%d" % (mask, i))
            for mask in range(4):
                shared = np.full(9, FILL, np.uint64) if mask & 1 else None
                longest = np.full(9, FILL, np.uint32) if mask & 2 else None
                d_shared = torch.full((9,), -1, dtype=torch.int64).cuda() if mask & 1 else None
                d_longest = _dev(np.full(9, FILL, np.uint32)) if mask & 2 else None
                torch.cuda.synchronize()
                rc = lib.tc_esa_doc_shared(cx, h._h, kind, 2, _p(shared), _p(longest))
                rd = lib.tc_esa_doc_shared_dev(cx, h._h, kind, 2, _dptr(d_shared), _dptr(d_longest))
                assert rc == rd == (0 if mask else TC_ERR_ARG), (kind, mask)
                if mask & 1:
                    _same(shared, ws, "shared alone")
                    _same(d_shared.cpu().numpy().astype(np.uint64), ws, "shared alone, dev")
                if mask & 2:
                    _same(longest, wl, "longest alone")
                    _same(d_longest, wl, "longest alone, dev")


def test_the_compositions_are_the_cover_of_the_reference(ctx):
    import textcomp
    t = _text(0xC0F, 3000, 4) + b"acgt" * 300 + _text(0xC0F, 1500, 4)
    n = len(t)
    ds = _split(n, 11, 11)
    ref = _ref(t, ds)
    with ctx.esa_build_docs(t, ds) as h:
        for kind in KINDS:
            for L in (1, 4, 12, 5000):
                cov = ref.cover(kind, L)
                ws, wl, wc = cover_ref.spans(cov)
                s, l, c = h.shared_spans(L, kind)
                _same(s, ws, "spans start")
                _same(l, wl, "spans len")
                d = h.shared_spans_dev(L, kind)
                _same(d[0], ws, "spans start, dev")
                assert c == d[2] == wc
                for m in (None, textcomp.SOFT_MASK):
                    out, c = h.shared_mask(L, kind, map=m)
                    _same(out, cover_ref.mask(t, cov, None if m is None else np.frombuffer(bytes(m), np.uint8)), "mask")
                    _same(h.shared_mask_dev(L, kind, map=m)[0].cpu().numpy(), out, "mask, dev")
                    assert c == wc
                out, c = h.shared_dedup(L, kind)
                assert out.tobytes() == cover_ref.dedup(t, cov) and c == wc
                assert h.shared_dedup_dev(L, kind)[0].cpu().numpy().tobytes() == out.tobytes()


def test_a_plain_handle_is_refused_and_the_older_queries_are_unchanged(ctx):
    import textcomp
    t = _text(0xA78, 3000, 4) + b"acgt" * 200
    n = len(t)
    ds = _split(n, 12, 12)
    ref = _ref(t, ds)
    lib, cx = ctx.lib, ctx.handle
    out, out64 = np.zeros(n, np.uint32), np.zeros(12, np.uint64)
    with ctx.esa_build(t) as plain, ctx.esa_build_docs(t, ds) as h:
        assert lib.tc_esa_doc_match(cx, plain._h, 0, 1, _p(out), None, None) == TC_ERR_ARG
        assert "no documents" in lib.tc_last_error(cx).decode()
        assert lib.tc_esa_doc_shared(cx, plain._h, 0, 1, _p(out64), None) == TC_ERR_ARG
        with pytest.raises(textcomp.TcError):
            plain.doc_match()
        with pytest.raises(textcomp.TcError):
            plain.doc_shared_dev()
        before = [h.device_bytes(p) for p in range(8)]
        with textcomp.Context(0) as other:                  # another context on the handle's device queries it: the scratch is its own
            _match(other, h, ref, "other context", clamps=(True,), min_lens=(2,))
            _match(ctx, h, ref, "first context", clamps=(False,), min_lens=(3,))
            _match(other, h, ref, "other context", clamps=(True,), min_lens=(1,))
        a, b = h.doc_match_dev(src=True), h.doc_match_dev(src=True)        # two calls give identical output
        assert all(bool((x == y).all()) for x, y in zip(a, b))
        # the handle is read-only: its bytes, its arrays and every older query are as before
        assert [h.device_bytes(p) for p in range(8)] == before and before[0] == sum(before[1:])
        E._all_queries(ctx, h, t, 400, 1)
        dref = R.DocRef(t, ds)
        _same(h.read("da"), dref.da.astype(np.uint32), "da")
        _same(h.read("pv"), dref.pv.astype(np.uint32), "pv")
        for what in ("text", "sa", "isa", "lcp"):
            assert np.array_equal(h.read(what), plain.read(what))
        s, l = np.arange(0, n - 8, 7), np.full(len(range(0, n - 8, 7)), 6)
        df, occ = dref.count(s, l, 0)
        got = h.doc_count(s, l, occ=True)
        _same(got[0], df, "doc_count afterwards")
        _same(got[1], occ, "occ afterwards")


def test_errors_leave_the_handle_and_the_context_usable(ctx):
    t = _text(0xE45, 999, 4)
    n = len(t)
    ds = _split(n, 5, 5)
    ref = _ref(t, ds)
    lib, cx = ctx.lib, ctx.handle
    with ctx.esa_build_docs(t, ds) as h:
        out, out64 = np.full(n, FILL, np.uint32), np.full(5, FILL, np.uint64)
        d_out = _dev(out)
        for kind in (2, -1, 7):
            assert lib.tc_esa_doc_match(cx, h._h, kind, 1, _p(out), None, None) == TC_ERR_ARG
            assert "TC_DOC_OTHER" in lib.tc_last_error(cx).decode()
            assert lib.tc_esa_doc_match_dev(cx, h._h, kind, 0, _dptr(d_out), None, None) == TC_ERR_ARG
            assert lib.tc_esa_doc_shared(cx, h._h, kind, 1, _p(out64), None) == TC_ERR_ARG
        assert lib.tc_esa_doc_shared(cx, h._h, 0, 0, _p(out64), None) == TC_ERR_ARG and "min_len" in lib.tc_last_error(cx).decode()
        assert lib.tc_esa_doc_shared_dev(cx, h._h, 1, 0, None, _dptr(d_out)) == TC_ERR_ARG
        assert lib.tc_esa_doc_match(cx, None, 0, 1, _p(out), None, None) == TC_ERR_ARG
        assert lib.tc_esa_doc_match(None, h._h, 0, 1, _p(out), None, None) == TC_ERR_ARG
        assert lib.tc_esa_doc_shared(cx, None, 0, 1, _p(out64), None) == TC_ERR_ARG
        assert (out == FILL).all() and (out64 == FILL).all() and (_np(d_out) == FILL).all()     # nothing was touched
        _match(ctx, h, ref, "after the errors", min_lens=(1, 2000))


def test_one_larger_text_against_the_document_counts(ctx):
    import torch
    t = _text(0x300, 200000, 4) + _text(0x301, 50000, 4) * 2 + b"a" * 1
    n = len(t)
    assert n == 300001
    ds = _split(n, 300, 300)
    with ctx.esa_build_docs(t, ds) as h:
        xl = h.doc_match_dev(clamp=False)
        host = h.doc_match(clamp=False)
        _same(xl, host, "dev and host")
        assert host.max() >= 50000 and (host == 0).sum() < n // 100
        pos = np.random.default_rng(0x300).integers(0, n, 20000)
        pos[:3] = (0, n - 1, 250000)
        d_pos = _dev(pos)
        at = xl[torch.from_numpy(pos).cuda()]
        # L = xl[i]: the substring occurs in a second document (answer 2) wherever xl[i] > 0
        df = _np(h.doc_count_dev(d_pos, at.contiguous(), limit=2))
        hit = host[pos] > 0
        assert (df[hit] == 2).all() and hit.sum() > 19000
        # L = xl[i] + 1, where it still fits the text: no second document
        fits = pos + host[pos].astype(np.int64) + 1 <= n
        df = _np(h.doc_count_dev(_dev(pos[fits]), _dev(host[pos][fits].astype(np.int64) + 1), limit=2))
        assert (df < 2).all() and fits.sum() > 19000
