"""Every analysis over the enhanced suffix array, one after another on ONE context, at the text sizes where a carve of the
shared workspace plan (csrc/tc_esa_plan.hpp) crosses a rounding: the arena rounds every carve up to 256 bytes, so an offset
moves where 16 + n crosses 64 (n = 48), 4 (n + 1) crosses 256 (n = 63) and n + 16 crosses 256 (n = 240).  The sizes run
upwards and then downwards, so that a smaller call runs in a workspace a larger one left dirty.  Everything is exact:
each result against the Python references of tests/*_ref.py, the sa a call hands back against tc_suffix_array, and for
each list call the sizes-only form and one capacity-too-small form (TC_ERR_CAPACITY, the count set, the message)."""
import ctypes as C

import numpy as np
import pytest

import cover_ref
import esa_ref
import kmer_ref
import lcp_ref
import lz_ref
import maw_ref
import pal_ref
import rep_ref
import sus_ref
import textmatch_ref
import tr_ref

pytestmark = pytest.mark.gpu

TC_ERR_CAPACITY = -2
SIZES = (1, 2, 47, 48, 63, 64, 240, 241)
K = 3               # the k of the k-mer list
COVER_L = 3         # the min_len of the repeat cover


@pytest.fixture(scope="module")
def ctx():
    import textcomp
    c = textcomp.Context(0)
    yield c
    c.close()


def _text(seed, n):
    return np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(seed).integers(0, 4, n)].tobytes()


_REF = {}


def _ref(n):
    """the two texts of n bytes and every expected result, computed once and never changed"""
    if n in _REF:
        return _REF[n]
    t, q = _text(0xE5A0 + n, n), _text(0x7E00 + n, n)
    r = {"t": t, "q": q}
    sa, lcp = lcp_ref.esa_direct(t)
    r["esa"] = (sa, lcp)
    lpf, src = lz_ref.lpf_src(t)
    r["lpf"] = (lpf, src)
    r["parse"] = lz_ref.parse_of(t, lpf, src)
    for kind in (rep_ref.MAXIMAL, rep_ref.SUPERMAXIMAL):
        r["rep", kind] = rep_ref.repeats(t, kind)                       # (pos, len, occ, row, sa)
    row, pos, occ = kmer_ref.by_esa(sa, lcp, K)
    r["kmers"] = (np.array(pos, np.uint32), np.array(occ, np.uint32), np.array(row, np.uint32))
    r["ms"] = textmatch_ref.stats(q, t)                                 # (ms_len, ms_pos, ms_occ)
    r["mems"] = textmatch_ref.mems_of(r["ms"][0], r["ms"][1], 2)
    r["runs"] = tr_ref.runs(t)
    r["pal"] = pal_ref.palindromes(np.frombuffer(t, np.uint8), None, 0, 2)
    r["maw"] = maw_ref.absent_words(t)                                  # (left, pos, len)
    r["up"], r["mus"], r["point"] = sus_ref.reference(t)
    for kind in (cover_ref.ALL, cover_ref.LATER):
        r["spans", kind] = cover_ref.spans(cover_ref.cover(t, COVER_L, 2, kind))    # (start, len, covered)
    r["Ref"] = esa_ref.Ref(t)
    _REF[n] = r
    return r


def _np(x):
    import torch
    if isinstance(x, torch.Tensor):
        a = x.cpu().numpy()
        return a.view(np.uint32) if x.dtype == torch.int32 else a
    return x


def _same(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        if g is None:
            continue
        g, w = _np(g), np.asarray(w)
        assert g.dtype in (np.uint32, np.uint8) and g.shape == w.shape, (what, k, g.dtype, g.shape, w.shape)
        bad = np.nonzero(g != w)[0]
        assert len(bad) == 0, "%s: array %d, [%d] = %d, want %d" % (what, k, bad[0], g[bad[0]], w[bad[0]])


def _too_small(ctx, dev, name, noun, head, outs, need, tail=0, what=""):
    """the list call `name` with one slot fewer than the `need` it reports: TC_ERR_CAPACITY, the count, the message.  head:
    the arguments between the context and the outputs; outs: the outputs' dtypes; tail: pointers behind the count"""
    import torch
    if need == 0:
        return          # (no capacity is too small for an empty list)
    if dev:
        bufs = [torch.empty(need, dtype=torch.uint8 if dt == np.uint8 else torch.int32, device="cuda") for dt in outs]
        ptrs = [b.data_ptr() for b in bufs]
        torch.cuda.synchronize()
    else:
        bufs = [np.empty(need, dt) for dt in outs]
        ptrs = [b.ctypes.data for b in bufs]
    count = C.c_uint64(need - 1)
    extra = [C.c_uint64() for _ in range(tail)]
    rc = getattr(ctx.lib, name + ("_dev" if dev else ""))(ctx.handle, *head, *ptrs, C.byref(count), *(C.byref(e) for e in extra))
    msg = ctx.lib.tc_last_error(ctx.handle).decode()
    assert (rc, count.value, msg) == (TC_ERR_CAPACITY, need, "need %d %s slots, have %d" % (need, noun, need - 1)), (what, name, dev)


def _all_calls(ctx, n):
    """the host and the _dev form of every call, in one order, on the one context"""
    import torch
    r = _ref(n)
    t, q = r["t"], r["q"]
    tag = "n=%d" % n
    d_t = torch.from_numpy(np.frombuffer(t, np.uint8).copy()).cuda()
    d_q = torch.from_numpy(np.frombuffer(q, np.uint8).copy()).cuda()
    sa = ctx.suffix_array(t)
    _same((sa,), r["esa"][:1], tag + " tc_suffix_array")
    text = {False: [t, n], True: [d_t.data_ptr(), n]}

    # the LCP array
    _same(ctx.lcp_array(t), r["esa"], tag + " lcp_array")
    d_sa = ctx.suffix_array_dev(d_t)
    _same((d_sa, ctx.lcp_array_dev(d_t, d_sa)), r["esa"], tag + " lcp_array_dev")

    # the LPF array and the parse
    _same(ctx.lpf_array(t), r["lpf"], tag + " lpf_array")
    _same(ctx.lpf_array_dev(d_t), r["lpf"], tag + " lpf_array_dev")
    assert ctx.lz_phrase_count(t) == len(r["parse"][0]), tag
    _same(ctx.lz_parse(t), r["parse"], tag + " lz_parse")
    _same(ctx.lz_parse_dev(d_t), r["parse"], tag + " lz_parse_dev")
    for dev in (False, True):
        _too_small(ctx, dev, "tc_lz_parse", "phrase", text[dev], (np.uint32,) * 2, len(r["parse"][0]), what=tag)

    # the repeats, with the suffix array
    for kind in (rep_ref.MAXIMAL, rep_ref.SUPERMAXIMAL):
        want = r["rep", kind]
        assert np.array_equal(want[4], sa), tag
        assert ctx.repeat_count(t, supermaximal=bool(kind)) == len(want[0]), tag
        _same(ctx.repeats(t, supermaximal=bool(kind), with_sa=True), want, tag + " repeats kind=%d" % kind)
        _same(ctx.repeats_dev(d_t, supermaximal=bool(kind), with_sa=True), want, tag + " repeats_dev kind=%d" % kind)
        for dev in (False, True):
            _too_small(ctx, dev, "tc_repeats", "repeat", text[dev] + [kind, 1, 2, None], (np.uint32,) * 4, len(want[0]), what=tag)

    # the k-mers, with the suffix array
    want = r["kmers"] + (sa,)
    assert ctx.kmer_count(t, K) == len(want[0]), tag
    _same(ctx.kmers(t, K, with_sa=True), want, tag + " kmers")
    _same(ctx.kmers_dev(d_t, K, with_sa=True), want, tag + " kmers_dev")
    for dev in (False, True):
        _too_small(ctx, dev, "tc_kmers", "k-mer", text[dev] + [K, 1, 0, None], (np.uint32,) * 3, len(want[0]), what=tag)

    # one text against the other
    _same(ctx.text_match_stats(q, t), r["ms"], tag + " text_match_stats")
    _same(ctx.text_match_stats_dev(d_q, d_t), r["ms"], tag + " text_match_stats_dev")
    assert ctx.text_mem_count(q, t, 2) == len(r["mems"][0]), tag
    _same(ctx.text_mems(q, t, 2), r["mems"], tag + " text_mems")
    _same(ctx.text_mems_dev(d_q, d_t, 2), r["mems"], tag + " text_mems_dev")
    lcs = textmatch_ref.lcs_of(r["ms"][0], r["ms"][1])
    assert ctx.text_lcs(q, t) == lcs and ctx.text_lcs_dev(d_q, d_t) == lcs, tag
    for dev in (False, True):
        head = [d_q.data_ptr() if dev else q, n] + text[dev] + [2]
        _too_small(ctx, dev, "tc_text_mems", "MEM", head, (np.uint32,) * 3, len(r["mems"][0]), what=tag)

    # the runs
    assert ctx.tandem_repeat_count(t) == len(r["runs"][0]), tag
    _same(ctx.tandem_repeats(t), r["runs"], tag + " tandem_repeats")
    _same(ctx.tandem_repeats_dev(d_t), r["runs"], tag + " tandem_repeats_dev")
    for dev in (False, True):
        _too_small(ctx, dev, "tc_tandem_repeats", "run", text[dev] + [1, 0, 2, 1], (np.uint32,) * 3, len(r["runs"][0]), what=tag)

    # the palindromes
    assert ctx.palindrome_count(t, min_len=2) == len(r["pal"][0]), tag
    _same(ctx.palindromes(t, min_len=2), r["pal"], tag + " palindromes")
    _same(ctx.palindromes_dev(d_t, min_len=2), r["pal"], tag + " palindromes_dev")
    for dev in (False, True):
        _too_small(ctx, dev, "tc_palindromes", "palindrome", text[dev] + [None, 0, 2], (np.uint32,) * 3, len(r["pal"][0]), what=tag)

    # the minimal absent words
    assert ctx.absent_word_count(t) == len(r["maw"][0]), tag
    _same(ctx.absent_words(t), r["maw"], tag + " absent_words")
    _same(ctx.absent_words_dev(d_t), r["maw"], tag + " absent_words_dev")
    for dev in (False, True):
        _too_small(ctx, dev, "tc_absent_words", "word", text[dev] + [2, 0], (np.uint8, np.uint32, np.uint32), len(r["maw"][0]), what=tag)

    # what is unique
    _same((ctx.unique_prefixes(t),), (r["up"],), tag + " unique_prefixes")
    _same((ctx.unique_prefixes_dev(d_t),), (r["up"],), tag + " unique_prefixes_dev")
    assert ctx.unique_substring_count(t) == len(r["mus"][0]), tag
    _same(ctx.unique_substrings(t), r["mus"], tag + " unique_substrings")
    _same(ctx.unique_substrings_dev(d_t), r["mus"], tag + " unique_substrings_dev")
    _same(ctx.shortest_unique(t), r["point"], tag + " shortest_unique")
    _same(ctx.shortest_unique_dev(d_t), r["point"], tag + " shortest_unique_dev")
    for dev in (False, True):
        _too_small(ctx, dev, "tc_unique_substrings", "MUS", text[dev] + [1, 0], (np.uint32,) * 2, len(r["mus"][0]), what=tag)

    # the repeat cover's spans, both kinds
    for kind in (cover_ref.ALL, cover_ref.LATER):
        ws, wl, wc = r["spans", kind]
        assert ctx.repeat_cover_count(t, COVER_L, 2, kind) == (len(ws), wc), tag
        for got in (ctx.repeat_spans(t, COVER_L, 2, kind), ctx.repeat_spans_dev(d_t, COVER_L, 2, kind)):
            _same(got[:2], (ws, wl), tag + " repeat_spans kind=%d" % kind)
            assert int(got[2]) == wc, tag
        for dev in (False, True):
            _too_small(ctx, dev, "tc_repeat_spans", "span", text[dev] + [COVER_L, 2, kind], (np.uint32,) * 2, len(ws), tail=1, what=tag)

    # the kept ESA and one batch of longest common extensions
    ref = r["Ref"]
    a = np.arange(n, dtype=np.uint32)
    b = a[::-1].copy()
    with ctx.esa_build(t) as h:
        _same((h.read("sa", ctx=ctx), h.read("lcp", ctx=ctx)), r["esa"], tag + " esa_build")
        _same(h.lce(a, b, 1, mm=True, ctx=ctx), ref.lce(a, b, 1), tag + " esa lce")
    with ctx.esa_build_dev(d_t) as h:
        _same(h.lce(a, b, 0, mm=True, ctx=ctx), ref.lce(a, b, 0), tag + " esa_build_dev lce")


def test_every_analysis_at_the_rounding_sizes_up_and_down(ctx):
    for n in SIZES + SIZES[::-1]:
        _all_calls(ctx, n)
