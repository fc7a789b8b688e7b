"""FM-index queries on imported indexes that no build wrote, against the numpy model of tests/fm_wire_ref.py.

tc_fm_import_dev takes a byte string from the caller and checks its header, its size, the popcount of the marks and the
range of the text samples; everything else in it -- the rank vectors first of all -- is caller data that the queries meet
as it is.  The rule (include/textcomp.h at tc_fm_import_dev): a malformed body is answered by TC_ERR_MALFORMED at import or
at the query, or by TC_OK with the answer the contents define, and every kernel stays inside the index's parts.  The model
defines that answer from the bytes of the string alone, so every comparison here is exact: the same numbers, or TcMalformed
where the model says MALFORMED.  What a device test cannot see -- a read outside a part -- is seen on the CPU: by the
model's accessors (tests/test_fm_wire_ref.py) and, for the loop of fm_count_kernel, by host/check/fm_count_kernels.cpp under
a sanitizer (tests/test_host_checks.py).

The base indexes (tests/fm_foreign_cases.py: four texts, four builds each) are built by the library and compared part for
part with the model's builder first; the damaged strings are made from them.  Every damaged string is imported on a second
context and, where the import succeeds, queried through the host and the _dev entries of count, locate, extract, count_mm /
locate_mm (k = 1, 2) and factorize.  _dev outputs carry a canary behind their last slot, checked whatever the call returns;
after every refusal the same context answers the undamaged index exactly."""
import ctypes as C

import numpy as np
import pytest

import fm_foreign_cases as FC
import fm_wire_ref as W

pytestmark = pytest.mark.gpu

GUARD = 8                                   # canary slots behind every _dev output
FILL = {"int64": 0x5A5A5A5A5A5A5A5A, "int32": 0x5A5A5A5A, "uint8": 0x5A}
BASES = [(t, b) for t in FC.TEXTS for b in FC.BUILDS]


@pytest.fixture(scope="module")
def ctx():
    import textcomp
    c = textcomp.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx2():
    import textcomp
    c = textcomp.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ the _dev entries, guarded
class Guarded:
    """a device output of `slots` slots with GUARD canary slots behind them"""

    def __init__(self, slots, dtype):
        import torch
        self.slots = slots
        self.t = torch.full((slots + GUARD,), FILL[dtype], dtype=getattr(torch, dtype), device="cuda")

    @property
    def ptr(self):
        return C.c_void_p(self.t.data_ptr())

    def check(self):
        assert bool((self.t[self.slots:] == FILL[str(self.t.dtype).split(".")[1]]).all()), "a _dev entry wrote behind its output"

    def list(self, count=None):
        return self.t[:self.slots if count is None else count].cpu().numpy().tolist()


def _dev_batch(pats):
    import torch
    from textcomp import FMIndexHandle
    flat, offs = FMIndexHandle._pack(pats)
    return torch.from_numpy(flat).cuda(), torch.from_numpy(offs.astype(np.int64)).cuda()


def _call(ctx, outs, fn, *args):
    """one _dev call: the canaries are checked whatever it returns"""
    import torch
    torch.cuda.synchronize()
    try:
        rc = fn(ctx.handle, *args)
        torch.cuda.synchronize()
    finally:
        for o in outs:
            o.check()
    ctx._check(rc)


def _split(offs, *arrays):
    return [tuple(a[offs[i]:offs[i + 1]] for a in arrays) for i in range(len(offs) - 1)]


def dev_count(ctx, fm, pats, k=None):
    d_flat, d_offs = _dev_batch(pats)
    out = Guarded(len(pats), "int64")
    p = (C.c_void_p(d_flat.data_ptr()), C.c_void_p(d_offs.data_ptr()), len(pats))
    if k is None:
        _call(ctx, [out], ctx.lib.tc_fm_count_dev, fm._h, *p, out.ptr)
    else:
        _call(ctx, [out], ctx.lib.tc_fm_count_mm_dev, fm._h, *p, k, out.ptr)
    return out.list()


def dev_locate(ctx, fm, pats, total, k=None):
    d_flat, d_offs = _dev_batch(pats)
    hoffs, hits, mm = Guarded(len(pats) + 1, "int64"), Guarded(total, "int64"), Guarded(total, "uint8")
    nh = C.c_uint64(total)
    p = (C.c_void_p(d_flat.data_ptr()), C.c_void_p(d_offs.data_ptr()), len(pats))
    if k is None:
        _call(ctx, [hoffs, hits], ctx.lib.tc_fm_locate_dev, fm._h, *p, hoffs.ptr, hits.ptr, C.byref(nh))
        assert nh.value == total
        return [list(h) for h, in _split(hoffs.list(), hits.list())]
    _call(ctx, [hoffs, hits, mm], ctx.lib.tc_fm_locate_mm_dev, fm._h, *p, k, hoffs.ptr, hits.ptr, mm.ptr, C.byref(nh))
    assert nh.value == total
    return [(list(h), list(d)) for h, d in _split(hoffs.list(), hits.list(), mm.list())]


def dev_factorize(ctx, fm, pats, total):
    d_flat, d_offs = _dev_batch(pats)
    foffs, fpos, flen = Guarded(len(pats) + 1, "int64"), Guarded(total, "int64"), Guarded(total, "int32")
    nf = C.c_uint64(total)
    _call(ctx, [foffs, fpos, flen], ctx.lib.tc_fm_factorize_dev, fm._h, C.c_void_p(d_flat.data_ptr()), C.c_void_p(d_offs.data_ptr()),
          len(pats), foffs.ptr, fpos.ptr, flen.ptr, C.byref(nf))
    assert nf.value == total
    return foffs.list(), fpos.list(), flen.list()


def dev_extract(ctx, fm, starts, lens):
    import torch
    d_starts = torch.tensor(starts, dtype=torch.int64, device="cuda")
    d_lens = torch.tensor(lens, dtype=torch.int64, device="cuda")
    total = sum(lens)
    offs, out = Guarded(len(starts) + 1, "int64"), Guarded(total, "uint8")
    nb = C.c_uint64(total)
    _call(ctx, [offs, out], ctx.lib.tc_fm_extract_dev, fm._h, C.c_void_p(d_starts.data_ptr()), C.c_void_p(d_lens.data_ptr()), len(starts),
          offs.ptr, out.ptr, C.byref(nb))
    assert nb.value == total
    blob = bytes(out.list())
    o = offs.list()
    return [blob[o[i]:o[i + 1]] for i in range(len(starts))]


# ------------------------------------------------------------------------------------------------ one index against the model
def _host_queries(fm, text_name):
    """{query: callable} through the host entries, answers in the model's shapes"""
    pats, mm, mm2 = FC.patterns(text_name)
    q = {"count": lambda: fm.count(pats).tolist(),
         "count_mm1": lambda: fm.count_mm(mm, 1).tolist(),
         "count_mm2": lambda: fm.count_mm(mm2, 2).tolist()}
    if fm.sa_rate:
        q["locate"] = lambda: [h.tolist() for h in fm.locate(pats)]
        q["locate_mm1"] = lambda: [(h.tolist(), d.tolist()) for h, d in fm.locate_mm(mm, 1)]
        q["locate_mm2"] = lambda: [(h.tolist(), d.tolist()) for h, d in fm.locate_mm(mm2, 2)]
        q["factorize"] = lambda: tuple(a.tolist() for a in fm.factorize(pats))
    if fm.text_rate:
        q["extract"] = lambda: fm.extract(*FC.extract_queries(text_name))
    return q


def _dev_queries(ctx, fm, text_name, want):
    """the same through the _dev entries; the capacities are the model's totals"""
    pats, mm, mm2 = FC.patterns(text_name)
    q = {"count": lambda: dev_count(ctx, fm, pats),
         "count_mm1": lambda: dev_count(ctx, fm, mm, 1),
         "count_mm2": lambda: dev_count(ctx, fm, mm2, 2)}
    if fm.sa_rate:
        q["locate"] = lambda: dev_locate(ctx, fm, pats, sum(want["count"]))
        q["locate_mm1"] = lambda: dev_locate(ctx, fm, mm, sum(want["count_mm1"]), 1)
        q["locate_mm2"] = lambda: dev_locate(ctx, fm, mm2, sum(want["count_mm2"]), 2)
        q["factorize"] = lambda: dev_factorize(ctx, fm, pats, want["factor_total"])
    if fm.text_rate:
        q["extract"] = lambda: dev_extract(ctx, fm, *FC.extract_queries(text_name))
    return q


def _first_difference(got, want):
    if type(got) is not type(want) or not isinstance(got, (list, tuple)) or len(got) != len(want):
        return "got %.200r, want %.200r" % (got, want)
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            return "[%d]: %s" % (i, _first_difference(g, w))
    return "equal"


def check_index(ctx, fm, text_name, want, label, after_refusal=None):
    """every query of both forms against the model's answers `want`; returns the number of refusals"""
    from textcomp import TcMalformed
    refused = 0
    for form, queries in (("host", _host_queries(fm, text_name)), ("dev", _dev_queries(ctx, fm, text_name, want))):
        assert set(queries) == set(want) - {"factor_total"}
        for name, call in queries.items():
            try:
                got = call()
            except TcMalformed:
                got = W.MALFORMED
            assert got == want[name], "%s: %s (%s): %s" % (label, name, form, _first_difference(got, want[name]))
            if got == W.MALFORMED:
                refused += 1
                if after_refusal:
                    after_refusal()
    return refused


def _to_device(wire):
    import torch
    return torch.from_numpy(np.frombuffer(wire, np.uint8).copy()).cuda()


def run_cases(ctx2, text_name, build, cases):
    """the damaged strings of one base index: import on ctx2 and every query, or the refusal the model predicts; after every
    refusal the undamaged index, imported on the same context, answers exactly"""
    from textcomp import FMIndexHandle, TcMalformed
    base = FC.base_index(text_name, build)
    n = base.n
    good = FMIndexHandle.import_dev(ctx2, _to_device(FC.base_wire(text_name, build)), n=n)
    hostq = _host_queries(good, text_name)

    def still_good():
        for name in ("count", "locate", "extract"):
            if name in hostq:
                assert hostq[name]() == base.base_answers[name], "after a refusal: " + name
    try:
        for name, wire in cases:
            label = "%s %s %s" % (text_name, build, name)
            verdict = W.import_verdict(wire)
            try:
                bad = FMIndexHandle.import_dev(ctx2, _to_device(wire), n=n)
            except TcMalformed:
                assert verdict == W.MALFORMED, label + ": refused at import, the model imports it"
                still_good()
                continue
            try:
                assert verdict == W.OK, label + ": imported, the model refuses it"
                ix = W.WireIndex(wire)
                assert (bad.sa_rate, bad.text_rate) == (ix.sa_rate, ix.text_rate)
                check_index(ctx2, bad, text_name, FC.answers(ix, text_name), label, still_good)
            finally:
                bad.close()
        check_index(ctx2, good, text_name, base.base_answers, "%s %s undamaged, at the end" % (text_name, build))
    finally:
        good.close()


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("text_name,build", BASES)
def test_base_indexes_are_the_builders(ctx, ctx2, text_name, build):
    """the library's export of every base index is the model builder's string, part for part (the padding between the parts
    is not defined), and both forms of every query answer the model's -- brute force's, by tests/test_fm_wire_ref.py --
    numbers on its import"""
    from textcomp import FMIndexHandle
    text = FC.text_of(text_name)
    sa_rate, text_rate = FC.rates_of(text_name, build)
    fm = ctx.fm_build(text, sa_rate=sa_rate, text_rate=text_rate)
    try:
        got = fm.export_dev(with_locate=True).cpu().numpy().tobytes()
        want = FC.base_wire(text_name, build)
        assert len(got) == len(want) and got[:W.HDR_BYTES] == want[:W.HDR_BYTES]
        for name, o, nb in W.header_layout(W.Header(want))[0]:
            assert got[o:o + nb] == want[o:o + nb], name
        base = FC.base_index(text_name, build)
        check_index(ctx, fm, text_name, base.base_answers, "built")
        imp = FMIndexHandle.import_dev(ctx2, _to_device(want), n=len(text))
        try:
            assert check_index(ctx2, imp, text_name, base.base_answers, "imported") == 0
        finally:
            imp.close()
    finally:
        fm.close()


FAMILY_CASES = [(f, t, b) for f in FC.FAMILIES for t, b in FC.FAMILY_BASES[f]]


@pytest.mark.parametrize("family,text_name,build", FAMILY_CASES)
def test_damaged_imports_answer_the_model(ctx2, family, text_name, build):
    cases = FC.family(family, text_name, build)
    assert cases, "the family has no case on this base"
    run_cases(ctx2, text_name, build, cases)


@pytest.mark.parametrize("chunk", range(FC.VR_CHUNKS))
def test_random_damages_answer_the_model(ctx2, chunk):
    per = FC.VR_CASES // FC.VR_CHUNKS
    for i in range(chunk * per, (chunk + 1) * per):
        text_name, build, name, wire = FC.random_case(i)
        run_cases(ctx2, text_name, build, [(name, wire)])
