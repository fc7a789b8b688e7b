"""The fused decode on blocks that no encoder wrote (tests/block_ref.py builds them, the CPU oracle judges them).

Every block goes through tc_decode and through tc_decode_dev on a tensor with 256 canary bytes behind the text; one
block per family also goes through tc_block_to_container_dev + tc_decode_container.  The expectation is always
block_ref.decode_block_ref: the same bytes, or TcMalformed.  After every refused call the same context decodes an
untouched encoder block exactly.

What this reaches that encoder output does not: the refusal of imtf257_check_kernel and the nine-bit path below it
(T5, M2 and M3 on sigma = 257), the chain kernel on streams that lack byte values or meet them late (T4 over 257, the
"late" text), the LF walk's refusal and the way through codes_to_syms_kernel to the symbol walk (M2 on ACGTN), counting
tables with empty symbols (T4), lists that are permuted or hold duplicates (T2, T3), the "value does not fit a byte"
flag of the byte-wide run-length decode (T1 with foreign values on runs of length 0, M1), and -- M3 -- last columns that
are no BWT of any text yet decode to a full-length text, which the library must return byte for byte.

Not observable here: every stream on which the LF walk refuses (no Nothing, or more than one) is one the reference
refuses too -- without a Nothing its text is empty, with a second one the walk meets it (fromJust) or misses its row and
comes out short -- so all that can be seen of the fall-back through codes_to_syms_kernel is that it refuses as well.

Out of scope: the chain kernel's outer `t += 2048` step over the tile maxima needs more than 8 M rows; no text here is
above 70 001 bytes.  The container formats carry neither a run of length 0 nor a value that does not fit their value
bits, so T1's zero-count blocks, most of M1 and M4's run lists go to tc_decode and tc_decode_dev only.
"""
import ctypes as C

import numpy as np
import pytest

import block_ref as B

pytestmark = pytest.mark.gpu

CANARY = 0xA5
GOOD_TEXT = b"mississippi" * 50


@pytest.fixture(scope="module")
def ctx():
    import textcomp
    c = textcomp.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def good(ctx):
    return ctx.encode(GOOD_TEXT)


def _c_block(blk, count_ptr, value_ptr):
    from textcomp import Block
    b = Block()
    b.n, b.primary, b.sigma, b.nruns = int(blk["n"]), int(blk["primary"]), int(blk["sigma"]), len(blk["run_count"])
    for i, v in enumerate(blk["final_list"]):
        b.final_list[i] = int(v)
    b.run_count, b.run_value = count_ptr, value_ptr
    return b


def _dev_runs(blk):
    import torch
    d_c = torch.from_numpy(np.ascontiguousarray(blk["run_count"], np.uint32).view(np.int32)).cuda()
    d_v = torch.from_numpy(np.ascontiguousarray(blk["run_value"], np.uint16).view(np.int16)).cuda()
    return d_c, d_v


def _host(ctx, blk):
    """tc_decode"""
    rc_ = np.ascontiguousarray(blk["run_count"], np.uint32)
    rv_ = np.ascontiguousarray(blk["run_value"], np.uint16)
    out = np.empty(int(blk["n"]), np.uint8)
    b = _c_block(blk, rc_.ctypes.data, rv_.ctypes.data)
    ctx._check(ctx.lib.tc_decode(ctx.handle, C.byref(b), C.c_void_p(out.ctypes.data)))
    return out.tobytes()


def _dev(ctx, blk):
    """tc_decode_dev into a tensor with a canary behind the n text bytes; the canary is checked whatever the call answers"""
    import torch
    n = int(blk["n"])
    d_c, d_v = _dev_runs(blk)
    d_out = torch.full((n + 256,), CANARY, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    b = _c_block(blk, d_c.data_ptr(), d_v.data_ptr())
    rc = ctx.lib.tc_decode_dev(ctx.handle, C.byref(b), C.c_void_p(d_out.data_ptr()))
    torch.cuda.synchronize()
    back = d_out.cpu().numpy()
    assert (back[n:] == CANARY).all(), "tc_decode_dev wrote behind the n text bytes (rc %d)" % rc
    ctx._check(rc)
    return back[:n].tobytes()


def _container(ctx, blk):
    """tc_block_to_container_dev, then tc_decode_container"""
    import torch
    d_c, d_v = _dev_runs(blk)
    bound = int(ctx.lib.tc_container_bound(len(blk["run_count"]), int(blk["sigma"])))
    buf = torch.zeros(bound + 64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    used = C.c_uint64(bound)
    b = _c_block(blk, d_c.data_ptr(), d_v.data_ptr())
    ctx._check(ctx.lib.tc_block_to_container_dev(ctx.handle, C.byref(b), C.c_void_p(buf.data_ptr()), C.byref(used)))
    return ctx.decode_container(buf[:used.value].cpu().numpy().tobytes())


def _expect(ctx, good, fn, blk, exp, what):
    import textcomp
    if exp == B.MALFORMED:
        with pytest.raises(textcomp.TcMalformed):
            got = fn(ctx, blk)
            pytest.fail("%s: decoded to %d bytes with TC_OK, the reference refuses the block" % (what, len(got)))
        assert ctx.decode(good) == GOOD_TEXT, "%s: the context does not decode a good block after the refusal" % what
    else:
        try:
            got = fn(ctx, blk)
        except textcomp.TcError as e:
            pytest.fail("%s: %s; the reference decodes the block to %d bytes" % (what, e, len(exp)))
        if got != exp:
            d = np.nonzero(np.frombuffer(got, np.uint8) != np.frombuffer(exp, np.uint8))[0]
            pytest.fail("%s: %d of %d bytes differ from the reference's text, the first at %d" % (what, len(d), len(exp), d[0]))


def _check(ctx, good, blk, exp, what, fns=(_host, _dev)):
    for fn in fns:
        _expect(ctx, good, fn, blk, exp, "%s %s" % (what, fn.__doc__.split()[0]))


def _params(families):
    return [pytest.param(f, a, n, id="%s-%s-%d" % (f, a, n)) for f in families for a, n in B.FAMILY_BASES[f]]


def test_base_blocks_are_the_encoders(ctx):
    """the blocks everything here starts from are, field by field, what tc_encode writes for the text"""
    for name, n in B.all_bases():
        ours, theirs = B.base_block(name, n), ctx.encode(B.base_text(name, n))
        assert (ours["n"], ours["primary"], ours["sigma"]) == (theirs["n"], theirs["primary"], theirs["sigma"]), (name, n)
        for k in ("final_list", "run_count", "run_value"):
            assert np.array_equal(ours[k], theirs[k]), (name, n, k)
        _check(ctx, None, ours, B.base_text(name, n), "%s-%d" % (name, n))


@pytest.mark.parametrize("family,name,n", _params(["T1", "T2", "T3", "T4", "T5"]))
def test_still_valid(ctx, good, family, name, n):
    """T: blocks the reference decodes to the text (runs cut up and zero-count runs, the list permuted / with duplicates /
    with symbols that never occur, a wrong primary) decode to the text"""
    for cid, blk, exp in B.cases(family, name, n):
        assert exp == B.base_text(name, n)
        _check(ctx, good, blk, exp, "%s %s-%d %s" % (family, name, n, cid))


@pytest.mark.parametrize("family,name,n", _params(["M1", "M2", "M3", "M4"]))
def test_damaged(ctx, good, family, name, n):
    """M: an index outside the list, no / a second Nothing, two rows of the last column swapped, lengths that do not add
    up -- the reference's answer, be it a refusal or a (different) text"""
    cs = B.cases(family, name, n)
    assert family == "M3" or any(exp == B.MALFORMED for _, _, exp in cs)
    for cid, blk, exp in cs:
        _check(ctx, good, blk, exp, "%s %s-%d %s" % (family, name, n, cid))


def test_m3_discriminates(ctx):
    """per alphabet the swaps hold at least five blocks that are no BWT of a text and still decode full length"""
    for name, ns in B.m3_bases():
        exps = [exp for n in ns for _, _, exp in B.cases("M3", name, n)]
        assert sum(e != B.MALFORMED for e in exps) >= 5 and sum(e == B.MALFORMED for e in exps) >= 5, name


def test_lists_out_of_range(ctx, good):
    """M5.  A list entry outside -1..255 is TC_ERR_ARG, as is sigma above TC_MAX_SIGMA; sigma = 0 with n > 0 decodes to
    the empty sequence (MTF/Internal.hs:202-209), which is not n bytes: TC_ERR_MALFORMED (textcomp.h, tc_decode)"""
    import textcomp
    for name, n in (("acgtn", 4096), ("s12", 4097), ("s100", 70001), ("b256", 4097)):
        for cid, blk, exp in B.m5_lists(B.base_block(name, n)):
            for fn in (_host, _dev):
                with pytest.raises(textcomp.TcError) as e:
                    fn(ctx, blk)
                assert e.value.code == (textcomp._lib.TC_ERR_ARG if exp == "arg" else textcomp._lib.TC_ERR_MALFORMED), (name, cid)
                assert ctx.decode(good) == GOOD_TEXT


def _container_cases():
    """one block per family that the container formats can carry (counts >= 1, values inside the format's value bits)"""
    pick = [("T1", "acgtn", 70001, "split"), ("T1", "b256", 4097, "split"), ("T2", "s12", 70001, "rev"),
            ("T3", "acgtn", 70001, "dups17"), ("T3", "s40", 70001, "dups257"), ("T4", "acgtn", 70001, "over46"),
            ("T4", "acgtn", 70001, "over257"), ("M1", "s12", 4097, "run0_v13"), ("M2", "acgtn", 70001, "no_nothing"),
            ("M2", "b256", 70001, "no_nothing"), ("M4", "s12", 4097, "n_too_small"), ("M4", "s12", 4097, "n_too_large")]
    out = []
    for fam, name, n, cid in pick:
        blk, exp = [(b, e) for i, b, e in B.cases(fam, name, n) if i == cid][0]
        out.append(("%s %s-%d %s" % (fam, name, n, cid), blk, exp))
    for name, n in (("b256", 70001), ("late", 70001), ("acgtn", 70001)):      # T5: a primary the header can hold
        cid, blk, exp = [c for c in B.cases("T5", name, n) if c[0] == "p%d" % (B.base_block(name, n)["primary"] + 1)][0]
        out.append(("T5 %s-%d %s" % (name, n, cid), blk, exp))
    for name, n in (("acgtn", 70001), ("b256", 70001), ("s12", 4097)):        # M2 / M3: one refused, one decoded
        for fam in ("M2", "M3"):
            cs = B.cases(fam, name, n)
            for want in (True, False):
                hit = [c for c in cs if (c[2] == B.MALFORMED) == want and c[0] != "no_nothing"]
                if hit:
                    out.append(("%s %s-%d %s" % (fam, name, n, hit[0][0]), hit[0][1], hit[0][2]))
    return out


def test_through_the_container(ctx, good):
    cs = _container_cases()
    assert sum(e == B.MALFORMED for _, _, e in cs) >= 5 and sum(e != B.MALFORMED for _, _, e in cs) >= 8
    for what, blk, exp in cs:
        _expect(ctx, good, _container, blk, exp, what + " container")


SELECTORS = [{"TC_IBWT_LF": "0"}, {"TC_DECODE_BYTES": "0"}, {"TC_MTF_FORCE_GENERAL": "1"}, {"TC_MTF_SENTINEL_SPLIT": "0"},
             {"TC_MTF_WAVE_CHUNKS": "1"}]


def _selector_params():
    return [pytest.param(f, a, n, id="%s-%s-%d" % (f, a, n)) for f in ("T1", "T2", "T3", "T4", "T5", "M3")
            for a, n in B.FAMILY_BASES[f] if n in B.SELECTOR_LENGTHS]


@pytest.mark.parametrize("family,name,n", _selector_params())
@pytest.mark.parametrize("env", SELECTORS, ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()))
def test_selectors(ctx, good, env, family, name, n, monkeypatch):
    """the same answers on the alternative paths (the library reads the selectors per call)"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for cid, blk, exp in B.cases(family, name, n):
        _check(ctx, good, blk, exp, "%s %s-%d %s" % (family, name, n, cid))
