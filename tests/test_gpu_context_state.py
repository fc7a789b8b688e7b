"""One context, many calls: what a context keeps from one call to the next (the workspace, carved differently by
size and grown in place; the reused slots of its host scalars; the device error word; the sticky single-ticket
mode) must never change a result.  One scripted sequence walks sizes and paths up and down on ONE context with
failing calls in between; every step must equal the oracle (or, for the 2^27 record, the oracle's digest), every
failing call must return its code and leave a message, and the call after it must be exact.  tc_stats describes
the last encode alone: the path tests read msd_path, msd_keyonly, seg_rounds, chain_rounds and finish_pass as
evidence of which path ran, so no field may survive from an earlier call.

The ticket redo: round 0's radix passes draw XCD-grouped tile tickets; if a look-back spin runs out there, the
suffix sort is redone with the single counter and the context keeps that mode (csrc/tc_sa_host.hpp,
ticket_check).  TC_DBG_TICKET_TRIP=1 makes the first attempt's check find the flag set, so the redo runs on the
spent attempt's buffers and counters."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
from test_gpu_fullsize import DIGESTS, _assert_digest

pytestmark = pytest.mark.gpu

PATH_FIELDS = ("msd_path", "msd_keyonly", "seg_rounds", "chain_rounds", "finish_pass")


def _oracle_block(text):
    L = O.bwt_encode_arr(text)
    idx, fl = O.mtf_encode_arr(L)
    counts, vals = O.rle_encode_u32_arr(idx)
    return int(np.nonzero(L < 0)[0][0]), fl.tolist(), counts.tolist(), vals.tolist()


def _same(blk, exp):
    prim, fl, counts, vals = exp
    assert blk["primary"] == prim and blk["final_list"].tolist() == fl
    assert blk["run_count"].tolist() == counts and blk["run_value"].tolist() == vals


def _fresh_stats(ctx, n, **fields):
    """the stats of the last encode describe it alone: its size, the given path fields, nothing past its rounds"""
    st = ctx.stats()
    assert st.n == n and st.N == (n + 1 if n else 0)
    for k, v in fields.items():
        assert getattr(st, k) == v, (k, getattr(st, k), v)
    for r in range(st.rounds, len(st.m)):
        assert st.m[r] == 0 and st.passes[r] == 0 and st.key_bytes[r] == 0 and st.h[r] == 0, r
    return st


def _failed(ctx, exc, code):
    assert exc.value.code == code, (exc.value.code, code)
    assert ctx.lib.tc_last_error(ctx.handle) != b""


def _big(ctx, n):
    """the 2^27-suffix record by tc_encode_dev (the MSD way by default) against the oracle's digest"""
    import torch
    from textcomp import Block
    d = DIGESTS["n%d" % n]
    lib = ctx.lib
    t = torch.empty(n, dtype=torch.uint8, device="cuda")
    assert lib.tc_generate_dev(ctx.handle, 0, d["seed"], n, C.c_void_p(t.data_ptr())) == 0
    cnt = torch.empty(n + 2, dtype=torch.int32, device="cuda")
    val = torch.empty(n + 2, dtype=torch.int16, device="cuda")
    blk = Block()
    blk.nruns, blk.run_count, blk.run_value = n + 2, cnt.data_ptr(), val.data_ptr()
    ctx._check(lib.tc_encode_dev(ctx.handle, C.c_void_p(t.data_ptr()), n, C.byref(blk)))
    st = _fresh_stats(ctx, n, msd_path=1)
    _assert_digest(lib, ctx, d, blk, cnt, val, t)
    return st


def test_one_context_many_calls():
    import textcomp
    from textcomp import TcError, TcMalformed, _lib
    ctx = textcomp.Context(0)
    lib = ctx.lib
    t20 = O.gen_acgtn(0xC2, 1 << 20)
    e20 = _oracle_block(t20)
    t16 = O.gen_ascii(0xE1, 1 << 16)
    e16 = _oracle_block(t16)
    t257 = np.tile(np.arange(256, dtype=np.uint8), 600)
    t257[::97] = O.gen_acgtn(0xE2, len(t257[::97]))                  # all 256 byte values + the sentinel, long repeats
    e257 = _oracle_block(t257)
    big = (1 << 27) - 1                                              # N = 2^27: the MSD way (tests/test_gpu_fullsize.py)

    # 1. LSD way
    blk20 = ctx.encode(t20)
    _same(blk20, e20)
    _fresh_stats(ctx, 1 << 20, msd_path=0, msd_keyonly=0, finish_pass=1)
    with pytest.raises(TcError) as e:                                # capacity: encode
        ctx.encode(t20, cap=100)
    _failed(ctx, e, _lib.TC_ERR_CAPACITY)
    # 2. MSD way: the workspace grows, the MSD tables are carved
    st = _big(ctx, big)
    assert st.msd_keyonly == 1
    with pytest.raises(TcError) as e:                                # capacity: container
        ctx.encode_container(t16, cap=700)
    _failed(ctx, e, _lib.TC_ERR_CAPACITY)
    # 3. a small record on the grown workspace, carved without the MSD tables
    _same(ctx.encode(t16), e16)
    _fresh_stats(ctx, 1 << 16, msd_path=0, msd_keyonly=0)
    prim = C.c_uint64()
    assert lib.tc_bwt_encode(ctx.handle, None, 10, None, C.byref(prim)) == _lib.TC_ERR_ARG
    assert lib.tc_last_error(ctx.handle) != b""
    # 4. sigma = 257
    blk257 = ctx.encode(t257)
    _same(blk257, e257)
    assert blk257["sigma"] == 257
    _fresh_stats(ctx, len(t257), msd_path=0, msd_keyonly=0)
    assert ctx.decode(blk257) == t257.tobytes()
    blob = bytearray(ctx.encode_container(t16))                      # a flipped payload byte
    blob[len(blob) // 2] ^= 0x10
    with pytest.raises(TcMalformed) as e:
        ctx.decode_container(bytes(blob))
    _failed(ctx, e, _lib.TC_ERR_MALFORMED)
    # 5. the empty text, then n = 1
    blk0 = ctx.encode(b"")
    assert blk0["n"] == 0 and len(blk0["run_count"]) == 0
    _fresh_stats(ctx, 0, **{k: 0 for k in PATH_FIELDS})
    _same(ctx.encode(b"q"), _oracle_block(np.frombuffer(b"q", np.uint8)))
    _fresh_stats(ctx, 1, msd_path=0, msd_keyonly=0, seg_rounds=0, chain_rounds=0)
    idx, fl = O.mtf_encode_arr(O.bwt_encode_arr(t16))                # an index out of range: the device flag
    idx = idx.astype(np.uint16)
    idx[len(idx) // 3] = len(fl) + 3
    with pytest.raises(TcMalformed) as e:
        ctx.mtf_decode(idx, fl)
    _failed(ctx, e, _lib.TC_ERR_MALFORMED)
    # 6. FM index
    fm = ctx.fm_build(t16)
    ofm = O.FMIndex(t16)
    pats = [t16[i:i + k].tobytes() for i, k in ((0, 3), (400, 5), (9000, 2), (60000, 9))] + [b"\x01\x02"]
    assert [int(v) or None for v in fm.count(pats)] == [ofm.count(p) for p in pats]
    assert [h.tolist() for h in fm.locate(pats)] == [ofm.locate(p) for p in pats]
    fm.close()
    rng = np.random.default_rng(9)                                   # Q9: bwt_decode_sym on a non-BWT sequence
    for _ in range(100):                                             # (two Nothings: the walk meets the second one)
        x = rng.integers(0, 4, 3000).astype(np.int16)
        x[rng.integers(0, 3000, 2)] = -1
        try:
            O.bwt_decode_arr(x)
        except O.OracleMalformed:
            break
    else:
        raise AssertionError("no malformed sequence drawn")
    with pytest.raises(TcMalformed) as e:
        ctx.bwt_decode_sym(x)
    _failed(ctx, e, _lib.TC_ERR_MALFORMED)
    # 7. decode of step 1's block
    assert ctx.decode(blk20) == t20.tobytes()
    # 8. step 1 again, byte-identical
    again = ctx.encode(t20)
    for k in ("primary", "sigma"):
        assert again[k] == blk20[k]
    for k in ("final_list", "run_count", "run_value"):
        assert again[k].tobytes() == blk20[k].tobytes()
    _fresh_stats(ctx, 1 << 20, msd_path=0, msd_keyonly=0, finish_pass=1)
    # 9. step 2 again
    _big(ctx, big)
    ctx.close()


@pytest.mark.parametrize("case", ["lsd_1mib", "lsd_16mib", "msd_forced", "suffix_array"])
def test_ticket_redo(case, monkeypatch):
    """the redo of the suffix sort with the single ticket counter, on the spent first attempt's buffers"""
    import torch
    import textcomp
    from textcomp import Block
    ctx = textcomp.Context(0)
    monkeypatch.setenv("TC_DBG_TICKET_TRIP", "1")
    t20 = O.gen_acgtn(0xC2, 1 << 20)
    if case == "lsd_1mib":
        _same(ctx.encode(t20), _oracle_block(t20))
        assert ctx.stats().msd_path == 0
        fallbacks = 1
    elif case == "lsd_16mib":
        n = 1 << 24
        d = DIGESTS["n%d" % n]
        lib = ctx.lib
        t = torch.empty(n, dtype=torch.uint8, device="cuda")
        assert lib.tc_generate_dev(ctx.handle, 0, d["seed"], n, C.c_void_p(t.data_ptr())) == 0
        cnt = torch.empty(n + 2, dtype=torch.int32, device="cuda")
        val = torch.empty(n + 2, dtype=torch.int16, device="cuda")
        blk = Block()
        blk.nruns, blk.run_count, blk.run_value = n + 2, cnt.data_ptr(), val.data_ptr()
        ctx._check(lib.tc_encode_dev(ctx.handle, C.c_void_p(t.data_ptr()), n, C.byref(blk)))
        assert ctx.stats().msd_path == 0 and ctx.stats().ticket_fallbacks == 1
        _assert_digest(lib, ctx, d, blk, cnt, val, t)
        fallbacks = 1
    elif case == "msd_forced":
        # the MSD way's partition levels draw no tile tickets (tc_msd.hpp): round 0 has nothing to redo there
        monkeypatch.setenv("TC_SA_MSD_MIN_LOG2", "10")
        _same(ctx.encode(t20), _oracle_block(t20))
        assert ctx.stats().msd_path == 1
        fallbacks = 0
    else:
        t = O.gen_ascii(0xE3, 300000)
        assert ctx.suffix_array(t).tolist() == O.suffix_array(t).tolist()
        fallbacks = 1
    assert ctx.stats().ticket_fallbacks == fallbacks
    # later calls on the same context: still exact, the context keeps its mode (no second redo)
    monkeypatch.delenv("TC_SA_MSD_MIN_LOG2", raising=False)
    t2 = O.gen_ascii(0xE4, 1 << 20)
    blk = ctx.encode(t2)
    _same(blk, _oracle_block(t2))
    assert ctx.stats().ticket_fallbacks == 1
    assert ctx.decode(blk) == t2.tobytes()
    ctx.close()
