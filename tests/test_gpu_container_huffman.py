"""Huffman-coded containers (run format id 3, tc_ctx_set_container_coding): what the device writes is judged by the
numpy restatement of the format text (tests/huffman_format.py, pinned by tests/test_huffman_format.py) over the
ORACLE's runs; it round-trips through every container entry point; it is never larger than the packed container and
falls back to it where it would be; the default coding's bytes are untouched; malformed bodies are refused.

The margin of test_compresses_as_well_as_huffman_can: the excess of the coded bits over an optimal Huffman code WITHOUT
a length limit was computed for every text of TEXTS with the restatement's own length builder (package-merge,
L_max = 12) and measured on an MI355X for the library's (the same algorithm on the host): 0.00000 % on all eleven
texts, both builders alike (the longest unlimited code of any of them is 11 bits, bytes256: the limit never binds) --
so m is the floor the rule sets, 0.5 %."""
import ctypes as C
import struct
import threading

import numpy as np
import pytest

import classgen
import huffman_format as H
import oracle as O
from huffman_cases import checksum64 as _checksum64, header as _header, resealed as _resealed, set_coding as _set

pytestmark = pytest.mark.gpu

PACKED, HUFFMAN = 0, 1
HDR = 640
M_EXCESS = 0.005


@pytest.fixture(scope="module")
def ctx():
    import textcomp
    c = textcomp.Context(0)
    yield c
    c.close()


def _texts():
    r = np.random.default_rng(77)
    n = 1 << 20
    out = {}
    for k in (65541, 300001, n + 7):
        out["acgtn_n%d" % k] = O.gen_acgtn(0x77 + k, k)
    for name in ("zipf_words", "ascii96", "bytes256", "genome_like", "dev_runs", "dev_gaps"):
        out[name] = classgen.make(name, n)
    out["long_runs_then_noise"] = np.concatenate([np.full(70000, 71, np.uint8), O.gen_acgtn(5, 50000), np.full(40000, 84, np.uint8)])
    out["sigma7"] = np.frombuffer(b"ABCDEF", np.uint8)[r.integers(0, 6, 50000)]
    return out


TEXTS = _texts()
_ORACLE = {}


def _oracle_block(name):
    if name not in _ORACLE:
        L = O.bwt_encode_arr(TEXTS[name])
        idx, fl = O.mtf_encode_arr(L)
        counts, vals = O.rle_encode_u32_arr(idx)
        _ORACLE[name] = (int(np.nonzero(L < 0)[0][0]), fl, np.asarray(counts, np.int64), np.asarray(vals, np.int64))
    return _ORACLE[name]


def _dev(text):
    import torch
    if len(text) == 0:
        return torch.zeros(16, dtype=torch.uint8, device="cuda")
    return torch.from_numpy(np.ascontiguousarray(text)).cuda()


def _encode_dev(ctx, text, coding):
    """tc_encode_container_dev under `coding` (the context is left PACKED) -> (bytes, device buffer, used)"""
    import torch
    n = len(text)
    d_text = _dev(text)
    bound = int(ctx.lib.tc_container_bound(n + 2, 257))
    buf = torch.full((bound + 64,), 0xAB, dtype=torch.uint8, device="cuda")    # dirty: the call must not rely on zeros
    torch.cuda.synchronize()
    _set(ctx, coding)
    try:
        used = ctx.encode_container_dev(d_text.data_ptr(), n, buf.data_ptr(), bound)
    finally:
        _set(ctx, PACKED)
    return buf[:used].cpu().numpy().tobytes(), buf, used


def _to_block_dev(ctx, d_buf, used, nruns, n):
    """tc_container_to_block_dev + tc_decode_dev -> (rc of the first call, counts, values, text bytes)"""
    import torch
    from textcomp import Block
    o_c = torch.zeros(nruns + 1, dtype=torch.int32, device="cuda")
    o_v = torch.zeros(nruns + 1, dtype=torch.int16, device="cuda")
    d_out = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    blk = Block()
    blk.nruns, blk.run_count, blk.run_value = nruns, o_c.data_ptr(), o_v.data_ptr()
    rc = ctx.lib.tc_container_to_block_dev(ctx.handle, C.c_void_p(d_buf.data_ptr()), used, C.byref(blk))
    if rc != 0:
        return rc, None, None, None
    assert ctx.lib.tc_decode_dev(ctx.handle, C.byref(blk), C.c_void_p(d_out.data_ptr())) == 0, ctx.lib.tc_last_error(ctx.handle)
    return 0, o_c[:nruns].cpu().numpy().view(np.uint32).astype(np.int64), o_v[:nruns].cpu().numpy().astype(np.int64), d_out[:n].cpu().numpy().tobytes()


# ---- 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TEXTS), ids=list(TEXTS))
def test_decodes_to_the_oracles_runs_by_an_independent_reader(ctx, name):
    text = TEXTS[name]
    blob, _, _ = _encode_dev(ctx, text, HUFFMAN)
    primary, fl, counts, vals = _oracle_block(name)
    h = _header(blob)
    assert h["n"] == len(text) and h["primary"] == primary and h["nruns"] == len(counts) and h["sigma"] == len(fl)
    assert list(struct.unpack_from("<%dh" % h["sigma"], blob, 64)) == [int(x) for x in fl]
    assert h["body"] == len(blob) - HDR and h["nesc"] == 0
    assert h["format"] == 3, "a fallback to the packed body here is a failure"
    body = blob[HDR:]
    c, v = H.read_body(body, len(counts), h["sigma"])
    assert np.array_equal(c, counts) and np.array_equal(v, vals)
    K, nchunks, nsyms, lmax = struct.unpack_from("<4I", body, 0)
    lengths = np.frombuffer(body, np.uint8, nsyms, 16)
    assert lmax <= 12 and lengths.max() <= lmax and H.kraft(lengths, lmax) <= 1 << lmax
    assert len(blob) < HDR + H.packed_body_bytes(counts, h["sigma"])
    print("%s: n %d, runs %d, container %d B = %.4f B/B (packed body %d B)" % (name, len(text), len(counts), len(blob), len(blob) / len(text), H.packed_body_bytes(counts, h["sigma"])))


# ---- 2 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["acgtn_n300001", "zipf_words", "bytes256", "dev_gaps", "sigma7"])
def test_round_trip_device_and_host(ctx, name):
    import textcomp
    text = TEXTS[name]
    blob, d_buf, used = _encode_dev(ctx, text, HUFFMAN)
    _, _, counts, vals = _oracle_block(name)
    rc, c, v, back = _to_block_dev(ctx, d_buf, used, len(counts), len(text))
    assert rc == 0, ctx.lib.tc_last_error(ctx.handle)
    assert np.array_equal(c, counts) and np.array_equal(v, vals) and back == text.tobytes()
    host = ctx.encode_container(text, coding="huffman")
    assert ctx.container_coding == "packed"                  # the keyword restores the context's value
    assert host == blob
    assert textcomp.container_coding(host) == "huffman"
    assert ctx.decode_container(host) == text.tobytes()
    # tc_block_to_container_dev from a block made by tc_encode_dev: the one-call container's bytes
    import torch
    from textcomp import Block
    n = len(text)
    d_text = _dev(text)
    d_c = torch.empty(n + 2, dtype=torch.int32, device="cuda")
    d_v = torch.empty(n + 2, dtype=torch.int16, device="cuda")
    blk = Block()
    blk.nruns, blk.run_count, blk.run_value = n + 2, d_c.data_ptr(), d_v.data_ptr()
    assert ctx.lib.tc_encode_dev(ctx.handle, C.c_void_p(d_text.data_ptr()), n, C.byref(blk)) == 0
    bound = int(ctx.lib.tc_container_bound(n + 2, 257))
    b = torch.full((bound + 64,), 0xCD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ub = C.c_uint64(bound)
    _set(ctx, HUFFMAN)
    try:
        assert ctx.lib.tc_block_to_container_dev(ctx.handle, C.byref(blk), C.c_void_p(b.data_ptr()), C.byref(ub)) == 0
    finally:
        _set(ctx, PACKED)
    assert b[:ub.value].cpu().numpy().tobytes() == blob


def test_round_trip_stream_and_mixed_codings(ctx):
    import textcomp
    text = np.concatenate([TEXTS["acgtn_n300001"], TEXTS["ascii96"][:250000], TEXTS["sigma7"]])   # 600 001 bytes
    block = 250000                                                                              # 3 records, a short last one
    s_h = ctx.encode_stream(text, block, coding="huffman")
    s_p = ctx.encode_stream(text, block)
    assert ctx.stream_info(s_h) == (len(text), 3) and len(s_h) < len(s_p)
    assert ctx.decode_stream(s_h) == text.tobytes()
    # records of both codings in one stream: readers go by each header
    def split(s):
        out, off = [], 0
        while off < len(s):
            ln = HDR + _header(s[off:])["body"]
            out.append(s[off:off + ln])
            off += ln
        return out
    rh, rp = split(s_h), split(s_p)
    assert [textcomp.container_coding(r) for r in rh] == ["huffman"] * 3
    assert [textcomp.container_coding(r) for r in rp] == ["packed"] * 3
    mixed = rh[0] + rp[1] + rh[2]
    assert ctx.stream_info(mixed) == (len(text), 3)
    assert ctx.decode_stream(mixed) == text.tobytes()
    assert ctx.decode_stream(rp[0] + rh[1] + rp[2]) == text.tobytes()


# ---- 3 ------------------------------------------------------------------------------------------------------------------
def _fallback_texts():
    out = {"acgtn_n%d" % n: O.gen_acgtn(0x77 + n, n) for n in (0, 1, 2, 15, 33, 257)}
    out["unary_100k"] = np.full(100000, 65, np.uint8)
    return out


FALLBACK = _fallback_texts()


@pytest.mark.parametrize("name", list(FALLBACK), ids=list(FALLBACK))
def test_never_larger_small_records_stay_packed(ctx, name):
    """head, length table and directory alone outweigh the packed body of these: byte-identical to the packed container"""
    text = FALLBACK[name]
    a, d_buf, used = _encode_dev(ctx, text, HUFFMAN)
    b, _, _ = _encode_dev(ctx, text, PACKED)
    assert a == b
    h = _header(a)
    assert h["format"] == (0 if h["sigma"] <= 6 else 1 if h["sigma"] <= 16 else 2)
    if len(text):
        rc, _, _, back = _to_block_dev(ctx, d_buf, used, int(h["nruns"]), len(text))
        assert rc == 0 and back == text.tobytes()


def test_block_with_a_zero_count_is_packed(ctx):
    import torch
    from textcomp import Block
    r = np.random.default_rng(3)
    nr = 50000
    counts = r.integers(1, 4, nr).astype(np.uint32)
    counts[12345] = 0
    vals = r.integers(0, 6, nr).astype(np.uint16)
    d_c, d_v = torch.from_numpy(counts.view(np.int32)).cuda(), torch.from_numpy(vals.view(np.int16)).cuda()
    blk = Block()
    blk.n, blk.primary, blk.sigma, blk.nruns = int(counts.sum()) - 1, 5, 6, nr
    blk.run_count, blk.run_value = d_c.data_ptr(), d_v.data_ptr()
    bound = int(ctx.lib.tc_container_bound(nr, 6))
    outs = []
    for coding in (HUFFMAN, PACKED):
        buf = torch.full((bound + 64,), 0xEE, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        used = C.c_uint64(bound)
        _set(ctx, coding)
        try:
            assert ctx.lib.tc_block_to_container_dev(ctx.handle, C.byref(blk), C.c_void_p(buf.data_ptr()), C.byref(used)) == 0
        finally:
            _set(ctx, PACKED)
        outs.append(buf[:used.value].cpu().numpy().tobytes())
    assert outs[0] == outs[1] and _header(outs[0])["format"] == 0
    # the same block without the zero is Huffman-coded, and smaller
    counts[12345] = 1
    d_c = torch.from_numpy(counts.view(np.int32)).cuda()
    blk.run_count = d_c.data_ptr()
    buf = torch.full((bound + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    used = C.c_uint64(bound)
    _set(ctx, HUFFMAN)
    try:
        assert ctx.lib.tc_block_to_container_dev(ctx.handle, C.byref(blk), C.c_void_p(buf.data_ptr()), C.byref(used)) == 0
    finally:
        _set(ctx, PACKED)
    blob = buf[:used.value].cpu().numpy().tobytes()
    assert _header(blob)["format"] == 3 and len(blob) < len(outs[0])
    c, v = H.read_body(blob[HDR:], nr, 6)
    assert np.array_equal(c, counts.astype(np.int64)) and np.array_equal(v, vals.astype(np.int64))


def test_capacity_report_is_the_bytes_needed(ctx):
    import torch
    text = TEXTS["acgtn_n300001"]
    blob, _, _ = _encode_dev(ctx, text, HUFFMAN)
    d_text = _dev(text)
    small = torch.zeros(HDR + 4096, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    used = C.c_uint64(HDR + 4096)
    _set(ctx, HUFFMAN)
    try:
        rc = ctx.lib.tc_encode_container_dev(ctx.handle, C.c_void_p(d_text.data_ptr()), len(text), C.c_void_p(small.data_ptr()), C.byref(used))
        assert rc == -2 and used.value == len(blob)
        exact = torch.zeros(len(blob) + 16, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert ctx.encode_container_dev(d_text.data_ptr(), len(text), exact.data_ptr(), len(blob)) == len(blob)
        assert exact[:len(blob)].cpu().numpy().tobytes() == blob
    finally:
        _set(ctx, PACKED)


# ---- 4 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TEXTS), ids=list(TEXTS))
def test_compresses_as_well_as_huffman_can(ctx, name):
    blob, _, _ = _encode_dev(ctx, TEXTS[name], HUFFMAN)
    _, fl, counts, vals = _oracle_block(name)
    sigma = len(fl)
    hist = H.histogram(counts, vals, sigma)
    best = H.optimal_huffman_bits(hist)
    body = blob[HDR:]
    K, nchunks, nsyms, lmax = struct.unpack_from("<4I", body, 0)
    doff = 16 + ((nsyms + 15) & ~15)
    chunk_bits = np.frombuffer(body, "<u4", nchunks, doff).astype(np.int64)
    payload_bits = 32 * int(((chunk_bits + 31) // 32).sum())
    lengths = np.frombuffer(body, np.uint8, nsyms, 16).astype(np.int64)
    own = H.build_lengths(hist, lmax).astype(np.int64)
    print("%s: optimal %d bits; library lengths %+.5f %%, restatement's builder %+.5f %%; payload %d bits in %d chunks"
          % (name, best, 100.0 * (int((hist * lengths).sum()) - best) / best, 100.0 * (int((hist * own).sum()) - best) / best,
             payload_bits, nchunks))
    assert int(chunk_bits.sum()) == int((hist * lengths).sum())
    assert payload_bits <= best * (1 + M_EXCESS) + 32 * nchunks


# ---- 5 ------------------------------------------------------------------------------------------------------------------
def test_default_is_untouched(ctx):
    import textcomp
    import torch
    texts = [TEXTS["acgtn_n65541"], TEXTS["sigma7"], TEXTS["ascii96"][:120000]]
    with textcomp.Context(0) as fresh:
        assert fresh.lib.tc_ctx_get_container_coding(fresh.handle) == 0 and fresh.container_coding == "packed"
        first = [_encode_dev(fresh, t, PACKED)[0] for t in texts]
        _set(fresh, HUFFMAN)
        assert fresh.lib.tc_ctx_get_container_coding(fresh.handle) == 1
        assert fresh.lib.tc_ctx_set_container_coding(fresh.handle, 2) == -1 and fresh.lib.tc_ctx_set_container_coding(fresh.handle, -1) == -1
        assert fresh.lib.tc_ctx_get_container_coding(fresh.handle) == 1
        # a failed call (capacity 0) does not change the setting
        d_text = _dev(texts[0])
        buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        used = C.c_uint64(0)
        assert fresh.lib.tc_encode_container_dev(fresh.handle, C.c_void_p(d_text.data_ptr()), len(texts[0]), C.c_void_p(buf.data_ptr()), C.byref(used)) == -2
        assert fresh.lib.tc_ctx_get_container_coding(fresh.handle) == 1
        huff = [_encode_dev(fresh, t, HUFFMAN)[0] for t in texts]      # (leaves the context PACKED)
        assert fresh.lib.tc_ctx_get_container_coding(fresh.handle) == 0
        again = [_encode_dev(fresh, t, PACKED)[0] for t in texts]
    assert first == again
    assert [_header(b)["format"] for b in first] == [0, 1, 2]
    assert [_header(b)["format"] for b in huff] == [3, 3, 3]
    assert all(len(h) < len(p) for h, p in zip(huff, first))


def test_two_contexts_two_codings_two_threads(ctx):
    import textcomp
    import torch
    text = TEXTS["acgtn_n300001"]
    want = {PACKED: _encode_dev(ctx, text, PACKED)[0], HUFFMAN: _encode_dev(ctx, text, HUFFMAN)[0]}
    d_text = _dev(text)
    bound = int(ctx.lib.tc_container_bound(len(text) + 2, 257))
    bufs = {c: torch.zeros(bound + 64, dtype=torch.uint8, device="cuda") for c in want}
    torch.cuda.synchronize()
    ctxs = {c: textcomp.Context(0) for c in want}
    got, errs = {c: [] for c in want}, []
    for c in want:
        _set(ctxs[c], c)

    def work(c):
        try:
            for _ in range(4):
                used = ctxs[c].encode_container_dev(d_text.data_ptr(), len(text), bufs[c].data_ptr(), bound)
                got[c].append(bufs[c][:used].cpu().numpy().tobytes())
        except Exception as e:      # noqa: BLE001
            errs.append(e)
    th = [threading.Thread(target=work, args=(c,)) for c in want]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for c in want:
        assert ctxs[c].lib.tc_ctx_get_container_coding(ctxs[c].handle) == c
        ctxs[c].close()
    assert not errs, errs
    for c in want:
        assert got[c] == [want[c]] * 4


# ---- 6 ------------------------------------------------------------------------------------------------------------------
def test_malformed_bodies_are_refused(ctx):
    import torch
    text = TEXTS["acgtn_n65541"]
    good, _, _ = _encode_dev(ctx, text, HUFFMAN)
    h = _header(good)
    assert h["format"] == 3 and _checksum64(good[HDR:]) == h["checksum"]
    sigma, nruns = h["sigma"], int(h["nruns"])
    body = good[HDR:]
    K, nchunks, nsyms, lmax = struct.unpack_from("<4I", body, 0)
    assert nchunks > 8
    doff = 16 + ((nsyms + 15) & ~15)
    poff = doff + ((4 * nchunks + 15) & ~15)
    lengths = np.frombuffer(body, np.uint8, nsyms, 16)
    codes = H.canonical_codes(lengths)

    def edit(fn, extra=0):
        b = bytearray(body) + bytearray(extra)
        fn(b)
        return _resealed(good, b)

    def put32(off, val):
        return lambda b: struct.pack_into("<I", b, off, val & 0xFFFFFFFF)

    def first_token_is_a_digit(b):
        # the first code of the payload replaced by RUNA's, left-aligned in the first word (the rest of the word zero)
        struct.pack_into("<I", b, poff, int(codes[sigma]) << (32 - int(lengths[sigma])))
    assert lengths[sigma] > 0
    last = doff + 4 * (nchunks - 1)
    last_bits = struct.unpack_from("<I", body, last)[0]
    cases = {
        "length above L_max": edit(lambda b: b.__setitem__(16, lmax + 1)),
        "Kraft sum above 1": edit(lambda b: b.__setitem__(slice(16, 16 + nsyms), bytes([1] * nsyms))),
        "nsyms != sigma + 2": edit(put32(8, nsyms + 1)),
        "directory entry one word short": edit(put32(last, last_bits - 32)),
        "directory entry one word long": edit(put32(last, last_bits + 32)),
        "first directory entry one word long": edit(put32(doff, struct.unpack_from("<I", body, doff)[0] + 32)),
        "nchunks + 1": edit(put32(4, nchunks + 1)),
        "nchunks - 1": edit(put32(4, nchunks - 1)),
        "first token is a digit": edit(first_token_is_a_digit),
        "K = 0": edit(put32(0, 0)),
        "K = 3": edit(put32(0, 3)),
        "K = 2048": edit(put32(0, 2048)),
        "L_max = 0": edit(put32(12, 0)),
        "L_max = 13": edit(put32(12, 13)),
        "a directory entry of 2^32 - 1 bits": edit(put32(doff + 8, 0xFFFFFFFF)),
        "16 bytes more payload": edit(lambda b: None, extra=16),
        "truncated payload": _resealed(good, body[:-16]),
        "format = 4": bytes(bytearray(good[:60]) + struct.pack("<I", 4) + bytearray(good[64:])),
    }
    flipped = bytearray(good)
    flipped[HDR + poff + 40] ^= 0x10
    cases["a flipped payload bit (checksum not recomputed)"] = bytes(flipped)
    for what, blob in cases.items():
        assert len(blob) % 16 == 0, what
        d = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).cuda()
        torch.cuda.synchronize()
        rc, _, _, _ = _to_block_dev(ctx, d, len(blob), nruns, len(text))
        assert rc == -3, (what, rc, ctx.lib.tc_last_error(ctx.handle))
        with pytest.raises(Exception) as ei:
            ctx.decode_container(blob)
        assert getattr(ei.value, "code", None) == -3, what
        # a good container decodes on the same context straight after
        d = torch.from_numpy(np.frombuffer(good, np.uint8).copy()).cuda()
        torch.cuda.synchronize()
        rc, _, _, back = _to_block_dev(ctx, d, len(good), nruns, len(text))
        assert rc == 0 and back == text.tobytes(), what
    import textcomp
    with pytest.raises(textcomp.TcMalformed):
        textcomp.container_coding(cases["format = 4"])


# ---- 7 ------------------------------------------------------------------------------------------------------------------
def test_at_scale_once(ctx):
    import torch
    from textcomp import Block
    n = 1 << 28
    d_text = torch.empty(n, dtype=torch.uint8, device="cuda")
    assert ctx.lib.tc_generate_dev(ctx.handle, 0, 0xC2, n, C.c_void_p(d_text.data_ptr())) == 0
    cap = n // 2 + 4096
    buf = torch.empty(cap, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    _set(ctx, HUFFMAN)
    try:
        used = ctx.encode_container_dev(d_text.data_ptr(), n, buf.data_ptr(), cap)
    finally:
        _set(ctx, PACKED)
    h = _header(buf[:HDR].cpu().numpy().tobytes())
    assert h["format"] == 3 and h["n"] == n
    print("2^28 iid ACGTN: Huffman container %d bytes = %.4f bytes per input byte (%d runs)" % (used, used / n, h["nruns"]))
    assert used < 0.40 * n      # (the packed container of this record: 0.42 n)
    k = int(h["nruns"])
    o_c = torch.empty(k + 1, dtype=torch.int32, device="cuda")
    o_v = torch.empty(k + 1, dtype=torch.int16, device="cuda")
    blk = Block()
    blk.nruns, blk.run_count, blk.run_value = k, o_c.data_ptr(), o_v.data_ptr()
    assert ctx.lib.tc_container_to_block_dev(ctx.handle, C.c_void_p(buf.data_ptr()), used, C.byref(blk)) == 0, ctx.lib.tc_last_error(ctx.handle)
    del buf
    back = torch.empty(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert ctx.lib.tc_decode_dev(ctx.handle, C.byref(blk), C.c_void_p(back.data_ptr())) == 0, ctx.lib.tc_last_error(ctx.handle)
    assert torch.equal(back, d_text)
