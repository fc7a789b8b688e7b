"""The Huffman container kernels (run format id 3, csrc/tc_huff.hpp) on run lists NO TEXT PRODUCES.  The run lists of
tests/test_gpu_container_huffman.py all come from BWT -> MTF -> RLE of a text: counts of 1..4, chunks of a few thousand
bits, a mild token histogram, and -- on the read side -- only bodies this library wrote (K = 1024, L_max = 12, a
complete code).  Here the blocks are synthetic (tests/huffman_cases.py), handed to tc_block_to_container_dev and taken
back by tc_container_to_block_dev with a small fixed n and primary (the container layer checks their ranges only);
none of them is ever passed to tc_decode_dev.

A  the writer, byte for byte against the numpy restatement (tests/huffman_format.py): chunks of several LDS windows,
   31-digit counts, histograms on which the length limit binds, one and two coded tokens, the format boundaries of
   sigma, chunk-count edges, a directory scan of two turns, and the never-larger decision on both of its sides.  Every
   case first asserts ON THE CPU that it reaches the regime it is named for.
B  the reader on bodies the restatement wrote: K from 1 to above nruns, L_max from 1 to 12, incomplete codes.
C  the same verdict as the restatement on a fixed, seeded list of single mutations of three bodies.

Part A's equality of the coded size (sum of hist x length, the device's lengths against the restatement's) has no
tolerance because both builders are optimal under the limit; tests/test_huffman_format.py checks the restatement's
builder exhaustively on small cases."""
import ctypes as C
import struct

import numpy as np
import pytest

import huffman_cases as S
import huffman_format as H
import oracle as O
from huffman_cases import HDR, HUFFMAN, PACKED

pytestmark = pytest.mark.gpu

N_FIXED, PRIMARY_FIXED = 1000, 7      # header fields of every synthetic block: in range, related to nothing


@pytest.fixture(scope="module")
def ctx():
    import textcomp
    c = textcomp.Context(0)
    yield c
    c.close()


class _DevBlock:
    """a tc_block over device copies of (counts, vals)"""

    def __init__(self, counts, vals, sigma):
        import torch
        from textcomp import Block
        self.nruns, self.sigma = len(counts), sigma
        self.d_c = torch.from_numpy(np.asarray(counts, np.int64).astype(np.uint32).view(np.int32)).cuda()
        self.d_v = torch.from_numpy(np.asarray(vals, np.int64).astype(np.uint16).view(np.int16)).cuda()
        self.final_list = [(7 * i + 3) % 251 for i in range(sigma)]
        b = Block()
        b.n, b.primary, b.sigma, b.nruns = N_FIXED, PRIMARY_FIXED, sigma, self.nruns
        for i, x in enumerate(self.final_list):
            b.final_list[i] = x
        b.run_count, b.run_value = self.d_c.data_ptr(), self.d_v.data_ptr()
        self.blk = b
        torch.cuda.synchronize()


def _write(ctx, db, coding, cap=None, fill=0xAB):
    """tc_block_to_container_dev under `coding` into a dirty buffer (the context is left PACKED) -> (rc, bytes reported,
    container bytes or None, device buffer)"""
    import torch
    bound = int(ctx.lib.tc_container_bound(db.nruns, db.sigma))
    buf = torch.full((bound + 64,), fill, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    used = C.c_uint64(bound if cap is None else cap)
    S.set_coding(ctx, coding)
    try:
        rc = ctx.lib.tc_block_to_container_dev(ctx.handle, C.byref(db.blk), C.c_void_p(buf.data_ptr()), C.byref(used))
    finally:
        S.set_coding(ctx, PACKED)
    blob = buf[:used.value].cpu().numpy().tobytes() if rc == 0 else None
    if rc == 0:
        # the capacity offered is the writer's to use: the nibble packer zeroes its worst case (two nibbles per run)
        # before it packs, so a PACKED container may be followed by zeros inside the capacity.  A Huffman body is
        # written to its size and no further; nothing is ever written behind the capacity.
        cap_end = used.value if S.header(blob)["format"] == 3 else (bound if cap is None else cap)
        assert (buf[cap_end:] == fill).all().item(), "bytes behind the container (format 3) or behind the capacity were written"
    return rc, used.value, blob, buf


def _read(ctx, d_buf, used, nruns):
    """tc_container_to_block_dev alone -> (rc, block, counts, values)"""
    import torch
    from textcomp import Block
    o_c = torch.zeros(nruns + 1, dtype=torch.int32, device="cuda")
    o_v = torch.zeros(nruns + 1, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    blk = Block()
    blk.nruns, blk.run_count, blk.run_value = nruns, o_c.data_ptr(), o_v.data_ptr()
    rc = ctx.lib.tc_container_to_block_dev(ctx.handle, C.c_void_p(d_buf.data_ptr()), used, C.byref(blk))
    if rc != 0:
        return rc, None, None, None
    assert o_c[nruns].item() == 0 and o_v[nruns].item() == 0, "a run behind the last one was written"
    return 0, blk, o_c[:nruns].cpu().numpy().view(np.uint32).astype(np.int64), o_v[:nruns].cpu().numpy().view(np.uint16).astype(np.int64)


def _read_bytes(ctx, blob, nruns):
    import torch
    d = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return _read(ctx, d, len(blob), nruns)


def _check_block_header(db, blk):
    assert (blk.n, blk.primary, blk.sigma, blk.nruns) == (N_FIXED, PRIMARY_FIXED, db.sigma, db.nruns)
    assert list(blk.final_list[:db.sigma]) == db.final_list


# ---- A: the writer ----------------------------------------------------------------------------------------------------
def _edge_runs(nruns):
    return S.mild(1000 + nruns, nruns, 9)


def _big():
    r = np.random.default_rng(9)
    n = S.SCAN_TURN * H.K_DEFAULT + 1025
    return r.integers(1, 4, n).astype(np.int64), r.integers(0, 6, n).astype(np.int64), 6


# name -> (generator, check of the regime on the result of S.regime; a failure of it is a failure of the GENERATOR)
HUFFMAN_CASES = {
    "fibonacci_sigma24": (lambda: S.fib_values(22, 24, 1), lambda c, g: g["unlimited_depth"] > 12 and g["longest"] == 12 and g["limited_bits"] > g["unlimited_bits"]),
    "fibonacci_all_259_tokens": (lambda: S.fib_all_tokens(2), lambda c, g: g["coded"] == 259 and g["unlimited_depth"] > 12 and g["longest"] == 12 and g["limited_bits"] > g["unlimited_bits"]),
    "chunk_of_three_windows": (lambda: S.long_chunk(3), lambda c, g: g["chunk_words"][1] > 2 * S.IMG_WORDS and g["straddlers"] >= 2 and g["chunk_words"][0] < S.IMG_WORDS and g["chunk_words"][2:].max() < S.IMG_WORDS and len(g["chunk_words"]) > 3),
    "every_digit_count": (lambda: S.every_digit_count(4), lambda c, g: set(S.ndigits(c).tolist()) == set(range(32)) and int(c.max()) == S.U32_MAX and all(x in set(c.tolist()) for k in range(2, 32) for x in ((1 << k) - 1, 1 << k, (1 << k) + 1))),
    "rare_runa_12_bits": (lambda: S.rare_digit(5, 0), lambda c, g: g["lengths"][17] == 12 and g["max_thread_bits"] > 4 * 31 * 12 and g["max_thread_bits"] > 64 * 20),
    "rare_runb_12_bits": (lambda: S.rare_digit(6, 1), lambda c, g: g["lengths"][18] == 12 and g["max_thread_bits"] > 4 * 31 * 12),
    "single_token_sigma1": (lambda: S.single_token(5000, 1), lambda c, g: g["coded"] == 1 and g["lengths"].tolist() == [1, 0, 0]),
    "single_token_sigma2": (lambda: S.single_token(5000, 2), lambda c, g: g["coded"] == 1 and g["lengths"].tolist() == [1, 0, 0, 0]),
    "two_tokens": (lambda: S.two_tokens(7), lambda c, g: g["coded"] == 2 and g["longest"] == 1),
    "two_tokens_value_and_runa": (lambda: (1 + (np.arange(5000) % 3 == 0).astype(np.int64), np.zeros(5000, np.int64), 1), lambda c, g: g["coded"] == 2 and g["hist"][1] > 0),
    "sigma6": (lambda: S.mild(16, 30000, 6), lambda c, g: (c >= 5).any()),
    "sigma7": (lambda: S.mild(17, 30000, 7), lambda c, g: (c >= 15).any()),
    "sigma16": (lambda: S.mild(26, 30000, 16), lambda c, g: (c >= 15).any()),
    "sigma17": (lambda: S.mild(27, 30000, 17), lambda c, g: (c >= 127).any()),
    "nruns_3071": (lambda: _edge_runs(3 * 1024 - 1), lambda c, g: len(g["chunk_bits"]) == 3),
    "nruns_3072": (lambda: _edge_runs(3 * 1024), lambda c, g: len(g["chunk_bits"]) == 3),
    "nruns_3073": (lambda: _edge_runs(3 * 1024 + 1), lambda c, g: len(g["chunk_bits"]) == 4 and g["chunk_bits"][3] <= 12 * 32),
    "directory_scan_of_two_turns": (_big, lambda c, g: len(g["chunk_bits"]) > S.SCAN_TURN + 1),
}


@pytest.mark.parametrize("name", list(HUFFMAN_CASES), ids=list(HUFFMAN_CASES))
def test_writer_matches_the_restatement_byte_for_byte(ctx, name):
    gen, reaches = HUFFMAN_CASES[name]
    counts, vals, sigma = gen()
    nruns = len(counts)
    g = S.regime(counts, vals, sigma)
    assert reaches(counts, g), "the generator no longer reaches the regime this case is named for"
    packed = H.packed_body_bytes(counts, sigma)
    own = H.write_body(counts, vals, sigma)
    assert len(own) < packed, "meant to be Huffman-coded"
    db = _DevBlock(counts, vals, sigma)
    rc, used, blob, d_buf = _write(ctx, db, HUFFMAN)
    assert rc == 0, ctx.lib.tc_last_error(ctx.handle)
    h = S.header(blob)
    body = blob[HDR:]
    print("%s: nruns %d, sigma %d, body %d B against packed %d B, largest chunk %d words, longest code %d (unlimited %d), coded tokens %d, format %d"
          % (name, nruns, sigma, len(body), packed, g["max_chunk_words"], g["longest"], g["unlimited_depth"], g["coded"], h["format"]))
    assert h["format"] == 3, "a fallback to the packed body here is a failure"
    assert (h["n"], h["primary"], h["nruns"], h["sigma"]) == (N_FIXED, PRIMARY_FIXED, nruns, sigma)
    assert h["nesc"] == 0 and h["body"] == len(body) == used - HDR and h["checksum"] == S.checksum64(body)
    assert list(struct.unpack_from("<%dh" % sigma, blob, 64)) == db.final_list
    K, nchunks, nsyms, lmax = struct.unpack_from("<4I", body, 0)
    assert (K, nchunks, nsyms, lmax) == (1024, (nruns + 1023) // 1024, sigma + 2, 12)
    lengths = np.frombuffer(body, np.uint8, nsyms, 16).astype(np.int64)
    assert lengths.max() <= 12 and H.kraft(lengths, 12) <= 1 << 12
    assert ((lengths > 0) == (g["hist"] > 0)).all()
    assert int((g["hist"] * lengths).sum()) == g["limited_bits"], "the device's lengths are not optimal under the limit"
    assert len(body) == len(own)
    want = H.write_body(counts, vals, sigma, lengths=lengths, K=1024, lmax=12)
    if body != want:
        a, b = np.frombuffer(body, np.uint8), np.frombuffer(want, np.uint8)
        bad = np.nonzero(a != b)[0]
        L = S.body_layout(want)
        pytest.fail("%d bytes differ from the restatement's body, first at body offset %d (payload word %d), last at %d"
                    % (len(bad), bad[0], (int(bad[0]) - L["poff"]) // 4, bad[-1]))
    rc, blk, c, v = _read(ctx, d_buf, used, nruns)
    assert rc == 0, ctx.lib.tc_last_error(ctx.handle)
    _check_block_header(db, blk)
    assert np.array_equal(c, counts) and np.array_equal(v, vals)
    # the capacity report names exactly the bytes later used, and those bytes are enough
    rc2, need, _, _ = _write(ctx, db, HUFFMAN, cap=HDR + 32)
    assert rc2 == -2 and need == used
    rc3, used3, blob3, _ = _write(ctx, db, HUFFMAN, cap=used, fill=0x5C)
    assert rc3 == 0 and used3 == used and blob3 == blob


def _tiny(nruns, sigma, escapes=()):
    counts = np.ones(nruns, np.int64)
    for i, c in enumerate(escapes):
        counts[3 + 5 * i] = c
    return counts, np.zeros(nruns, np.int64), sigma


# records of one value token around both comparisons of the never-larger rule: head, lengths and directory are
# 48 bytes at sigma 6 and 7, 64 at sigma 16 and 17; (nruns, sigma, escapes) -> the side the record must fall on
NEVER_LARGER = {
    "sigma6_nruns128_fixed_plus_16_equals_packed": (_tiny(128, 6), False),
    "sigma6_nruns129_body_equals_packed": (_tiny(129, 6), False),
    "sigma6_nruns160_body_equals_packed": (_tiny(160, 6), False),
    "sigma6_nruns161_body_16_below_packed": (_tiny(161, 6), True),
    "sigma6_nruns150_one_escape_body_4_below_packed": (_tiny(150, 6, [9]), True),
    "sigma6_nruns120_four_escapes_body_equals_packed": (_tiny(120, 6, [5, 6, 7, 8]), False),
    "sigma7_nruns56_fixed_plus_16_above_packed": (_tiny(56, 7), False),
    "sigma7_nruns64_body_equals_packed": (_tiny(64, 7), False),
    "sigma7_nruns65_body_8_below_packed": (_tiny(65, 7), True),
    "sigma7_nruns57_one_escape_body_8_below_packed": (_tiny(57, 7, [15]), True),
    "sigma7_nruns57_count_14_is_no_escape": (_tiny(57, 7, [14]), False),
    "sigma16_nruns80_body_equals_packed": (_tiny(80, 16), False),
    "sigma16_nruns81_body_8_below_packed": (_tiny(81, 16), True),
    "sigma17_nruns40_body_equals_packed": (_tiny(40, 17), False),
    "sigma17_nruns41_body_8_below_packed": (_tiny(41, 17), True),
    "sigma17_nruns36_one_escape_body_equals_packed": (_tiny(36, 17, [127]), False),
    "sigma17_nruns37_one_escape_body_8_below_packed": (_tiny(37, 17, [127]), True),
    "sigma17_nruns37_count_126_is_no_escape": (_tiny(37, 17, [126]), False),
    "random_u32_counts_sigma6": (S.random_u32_counts(8), False),
}


@pytest.mark.parametrize("name", list(NEVER_LARGER), ids=list(NEVER_LARGER))
def test_never_larger_on_both_sides_of_the_comparison(ctx, name):
    (counts, vals, sigma), huffman = NEVER_LARGER[name]
    nruns = len(counts)
    packed = H.packed_body_bytes(counts, sigma)
    own = H.write_body(counts, vals, sigma)
    L = S.body_layout(own)
    # the side is the restatement's prediction, and the name says how close to the comparison the record lies
    assert (len(own) < packed) == huffman
    if "body_equals_packed" in name:
        assert len(own) == packed
    if "fixed_plus_16_equals_packed" in name:
        assert L["poff"] + 16 == packed
    if "fixed_plus_16_above_packed" in name:
        assert L["poff"] + 16 > packed
    if "_below_packed" in name:
        assert packed - len(own) == int(name.split("_below_packed")[0].rsplit("_", 1)[1])
    if name.startswith("random_u32"):
        assert L["poff"] + 16 < packed < len(own)       # decided by the second comparison, on the payload's size
    db = _DevBlock(counts, vals, sigma)
    rc, used, blob, d_buf = _write(ctx, db, HUFFMAN)
    assert rc == 0, ctx.lib.tc_last_error(ctx.handle)
    rcp, usedp, blobp, _ = _write(ctx, db, PACKED, fill=0x33)
    assert rcp == 0 and usedp == HDR + packed, "the packed body's size is not what the format text gives"
    h = S.header(blob)
    print("%s: nruns %d, sigma %d, Huffman body %d B against packed %d B -> format %d" % (name, nruns, sigma, len(own), packed, h["format"]))
    if huffman:
        assert h["format"] == 3 and h["nesc"] == 0 and used < usedp and used == HDR + len(own)
        lengths = np.frombuffer(blob, np.uint8, sigma + 2, HDR + 16)
        assert blob[HDR:] == H.write_body(counts, vals, sigma, lengths=lengths)
    else:
        assert blob == blobp and h["format"] == (0 if sigma <= 6 else 1 if sigma <= 16 else 2)
    rc, blk, c, v = _read(ctx, d_buf, used, nruns)
    assert rc == 0, ctx.lib.tc_last_error(ctx.handle)
    _check_block_header(db, blk)
    assert np.array_equal(c, counts) and np.array_equal(v, vals)


def test_block_with_a_value_at_sigma_or_above_is_packed(ctx):
    counts, vals, sigma = S.mild(41, 20000, 7)
    db = _DevBlock(counts, vals, sigma)
    rc, _, good, _ = _write(ctx, db, HUFFMAN)
    assert rc == 0 and S.header(good)["format"] == 3
    for bad_value in (7, 9):
        v2 = vals.copy()
        v2[12345] = bad_value
        db = _DevBlock(counts, v2, sigma)
        rc, _, a, _ = _write(ctx, db, HUFFMAN)
        rcp, _, b, _ = _write(ctx, db, PACKED, fill=0x33)
        assert rc == 0 and rcp == 0 and a == b and S.header(a)["format"] == 1 and len(a) > len(good)


# ---- B: the reader on bodies this library did not write -------------------------------------------------------------------
def _carrier(ctx, counts, vals, sigma):
    """a device-written (packed) container of these runs: the header every foreign body is wrapped in"""
    db = _DevBlock(counts, vals, sigma)
    rc, _, blob, _ = _write(ctx, db, PACKED)
    assert rc == 0
    return db, blob


def _plus_one(lengths, lmax):
    """every length raised by one where that stays <= lmax: a valid code with a Kraft sum below 1"""
    ln = np.asarray(lengths, np.int64)
    return np.where((ln > 0) & (ln < lmax), ln + 1, ln)


def _gapped(hist):
    """lengths from {2, 7, 12} only, shorter for the frequent: gaps between the used lengths, Kraft sum below 1"""
    order = sorted((s for s in range(len(hist)) if hist[s] > 0), key=lambda s: (-int(hist[s]), s))
    ln = np.zeros(len(hist), np.int64)
    for rank, s in enumerate(order):
        ln[s] = 2 if rank < 2 else 7 if rank < 10 else 12
    return ln


def _foreign_bodies():
    out = {}
    c, v, s = S.mild(51, 10007, 9)
    for K in (1, 2, 64, 512, 4096, 16384):
        out["K%d" % K] = (c, v, s, dict(K=K))
    hist = H.histogram(c, v, s)
    cf, vf, sf = S.fib_values(20, 22, 55)                # 17 710 runs; the unlimited code is 19 deep, so every limit binds
    for lmax in (5, 9, 11, 12):
        out["lmax%d" % lmax] = (cf, vf, sf, dict(lmax=lmax, K=256))
    out["lmax9_every_length_plus_one"] = (c, v, s, dict(lmax=9, K=128, lengths=_plus_one(H.build_lengths(hist, 8), 9)))
    out["lmax12_lengths_2_7_12"] = (c, v, s, dict(lmax=12, K=1024, lengths=_gapped(hist)))
    c2, v2, s2 = S.two_tokens(52, 9001, 2)
    out["lmax1_two_tokens"] = (c2, v2, s2, dict(lmax=1, K=32))
    c1, v1, s1 = S.single_token(9001, 3)
    out["lmax1_one_token"] = (c1, v1, s1, dict(lmax=1, K=8))
    r = np.random.default_rng(53)
    c4, v4 = r.integers(1, 3, 7001).astype(np.int64), r.integers(0, 2, 7001).astype(np.int64)       # tokens 0, 1, RUNA
    out["lmax2_three_tokens"] = (c4, v4, 2, dict(lmax=2, K=2048))
    c5, v5, s5 = S.long_chunk(54, nruns=9000)
    c5[:4096] = r.integers(1 << 31, 1 << 32, 4096)
    out["K4096_huge_counts"] = (c5, v5, s5, dict(K=4096))
    return out


FOREIGN = _foreign_bodies()


@pytest.mark.parametrize("name", list(FOREIGN), ids=list(FOREIGN))
def test_reader_takes_bodies_this_library_did_not_write(ctx, name):
    counts, vals, sigma, kw = FOREIGN[name]
    nruns = len(counts)
    body = H.write_body(counts, vals, sigma, **kw)
    L = S.body_layout(body)
    lengths = np.frombuffer(body, np.uint8, L["nsyms"], 16).astype(np.int64)
    # the regime, on the CPU
    assert L["K"] == kw.get("K", 1024) and L["lmax"] == kw.get("lmax", 12) and lengths.max() <= L["lmax"]
    assert (nruns % L["K"] != 0 or L["K"] == 1) and L["nchunks"] == (nruns + L["K"] - 1) // L["K"]
    if name == "K1":
        assert L["nchunks"] == nruns > S.SCAN_TURN
    if name == "K16384":
        assert L["K"] > nruns and L["nchunks"] == 1
    if "plus_one" in name or "2_7_12" in name:
        assert H.kraft(lengths, L["lmax"]) < 1 << L["lmax"], "meant to be an incomplete code"
    if "2_7_12" in name:
        assert set(lengths[lengths > 0].tolist()) == {2, 7, 12}
    if name.startswith("lmax") and "_" not in name:
        assert lengths.max() == L["lmax"] < max(S.unlimited_lengths(H.histogram(counts, vals, sigma))), "the limit is meant to bind"
    if name == "K4096_huge_counts":
        dirb = np.frombuffer(body, "<u4", L["nchunks"], L["doff"])
        assert 4096 + int(S.ndigits(counts[:4096]).sum()) > 100000 and dirb[0] > 200000, "one lane is meant to walk > 100 000 tokens"
    rc_, rv_ = H.read_body(body, nruns, sigma)
    assert np.array_equal(rc_, counts) and np.array_equal(rv_, vals)
    db, carrier = _carrier(ctx, counts, vals, sigma)
    blob = S.as_format3(carrier, body)
    rc, blk, c, v = _read_bytes(ctx, blob, nruns)
    print("%s: nruns %d, sigma %d, K %d, L_max %d, chunks %d, body %d B, Kraft %d / %d"
          % (name, nruns, sigma, L["K"], L["lmax"], L["nchunks"], len(body), H.kraft(lengths, L["lmax"]), 1 << L["lmax"]))
    assert rc == 0, ctx.lib.tc_last_error(ctx.handle)
    _check_block_header(db, blk)
    assert np.array_equal(c, rc_) and np.array_equal(v, rv_)


def test_host_path_decodes_a_foreign_body_of_a_real_text(ctx):
    """decode_container (host buffers) on a real text's runs re-coded with K = 64, L_max = 9 and an incomplete code"""
    text = O.gen_acgtn(0x53, 40001)
    good = ctx.encode_container(text, coding="huffman")
    h = S.header(good)
    assert h["format"] == 3
    nruns, sigma = int(h["nruns"]), h["sigma"]
    counts, vals = H.read_body(good[HDR:], nruns, sigma)
    lengths = _plus_one(H.build_lengths(H.histogram(counts, vals, sigma), 8), 9)
    body = H.write_body(counts, vals, sigma, lengths=lengths, K=64, lmax=9)
    assert H.kraft(lengths, 9) < 1 << 9 and body != good[HDR:]
    blob = S.as_format3(good, body)
    assert ctx.decode_container(blob) == text.tobytes()
    rc, _, c, v = _read_bytes(ctx, blob, nruns)
    assert rc == 0 and np.array_equal(c, counts) and np.array_equal(v, vals)


# ---- C: the same verdict as the restatement on damaged bodies -----------------------------------------------------------
def _base_from_a():
    c, v, s = S.every_digit_count(4)
    return c, v, s, H.write_body(c, v, s)


def _base_from_b():
    c, v, s = S.mild(31, 3000, 7)
    ln = _plus_one(H.build_lengths(H.histogram(c, v, s), 8), 9)
    return c, v, s, H.write_body(c, v, s, lengths=ln, K=64, lmax=9)


def _base_from_text():
    text = O.gen_acgtn(0x51, 20000)
    idx, fl = O.mtf_encode_arr(O.bwt_encode_arr(text))
    c, v = O.rle_encode_u32_arr(idx)
    c, v = np.asarray(c, np.int64), np.asarray(v, np.int64)
    return c, v, len(fl), H.write_body(c, v, len(fl))


# base -> (maker, seed of the mutation list); the seeds were chosen on the CPU, against the restatement alone, so that
# both verdicts occur at least 20 times per base (asserted below)
DAMAGED = {"every_digit_count": (_base_from_a, 101), "K64_lmax9_incomplete": (_base_from_b, 223), "text_acgtn_20000": (_base_from_text, 103)}


@pytest.mark.parametrize("name", list(DAMAGED), ids=list(DAMAGED))
def test_same_verdict_as_the_restatement_on_damaged_bodies(ctx, name):
    make, seed = DAMAGED[name]
    counts, vals, sigma, body = make()
    nruns = len(counts)
    muts = S.mutants(body, seed)
    verdicts = [S.verdict(b, nruns, sigma) for _, b in muts]
    refused = sum(v is None for v in verdicts)
    assert 100 <= len(muts) <= 140 and refused >= 20 and len(muts) - refused >= 20, (len(muts), refused)
    db, carrier = _carrier(ctx, counts, vals, sigma)
    base = S.as_format3(carrier, body)
    rc, _, c, v = _read_bytes(ctx, base, nruns)
    assert rc == 0 and np.array_equal(c, counts) and np.array_equal(v, vals)
    wrong = []
    changed = 0
    for (what, b), want in zip(muts, verdicts):
        rc, _, c, v = _read_bytes(ctx, S.as_format3(carrier, b), nruns)
        if want is None:
            if rc != -3:
                wrong.append("%s: the restatement refuses, the device answers %d" % (what, rc))
            rc, _, c, v = _read_bytes(ctx, base, nruns)
            assert rc == 0 and np.array_equal(c, counts) and np.array_equal(v, vals), "the base body after the refusal of: " + what
        else:
            changed += not (np.array_equal(want[0], counts) and np.array_equal(want[1], vals))
            if rc != 0:
                wrong.append("%s: the restatement decodes, the device answers %d (%s)" % (what, rc, ctx.lib.tc_last_error(ctx.handle)))
            elif not (np.array_equal(c, want[0]) and np.array_equal(v, want[1])):
                wrong.append("%s: both decode, to different runs" % what)
    print("%s: %d mutants, %d refused by both, %d decoded by both (%d of them to other runs than the base's)"
          % (name, len(muts), refused, len(muts) - refused, changed))
    assert not wrong, "\n".join(wrong)
