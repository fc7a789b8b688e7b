"""The pass over the text that finds the tied suffixes of key-only MSD levels again (csrc/tc_sa.hpp), in its form for
alphabets with a register table of codes: tied_probe_w_kernel stages the text raw in LDS, 16 bytes per store, makes the
codes by v_perm_b32, and deals the positions that pass its filter out over the lanes of a wave (TC_TIED_PROBE, default 1;
0 = tied_probe_kernel and its byte image of codes, which also serves every other alphabet).  A workgroup's four waves share
16384 positions (TPK_TILE), a wave goes through 4096 of them per turn, a thread through 64: the seams the lengths and the
planted ties below sit on.  Every case takes the key-only MSD way at a small size (TC_SA_MSD_MIN_LOG2=10, as tests/test_gpu_msd.py),
asserts that it did (msd_path, msd_keyonly, ties behind round 0) and that tc_dbg_tied_probe (include/textcomp_debug.h)
names the expected kernel, and compares the block field for field with the oracle's, with the block of the same context
under TC_TIED_PROBE=0 and with the block under TC_SA_MSD_KEYONLY=0.

Planted ties.  A place a is planted by writing t[a : a + ln] (ln in 22 .. 60) to a stretch of the text that nothing else
touches, not the other way round: the suffix at a then starts a copied stretch whatever else is planted around it, so places
one symbol apart (the tile seam 16384 - j, the seam 64 k - 1 / 64 k of two threads' windows) do not wipe each other out.
Places whose 22 symbols do not fit in front of the text's last 40 symbols are left out of that text (n = 16383 .. 16385 end
at the first tile seam: there t[n - 40:] = t[1000 : 1040], the tie that reaches the end of the text, lies across or against
it).  Before a case is relied on, the oracle's suffix array says on the CPU that every planted place has a neighbour equal
on the 21 key symbols."""
import ctypes as C

import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu

TILE = 16384          # TPK_TILE
OLD, NEW = 1, 2       # tc_dbg_tied_probe's out[0]


@pytest.fixture(scope="module")
def ctx():
    import textcomp
    c = textcomp.Context(0)
    c.lib.tc_dbg_tied_probe.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    c.lib.tc_dbg_tied_probe.restype = C.c_int
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _msd_for_small_records(monkeypatch):
    monkeypatch.setenv("TC_SA_MSD_MIN_LOG2", "10")


def _probe(ctx):
    out = (C.c_uint32 * 2)(7, 7)
    assert ctx.lib.tc_dbg_tied_probe(ctx.handle, out) == 0
    return int(out[0]), int(out[1])


def _oracle_block(t):
    L = O.bwt_encode_arr(t)
    idx, fl = O.mtf_encode_arr(L)
    counts, vals = O.rle_encode_u32_arr(idx)
    return dict(primary=int(np.nonzero(L < 0)[0][0]), final_list=fl.tolist(), run_count=counts, run_value=vals)


def _assert_block(blk, want, what):
    assert blk["primary"] == want["primary"], what
    assert list(blk["final_list"]) == list(want["final_list"]), what
    assert np.array_equal(blk["run_count"], want["run_count"]), what
    assert np.array_equal(blk["run_value"], want["run_value"]), what


def _keyonly_encode(ctx, t, kernel, what):
    """one encode that must go the key-only MSD way with ties and run `kernel` for them"""
    blk = ctx.encode(t)
    st = ctx.stats()
    used, found = _probe(ctx)
    print("%s: msd_path %d keyonly %d m[1] %d probe kernel %d found %d" % (what, st.msd_path, st.msd_keyonly, st.m[1], used, found))
    assert st.msd_path == 1 and st.msd_keyonly == 1 and st.m[1] > 0, what
    assert used == kernel and found > 0, (what, used, found)
    return blk


def _check(ctx, t, monkeypatch, kernel):
    t = np.ascontiguousarray(t, dtype=np.uint8)
    want = _oracle_block(t)
    blk = _keyonly_encode(ctx, t, kernel, "n=%d default" % len(t))
    monkeypatch.setenv("TC_TIED_PROBE", "0")
    old = _keyonly_encode(ctx, t, OLD, "n=%d TC_TIED_PROBE=0" % len(t))
    monkeypatch.delenv("TC_TIED_PROBE")
    monkeypatch.setenv("TC_SA_MSD_KEYONLY", "0")
    starts = ctx.encode(t)
    st = ctx.stats()
    assert st.msd_path == 1 and st.msd_keyonly == 0 and _probe(ctx)[0] == 0
    monkeypatch.delenv("TC_SA_MSD_KEYONLY")
    _assert_block(blk, want, "against the oracle")
    _assert_block(blk, old, "against TC_TIED_PROBE=0")
    _assert_block(blk, starts, "against TC_SA_MSD_KEYONLY=0")
    _assert_block(old, want, "TC_TIED_PROBE=0 against the oracle")
    return blk


def _tied_on_key(t, places, h):
    """CPU: every place has a neighbour in the oracle's suffix array that is equal on h symbols inside the text"""
    n = len(t)
    sa = O.suffix_array(t).astype(np.int64)
    rank = np.empty(n + 1, np.int64)
    rank[sa] = np.arange(n + 1)
    for a in places:
        ok = False
        for r in (rank[a] - 1, rank[a] + 1):
            if 0 <= r <= n:
                b = int(sa[r])
                ok = ok or (a + h <= n and b + h <= n and np.array_equal(t[a:a + h], t[b:b + h]))
        assert ok, "place %d of n=%d is not tied on %d symbols" % (a, n, h)


def _planted_acgtn(n):
    rng = np.random.default_rng(n)
    t = O.gen_acgtn(0x7E + n, n).copy()
    t[n - 40:] = t[1000:1040]                       # a tie that reaches the end of the text (codes 0 behind it)
    places = [0] + [TILE - j for j in (22, 21, 20, 1, 0)] + [64 * 37 - 1, 64 * 37]
    src = 3000                                      # stretches nothing else touches: 3000, 3100, ..
    kept = []
    for a in places:
        ln = min(int(rng.integers(22, 61)), n - 40 - a)
        if ln < 22:
            continue
        t[src:src + ln] = t[a:a + ln]
        src += 100
        kept.append(a)
    t[64 * 20 + 30:64 * 20 + 54] = t[64 * 20 + 4:64 * 20 + 28]   # both members inside one thread's 64 positions
    kept += [64 * 20 + 4, n - 40]
    assert src < 5000 and 0 in kept and 64 * 37 in kept
    _tied_on_key(t, kept, 21)
    return t, kept


@pytest.mark.parametrize("n", [16383, 16384, 16385, 16384 + 63, 16384 + 64, 16384 + 85, 2 * 16384 + 21, 100003])
def test_tied_probe_lengths_and_planted_ties(ctx, n, monkeypatch):
    """one tile less a symbol, one tile, one symbol more, a last tile shorter than / equal to / longer than the 64-byte
    overhang (and than the overhang plus the key), a third tile of a key's length, seven tiles"""
    t, kept = _planted_acgtn(n)
    if n >= TILE + 63:
        assert all(TILE - j in kept for j in (22, 21, 20, 1, 0)), kept
    _check(ctx, t, monkeypatch, NEW)


def test_tied_probe_more_hits_in_a_wave_than_its_list_holds(ctx, monkeypatch):
    """one copy of 5000 symbols: every position of a wave's 4096 is tied, eight times the 512 entries of the list the
    wave deals its positions out from (about 10 000 tied members, a third of what the table is made for).  The
    collision sample would send such a text the LSD way, and the plan would move suffix starts: TC_SA_MSD=2 and
    TC_SA_MSD_KEYONLY=2 keep it on the key-only levels"""
    monkeypatch.setenv("TC_SA_MSD", "2")
    t = O.gen_acgtn(0x7D, 100003).copy()
    t[60000:65000] = t[20000:25000]
    t[100003 - 40:] = t[1000:1040]
    _tied_on_key(t, [60000, 64979, 100003 - 40], 21)
    monkeypatch.setenv("TC_SA_MSD_KEYONLY", "2")
    blk = _keyonly_encode(ctx, t, NEW, "copy of 5000")
    assert _probe(ctx)[1] > 9000
    monkeypatch.setenv("TC_TIED_PROBE", "0")
    old = _keyonly_encode(ctx, t, OLD, "copy of 5000, TC_TIED_PROBE=0")
    monkeypatch.delenv("TC_TIED_PROBE")
    monkeypatch.setenv("TC_SA_MSD_KEYONLY", "0")
    starts = ctx.encode(t)
    assert ctx.stats().msd_keyonly == 0
    want = _oracle_block(t)
    _assert_block(blk, want, "against the oracle")
    _assert_block(blk, old, "against TC_TIED_PROBE=0")
    _assert_block(blk, starts, "against TC_SA_MSD_KEYONLY=0")


def _hash_shift(alpha):
    """radix_keygen_hash (csrc/tc_radix.hpp): the first shift at which three adjacent bits tell the bytes apart"""
    if len(alpha) > 8:
        return None
    for sh in range(6):
        if len({(int(b) >> sh) & 7 for b in alpha}) == len(alpha):
            return sh
    return None


def _text_with_copies(alpha, n, seed, h):
    rng = np.random.default_rng(seed)
    alpha = np.array(alpha, dtype=np.uint8)
    t = alpha[rng.integers(0, len(alpha), n)]
    spots = []
    for i in range(30):                             # 30 copies in stretches of their own
        ln = int(rng.integers(h + 1, 300))
        a, b = 1000 + 2000 * i, 70000 + 2000 * i + int(rng.integers(0, 64))
        t[b:b + ln] = t[a:a + ln]
        spots.append(b)
    t[n - 40:] = t[100:140]
    _tied_on_key(t, spots, h)
    return t


@pytest.mark.parametrize("alpha,s,sh", [((0x41, 0x61), 5, 3), ((0x20, 0x40, 0x80), 4, 4), ((0xF8, 0xF9, 0xFA, 0xFB, 0xFC, 0xFD, 0xFE), 2, 0)],
                         ids=["2-bytes", "3-bytes", "7-bytes-0xF8-0xFE"])
def test_tied_probe_other_field_widths(ctx, alpha, s, sh, monkeypatch):
    """B = 3, 4, 8: fields of 5, 4 and 2 symbols, keys of 35, 28 and 14, windows of 3, 2 and 1 units of the next thread;
    shifts 3, 4 and 0 of the register table; the last alphabet at the end of the byte range"""
    assert _hash_shift(alpha) == sh
    _check(ctx, _text_with_copies(alpha, 150000, len(alpha), 7 * s), monkeypatch, NEW)


@pytest.mark.parametrize("alpha,s", [(tuple(range(0x30, 0x3F)), 2), ((0x00, 0x40, 0x01, 0x80), 3), (tuple(range(0xF0, 0xF8)), 2)],
                         ids=["15-bytes", "4-bytes-no-shift", "8-bytes-base-9"])
def test_tied_probe_old_kernel_alphabets(ctx, alpha, s, monkeypatch):
    """alphabets the register table does not serve: 15 bytes; 4 bytes of which some two agree in every window of three
    bits (0x00 / 0x40 / 0x80 in bits 0-2, 0x00 / 0x01 in every window above bit 0 -- two bytes alone always differ in
    some window); 8 bytes that have a table but base 9.  tied_probe_kernel runs whatever TC_TIED_PROBE says"""
    assert (_hash_shift(alpha) is None) == (len(alpha) != 8)
    _check(ctx, _text_with_copies(alpha, 150000, len(alpha), 7 * s), monkeypatch, OLD)


@pytest.mark.parametrize("off", [1, 15])
def test_tied_probe_unaligned_device_text(ctx, off, monkeypatch):
    """tc_encode_dev on buf[off:]: no 16-byte unit of the text is aligned in memory, every unit is put together from
    byte loads; the block is that of the aligned encode of the same bytes"""
    import torch
    from textcomp import Block
    t, _ = _planted_acgtn(2 * 16384 + 21)
    n = len(t)
    want = _check(ctx, t, monkeypatch, NEW)
    buf = torch.zeros(n + 32, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[off:off + n] = torch.from_numpy(t).cuda()
    cap = n + 2
    cnt = torch.empty(cap, dtype=torch.int32, device="cuda")
    val = torch.empty(cap, dtype=torch.int16, device="cuda")
    b = Block()
    b.nruns, b.run_count, b.run_value = cap, cnt.data_ptr(), val.data_ptr()
    torch.cuda.synchronize()
    ctx._check(ctx.lib.tc_encode_dev(ctx.handle, C.c_void_p(buf.data_ptr() + off), n, C.byref(b)))
    st = ctx.stats()
    used, found = _probe(ctx)
    assert st.msd_path == 1 and st.msd_keyonly == 1 and st.m[1] > 0 and used == NEW and found > 0, (st.msd_path, st.msd_keyonly, used, found)
    k = int(b.nruns)
    got = dict(primary=int(b.primary), final_list=list(b.final_list[:b.sigma]),
               run_count=cnt[:k].cpu().numpy().astype(np.int64), run_value=val[:k].cpu().numpy().astype(np.int64))
    _assert_block(got, dict(primary=want["primary"], final_list=list(want["final_list"]),
                            run_count=want["run_count"].astype(np.int64), run_value=want["run_value"].astype(np.int64)),
                  "unaligned by %d against the aligned encode" % off)
