"""lcp_long_kernel (csrc/tc_lcp.hpp, step 3) in the form that runs on the device: 256 lanes, the 64 / 128 / 256 ramp of
loading lanes, chunk c = u * act + lane, the workgroup minimum over four waves, items handed round robin to the grid --
none of which the one-lane host check (host/check/lcp_kernels.cpp) has.  Every comparison is exact, on the whole LCP
array, through both entry paths (test_gpu_lcp._check_both); the references are lcp_ref.esa_direct below about 4000 bytes
and the C oracle's suffix array + lcp_ref.kasai above.  What an input claims to exercise -- "one long item of value m",
"more items than three grids", "so many per turn regime" -- is asserted from the reference alone (lcp_ref.long_items)
before the library is asked, so that a text that stops reaching its path fails instead of passing for nothing."""
import ctypes as C
import functools

import numpy as np
import pytest

import lcp_ref
import oracle as O
from test_gpu_lcp import _check_both, _dev_forms

pytestmark = pytest.mark.gpu

# ---- the geometry of lcp_long_kernel, restated from csrc/tc_lcp.hpp (LCP_NT, and `act`, `step`, `o0`, `o1` of the kernel)
LCP_NT = 256                 # lanes of a workgroup
WAVE = 64                    # lanes of a wave: `act` starts there and doubles up to LCP_NT
CHUNK = 16                   # bytes a lane compares per load
ROWS = 2                     # chunk rows a turn: chunk c = u * act + lane, u < ROWS
CAP16 = 16                   # the smallest cap tc_dbg_lcp_set_short_cap takes


def _act(turn):
    return min(WAVE << turn, LCP_NT)


def _turn_start(turn):
    """bytes above the cap at which turn `turn` starts"""
    return sum(ROWS * _act(t) * CHUNK for t in range(turn))


def _boundary_offsets():
    """d = stop - cap at every edge of the turn geometry: the first chunk and its neighbour; the row split of turns 0, 1,
    2 (lane 0 of row u = 1); the start of turns 1, 2, 3 (stop == step: the next turn answers 0); the first wave boundary
    inside a row of turn 1 (two waves); and a few bytes into turn 4.  Each edge with the byte before and after."""
    edges = {_turn_start(t) for t in (1, 2, 3)}
    edges |= {_turn_start(t) + _act(t) * CHUNK for t in (0, 1, 2)}
    edges.add(_turn_start(1) + WAVE * CHUNK)
    d = {0, 1, CHUNK - 1, CHUNK, CHUNK + 1, _turn_start(4) + 5}
    for e in edges:
        d |= {e - 1, e, e + 1}
    return sorted(d)


BOUNDARY_D = _boundary_offsets()
# the turn each offset stops in: one test case per turn
TURN_GROUPS = [[d for d in BOUNDARY_D if _turn_start(t) <= d < (_turn_start(t + 1) if t < 3 else 1 << 30)] for t in range(4)]


def test_the_boundary_list_is_the_one_the_geometry_gives():
    """with LCP_NT = 256 the derived offsets are these 27; a change of the ramp in tc_lcp.hpp has to be restated above"""
    assert BOUNDARY_D == [0, 1, 15, 16, 17, 1023, 1024, 1025, 2047, 2048, 2049, 3071, 3072, 3073, 4095, 4096, 4097, 6143,
                          6144, 6145, 10239, 10240, 10241, 14335, 14336, 14337, 22533]
    assert sum(len(g) for g in TURN_GROUPS) == len(BOUNDARY_D)


@pytest.fixture(scope="module")
def ctx():
    import textcomp
    with textcomp.Context(0) as c:
        yield c


@pytest.fixture
def set_cap(ctx):
    """tc_dbg_lcp_set_short_cap of include/textcomp_debug.h; the module's context leaves every test at the default"""
    fn = ctx.lib.tc_dbg_lcp_set_short_cap
    fn.argtypes = [C.c_void_p, C.c_uint32]
    fn.restype = C.c_int

    def set_(cap):
        assert fn(ctx.handle, cap) == 0
    yield set_
    assert fn(ctx.handle, 0) == 0


def _default_cap():
    from textcomp import _lib
    return _lib.TC_LCP_SHORT_CAP


_REFS = {}


def _reference(key, make_text):
    """(text, sa, lcp) of a named input, computed once and left unchanged"""
    if key not in _REFS:
        text = bytes(make_text())
        if len(text) < 4000:
            sa, lcp = lcp_ref.esa_direct(text)
        else:
            sa = O.suffix_array(text).astype(np.uint32)
            lcp = lcp_ref.kasai(text, sa)
        lcp.setflags(write=False)
        sa.setflags(write=False)
        _REFS[key] = (text, sa, lcp)
    return _REFS[key]


def _summary_of(lcp):
    return int(lcp.max()), int(np.argmax(lcp)), int(lcp.astype(np.uint64).sum())


# ---- a. a stop at every boundary of the turn geometry --------------------------------------------------------------
def _both_endings_text(c, d):
    """a pair that stops at a differing byte, then a pair that stops at the end of the text, both of c + d bytes (16
    letters: with 4, a text of 40 KB has a chance repeat of 16 bytes, a second long item at cap 16)"""
    rng = np.random.default_rng(0x10A0000 + 4096 * c + d)
    return (lcp_ref.planted_pair(rng, c + d, "mismatch", sigma=16, seps=b"#$")
            + lcp_ref.planted_pair(rng, c + d, "end", sigma=16, seps=b"%&"))


@functools.lru_cache(maxsize=None)
def _packed_mismatch_texts(c):
    """the "mismatch" pairs of every offset in a few texts of at most 256 KiB, every separator byte used once: a list
    of (text, the planted values), built once per cap"""
    rng = np.random.default_rng(0x10B0000 + c)
    texts, cur, ms, sep = [], b"", [], 128
    for d in BOUNDARY_D:
        pair = lcp_ref.planted_pair(rng, c + d, "mismatch", sigma=16, seps=bytes([sep, sep + 1]))
        sep += 2
        if len(cur) + len(pair) > (256 << 10):
            texts.append((cur, ms))
            cur, ms = b"", []
        cur += pair
        ms.append(c + d)
    texts.append((cur, ms))
    assert sep <= 256
    return texts


@pytest.mark.parametrize("turn", range(4))
@pytest.mark.parametrize("cap", [0, CAP16])
def test_a_stop_at_every_boundary_of_the_turn_geometry(ctx, set_cap, cap, turn):
    c = cap or _default_cap()
    set_cap(cap)
    for d in TURN_GROUPS[turn]:
        m = c + d
        text, sa, lcp = _reference(("a", c, d), lambda: _both_endings_text(c, d))
        by_byte, by_end = lcp_ref.long_items(text, sa, c, lcp)
        # the claim: one long item of m bytes that stops at a differing byte (d = 0: its first chunk stops at 0), and one
        # that stops at the end of the text -- but for d = 0, where the text ends on the cap and nothing is left to compare
        assert by_byte.tolist() == [m], (c, d, by_byte)
        assert by_end.tolist() == ([m] if d else []), (c, d, by_end)
        assert int(lcp.max()) == m
        print("cap %d d %d: %d bytes, long items %s + %s" % (c, d, len(text), by_byte.tolist(), by_end.tolist()))
        d_lcp = _check_both(ctx, text, sa, lcp)
        assert ctx.lcp_summary_dev(d_lcp) == _summary_of(lcp), (c, d)


@pytest.mark.parametrize("offset", [1, 3])
@pytest.mark.parametrize("cap", [0, CAP16])
def test_a_the_stops_by_a_differing_byte_on_a_misaligned_text(ctx, set_cap, cap, offset):
    c = cap or _default_cap()
    set_cap(cap)
    for k, (packed, ms) in enumerate(_packed_mismatch_texts(c)):
        text, sa, lcp = _reference(("a-packed", c, k), lambda: packed)
        assert len(text) <= (256 << 10)
        by_byte, by_end = lcp_ref.long_items(text, sa, c, lcp)
        for m in ms:
            assert int((by_byte == m).sum()) == 1 and m not in by_end, (c, m)
        print("cap %d text %d: %d bytes, planted %s, long items %d + %d" % (c, k, len(text), ms, len(by_byte), len(by_end)))
        sa_d, lcp_d, _ = _dev_forms(ctx, text, offset)
        assert np.array_equal(sa_d, sa)
        assert np.array_equal(lcp_d, lcp), "first difference at row %d" % int(np.flatnonzero(lcp_d != lcp)[:1].sum())


# ---- b. more long items than workgroups, in every turn regime ------------------------------------------------------
def _binary_text():
    # seed 1: 12 154 long items at cap 16, values 16 .. 29, none stopping at the end of the text
    rng = np.random.default_rng(1)
    return (rng.integers(0, 2, 1 << 16, dtype=np.uint8) + ord("A")).astype(np.uint8).tobytes()


MIXED_N = 1 << 19
MIXED_SEED = 3


def _mixed_text():
    """Four letters, and copies of 20 .. 9000 bytes pasted in, each from text that is already final into a stretch that
    no later copy touches (the way an LZ77 decoder writes), one random letter between two copies.  A long item of L
    bytes needs L bytes of its own that nothing overwrites, so 50 items above cap + 6144 together with 50 above
    cap + 2048 need more than 400 000 bytes: the text has 2^19, and the copy lengths come in three bands, one per turn
    regime, in turn."""
    rng = np.random.default_rng(MIXED_SEED)
    n = MIXED_N
    letters = np.frombuffer(b"ACGT", np.uint8)
    t = letters[rng.integers(0, 4, n)].copy()
    bands = ((20, 600), (CAP16 + _turn_start(1) + 40, 2600), (CAP16 + _turn_start(2) + 40, 6700))
    at, k = 12000, 0                          # the first 12000 bytes stay random
    while True:
        lo, hi = bands[k % 3]
        ln = int(rng.integers(lo, 9001 if k % 9 == 8 else hi))      # (every third of the long band: up to 9000)
        if at + ln + 1 > n:
            break
        a = int(rng.integers(0, at - ln))
        t[at:at + ln] = t[a:a + ln].copy()
        at += ln + 1
        k += 1
    return t.tobytes()


def test_b_more_long_items_than_three_grids(ctx, set_cap):
    import torch
    text, sa, lcp = _reference("b-binary", _binary_text)
    by_byte, by_end = lcp_ref.long_items(text, sa, CAP16, lcp)
    grid = 8 * torch.cuda.get_device_properties(0).multi_processor_count     # tc_persistent_grid(ctx, 8) of lcp_device
    print("binary text: %d + %d long items at cap 16, grid %d" % (len(by_byte), len(by_end), grid))
    assert len(by_byte) + len(by_end) >= 3 * grid
    set_cap(CAP16)
    _check_both(ctx, text, sa, lcp)


def test_b_items_of_every_turn_regime_in_one_list(ctx, set_cap):
    # seed 3 (chosen on the CPU): 511 long items at cap 16 -- 327 stop in turn 0, 126 in turn 1, 58 in turn 2 or later
    text, sa, lcp = _reference("b-mixed", _mixed_text)
    v = np.concatenate(lcp_ref.long_items(text, sa, CAP16, lcp)).astype(np.int64) - CAP16
    counts = [int(((v >= 0) & (v < _turn_start(1))).sum()), int(((v >= _turn_start(1)) & (v < _turn_start(2))).sum()),
              int((v >= _turn_start(2)).sum())]
    print("mixed text: long items per regime", counts)
    assert min(counts) >= 50, counts
    set_cap(CAP16)
    _check_both(ctx, text, sa, lcp)


# ---- c. the cap does not change the result -----------------------------------------------------------------------------
def _fibonacci():
    a, b = b"a", b"ab"
    while len(b) < (1 << 15) + 1:
        a, b = b, b + a
    return b[:(1 << 15) + 1]


@pytest.fixture(scope="module")
def genome_like(ctx):
    """tc_generate_dev kind 2 (genome-like: repeats of a few hundred bytes), 2^16 bytes"""
    import torch
    n = 1 << 16
    d = torch.empty(n, dtype=torch.uint8, device="cuda")
    assert ctx.lib.tc_generate_dev(ctx.handle, 2, 0x10C2, n, C.c_void_p(d.data_ptr())) == 0
    torch.cuda.synchronize()
    text = d.cpu().numpy().tobytes()
    return _reference("c-genome", lambda: text)


@pytest.mark.parametrize("cap", [16, 32, 48, 256, 1024, 65536])
def test_c_the_cap_does_not_change_the_result(ctx, set_cap, genome_like, cap):
    """the same four texts at every cap against the one reference each (so equal to one another), and pairs one below,
    on and above the cap: cap 32 takes the single 16-byte step after the first load of lcp_irreducible_kernel, cap 48
    its 32-byte loop once, cap 65536 keeps every comparison in that kernel"""
    set_cap(cap)
    cases = [_reference("c-mismatch", lambda: lcp_ref.planted_pair(np.random.default_rng(0x10C0), 3001, "mismatch")),
             _reference("c-end", lambda: lcp_ref.planted_pair(np.random.default_rng(0x10C1), 2999, "end")),
             genome_like,
             _reference("c-fibonacci", _fibonacci)]
    assert int(cases[0][2].max()) == 3001 and int(cases[1][2].max()) == 2999
    for text, sa, lcp in cases:
        _check_both(ctx, text, sa, lcp)
    for m in (cap - 1, cap, cap + 1):
        if m > 4096:
            continue
        for ending in ("mismatch", "end"):
            prng = np.random.default_rng(0x10C1000 + 2 * m + (ending == "end"))
            text, sa, lcp = _reference(("c-pair", m, ending), lambda: lcp_ref.planted_pair(prng, m, ending))
            by_byte, by_end = lcp_ref.long_items(text, sa, cap, lcp)
            # below the cap nothing is long; on it only a stop at a differing byte is; above it both are
            want = ([m] if m >= cap else [], []) if ending == "mismatch" else ([], [m] if m > cap else [])
            assert (by_byte.tolist(), by_end.tolist()) == want, (cap, m, ending)
            assert int(lcp.max()) == m
            d_lcp = _check_both(ctx, text, sa, lcp)
            assert ctx.lcp_summary_dev(d_lcp) == _summary_of(lcp)


# ---- d. the arguments of tc_dbg_lcp_set_short_cap --------------------------------------------------------------------
def test_d_set_short_cap_arguments(ctx, set_cap):
    from textcomp import _lib
    fn = ctx.lib.tc_dbg_lcp_set_short_cap         # (set_cap declared its argument types)
    for bad in (8, 15, 24, 65552):
        assert fn(ctx.handle, bad) == _lib.TC_ERR_ARG
    assert fn(None, 16) == _lib.TC_ERR_ARG
    # a refused value must not leave the context with a cap it cannot run on: the call after it is exact.  (The result
    # does not tell cap 16 from the default -- test c shows that no cap changes it -- so this does not prove that 16
    # stayed in force, only that the refusal left a working cap behind; the library has no call that reads the cap.)
    text, sa, lcp = _reference("b-binary", _binary_text)
    set_cap(CAP16)
    assert fn(ctx.handle, 24) == _lib.TC_ERR_ARG
    _check_both(ctx, text, sa, lcp)
    assert fn(ctx.handle, 0) == 0                 # the default again
    _check_both(ctx, text, sa, lcp)


# ---- e. a suffix array that is none, through the library ---------------------------------------------------------------
class Lcg:
    """the generator host/check/lcp_kernels.cpp uses for the same texts and arrays"""

    def __init__(self, seed):
        self.x = seed

    def next(self):
        self.x = (self.x * 1103515245 + 12345) & 0x7fffffff
        return self.x >> 16


def _malformed_text(n):
    """two letters, so that at cap 16 many comparisons are long, and the first 300 bytes once more in the middle: a
    long item at the default cap"""
    g = Lcg(n)
    t = bytearray(65 + (g.next() & 1) for _ in range(n))
    t[n // 2:n // 2 + 300] = t[0:300]
    return bytes(t)


def _malformed_arrays(sa, n):
    out = []
    for where in (0, n // 2, n):
        for value in (n + 1, 0xffffffff):
            bad = sa.copy()
            bad[where] = value
            out.append(("row %d = %#x" % (where, value), bad))
    bad = sa.copy()
    bad[n // 3] = sa[2 * n // 3]
    out.append(("one value twice", bad))
    bad = sa.copy()
    bad[n // 2 + 1] = sa[0]
    out.append(("row 0's value repeated", bad))
    return out


def _wrong_permutations(sa, n):
    shuffled = sa.copy()
    g = Lcg(n + 1)
    for i in range(n, 0, -1):
        j = g.next() % (i + 1)
        shuffled[i], shuffled[j] = shuffled[j], shuffled[i]
    return [("reversed", sa[::-1].copy()), ("shuffled", shuffled)]


@pytest.mark.parametrize("n", [1000, 4097])
@pytest.mark.parametrize("cap", [0, CAP16])
def test_e_a_malformed_suffix_array_is_refused_and_the_context_goes_on(ctx, set_cap, cap, n):
    """the documented answer TC_ERR_MALFORMED (LCP_ERR_SA through tc_sync_check) from the library itself, the device
    error word cleared, the context usable: the very next call is exact.  host/check/lcp_kernels.cpp walks the same
    arrays under host sanitizers: every one of these stays in bounds."""
    import textcomp
    import torch
    set_cap(cap)
    text, sa, lcp = _reference(("e", n), lambda: _malformed_text(n))
    by_byte, by_end = lcp_ref.long_items(text, sa, cap or _default_cap(), lcp)
    assert len(by_byte) + len(by_end) >= 1           # the long kernel has work in the valid calls
    d_text = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).cuda()
    d_good = torch.from_numpy(sa.view(np.int32).copy()).cuda()
    for k, (what, bad) in enumerate(_malformed_arrays(sa, n)):
        d_bad = torch.from_numpy(bad.view(np.int32).copy()).cuda()
        with pytest.raises(textcomp.TcMalformed):
            ctx.lcp_array_dev(d_text, d_bad)
        if k % 2:      # the next call: an encode and its decode ...
            assert ctx.decode(ctx.encode(text)) == text, what
        # ... or the LCP array of the suffix array itself
        got = ctx.lcp_array_dev(d_text, d_good).cpu().numpy().view(np.uint32)
        assert np.array_equal(got, lcp), what
    for what, perm in _wrong_permutations(sa, n):
        assert sorted(perm.tolist()) == list(range(n + 1))
        got = ctx.lcp_array_dev(d_text, torch.from_numpy(perm.view(np.int32).copy()).cuda()).cpu().numpy().view(np.uint32)
        p = perm.astype(np.int64)
        assert got[0] == 0 and np.all(got[1:] <= n - np.maximum(p[:-1], p[1:])), what
    got = ctx.lcp_array_dev(d_text, d_good).cpu().numpy().view(np.uint32)
    assert np.array_equal(got, lcp)
