"""Reference decode of a tc_block (the dict shape of Context.encode) and the foreign blocks built from it.

TEST INFRASTRUCTURE, CPU only: nothing here imports the product or a GPU library.  `decode_block_ref` composes
the oracle's own stages -- np.repeat, seqFromMTF, magicInverseBWT -- and never reads `primary`: the reference's
decode takes no primary, the Nothing in the stream decides.  Everything below it builds blocks that no encoder
writes.  A transformation ("T", still valid for the reference) asserts decode_block_ref(out) == text before it
returns; a damage ("M") asserts what the reference says about it.  tests/test_block_ref.py runs all of them
without a GPU, tests/test_gpu_decode_foreign.py hands them to the library.
"""
import functools
import random

import numpy as np

import oracle as O

MALFORMED = "malformed"
RLE_HUGE = 16384          # csrc/tc_rle.hpp: runs this long are queued for the whole grid
TILE = 32768              # MTF_TILE = GM_TILE = LF_BLOCK (symbols)
RLD_TILE = 4096           # runs per tile of the run-length decoder


# ------------------------------------------------------------------ reference
def ref_outcome(blk):
    """-> ("text", bytes) | ("short", bytes) | ("throw", stage): what the reference's stages make of the block"""
    n = int(blk["n"])
    cnt = np.asarray(blk["run_count"], dtype=np.int64)
    val = np.asarray(blk["run_value"], dtype=np.int64)
    if int(cnt.sum()) != n + 1:
        return ("throw", "length")
    idx = np.repeat(val, cnt)
    try:
        sym = O.mtf_decode_arr(idx, np.asarray(blk["final_list"], dtype=np.int16)[:int(blk["sigma"])])
    except O.OracleMalformed:
        return ("throw", "mtf")
    if len(sym) != len(idx):       # an empty list decodes to an empty sequence (MTF/Internal.hs:202-209)
        return ("short", b"")
    try:
        text = O.bwt_decode_arr(sym)
    except O.OracleMalformed:
        return ("throw", "bwt")
    return ("text" if len(text) == n else "short", text)


def decode_block_ref(blk):
    """the text as bytes, or MALFORMED"""
    kind, val = ref_outcome(blk)
    return val if kind == "text" else MALFORMED


def mtf_encode_over(sym, lst):
    """plain MTF encode of `sym` over the explicit initial list sorted(set(lst)) -> (idx int32[], final list int16[]).
    (The oracle's encoder only knows the alphabet of the symbols present.)"""
    l = sorted(set(int(v) for v in lst))
    idx = np.empty(len(sym), dtype=np.int32)
    for j, s in enumerate(np.asarray(sym).tolist()):
        i = l.index(s)
        idx[j] = i
        if i:
            l.insert(0, l.pop(i))
    return idx, np.array(l, dtype=np.int16)


def _mtf_encode(sym, lst):
    """mtf_encode_over; by the oracle's encoder where the list is exactly the symbols present (the same function
    there -- test_block_ref checks that -- and 50 times faster)"""
    sym = np.asarray(sym, dtype=np.int16)
    want = sorted(set(int(v) for v in lst))
    if want == np.unique(sym).tolist():
        return O.mtf_encode_arr(sym)
    return mtf_encode_over(sym, want)


def block_of(sym, lst):
    """the block of a symbol stream (int16, -1 = Nothing) encoded over `lst`; primary = the row of the first Nothing"""
    sym = np.asarray(sym, dtype=np.int16)
    idx, fl = _mtf_encode(sym, lst)
    cnt, val = O.rle_encode_u32_arr(idx)
    nothing = np.nonzero(sym < 0)[0]
    return dict(n=len(sym) - 1, primary=int(nothing[0]) if len(nothing) else 0, sigma=len(fl),
                final_list=fl.astype(np.int16), run_count=cnt.astype(np.uint32), run_value=val.astype(np.uint16))


def _copy(blk, **kw):
    out = dict(blk)
    for k in ("final_list", "run_count", "run_value"):
        out[k] = np.array(blk[k], copy=True)
    out.update(kw)
    return out


# ------------------------------------------------------------------ base texts
ACGTN_LENGTHS = (1, 2, 255, 256, 4095, 4096, 32767, 32768, 70001)
# name -> lengths.  sNN: NN byte values (sigma NN + 1); b256 / late: every byte value (sigma 257)
BASES = dict(acgtn=ACGTN_LENGTHS, s12=(4097, 70001), s40=(70001,), s100=(70001,), s150=(70001,), s200=(70001,),
             s255=(70001,), b256=(4097, 70001), late=(70001,))
SELECTOR_LENGTHS = (4096, 4097, 70001)


@functools.lru_cache(maxsize=None)
def base_text(name, n):
    if name == "acgtn":
        return O.gen_acgtn(0xF0 + n % 251, n).tobytes()
    rng = np.random.default_rng([n, sum(name.encode())])
    if name == "late":     # 16 values for 60 000 bytes, the other 240 first occur after that
        head = rng.integers(0, 16, 60000, dtype=np.uint8)
        tail = np.concatenate([np.arange(16, 256, dtype=np.uint8), rng.integers(0, 256, n - 60000 - 240, dtype=np.uint8)])
        return head.tobytes() + rng.permutation(tail).astype(np.uint8).tobytes()
    k = 256 if name == "b256" else int(name[1:])
    vals = (np.arange(k) * 256 // k + (0 if k == 256 else 1)).astype(np.uint8)   # spread over the byte range, never 0 unless all
    body = np.concatenate([vals, vals[rng.integers(0, k, n - k)]])
    return rng.permutation(body).astype(np.uint8).tobytes()


@functools.lru_cache(maxsize=None)
def base_sym(name, n):
    s = O.bwt_encode_arr(base_text(name, n))
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def base_block(name, n):
    """what the encoder writes for the text (test_gpu_decode_foreign checks that it is)"""
    sym = base_sym(name, n)
    blk = block_of(sym, np.unique(sym))
    assert decode_block_ref(blk) == base_text(name, n)
    return blk


def all_bases():
    return [(name, n) for name, ns in BASES.items() for n in ns]


# ------------------------------------------------------------------ T: still valid for the reference
def _valid(blk, text):
    assert decode_block_ref(blk) == text, "a transformation that should keep the block valid did not"
    return blk


def _cut_runs(blk, rnd, zero_value):
    """runs of count >= 2 split at random points; zero_value(k, v): the value of a zero-count run put in front of run k
    (value v), or None for no such run"""
    cnt, val = [], []
    for k, (c, v) in enumerate(zip(blk["run_count"].tolist(), blk["run_value"].tolist())):
        z = zero_value(k, v)
        if z is not None:
            cnt.append(0)
            val.append(z)
        while c >= 2 and rnd.random() < 0.67:
            a = rnd.randrange(1, c)
            cnt.append(a)
            val.append(v)
            c -= a
        cnt.append(c)
        val.append(v)
    return cnt, val


def t1_cut(blk, text, seed, zero_values=None):
    """every run of count >= 2 split at random points; zero-count runs inserted (in front of the first run, of one run in
    four, and behind the last) -- with an in-range value, or (zero_values) with values no list has.  The reference never
    indexes with a value it repeats zero times."""
    rnd = random.Random(seed)
    sigma = int(blk["sigma"])

    def zero_value(k, v):
        if k and rnd.random() >= 0.25:
            return None
        if zero_values is not None:
            return zero_values[k % len(zero_values)]
        return rnd.randrange(sigma) if rnd.random() < 0.5 else v

    cnt, val = _cut_runs(blk, rnd, zero_value)
    cnt.append(0)
    val.append(zero_values[-1] if zero_values is not None else 0)
    return _valid(_copy(blk, run_count=np.array(cnt, np.uint32), run_value=np.array(val, np.uint16)), text)


def t1_split_only(blk, text, seed):
    """runs cut up, no zero counts: the form every container format can carry"""
    cnt, val = _cut_runs(blk, random.Random(seed), lambda k, v: None)
    return _valid(_copy(blk, run_count=np.array(cnt, np.uint32), run_value=np.array(val, np.uint16)), text)


def t2_list(blk, text, mode, seed=0):
    fl = blk["final_list"]
    fl = fl[::-1].copy() if mode == "rev" else np.random.default_rng(seed).permutation(fl).astype(np.int16)
    return _valid(_copy(blk, final_list=fl), text)


def t3_dups(blk, text, total, seed=0):
    """duplicates appended until the list has `total` entries (sigma = total); the reference takes sort(unique(list))"""
    fl = blk["final_list"]
    extra = np.random.default_rng(seed).choice(fl, total - len(fl))
    return _valid(_copy(blk, final_list=np.concatenate([fl, extra]).astype(np.int16), sigma=total), text)


def t4_over(name, n, lst):
    """the text's symbols re-encoded over a list that holds symbols the stream does not"""
    return _valid(block_of(base_sym(name, n), lst), base_text(name, n))


def t4_lists():
    """name -> list for the ACGTN texts (A = 65: the unused bytes lie below it, so every index moves up)"""
    acgtn = [-1, 65, 67, 71, 78, 84]
    return {"6": acgtn, "7": acgtn + [33], "12": acgtn + list(range(33, 39)), "17": acgtn + list(range(33, 44)),
            "46": acgtn + list(range(20, 60)), "257": list(range(-1, 256))}


def t5_primary(blk, text, p):
    return _valid(_copy(blk, primary=int(p)), text)


def t5_values(blk, wide):
    true, N = int(blk["primary"]), int(blk["n"]) + 1
    vals = [0, true - 1, true + 1, N - 1, N, 1 << 40] if wide else [0, true + 1]
    return [v for v in dict.fromkeys(vals) if v >= 0 and v != true]


# ------------------------------------------------------------------ M: damaged; the reference decides
def m1_positions(blk):
    """run indices: the first, the last, one in each interior tile of symbols, and the first of the second and of the last
    tile of runs"""
    cnt = blk["run_count"].astype(np.int64)
    ends = np.cumsum(cnt)
    k = len(cnt)
    pos = {0, k - 1}
    tile = 4096 if int(blk["sigma"]) == 257 else TILE      # M257_TILE: the tiles of the sigma = 257 kernels
    for t in range(1, (int(ends[-1]) - 1) // tile):
        pos.add(int(np.searchsorted(ends, t * tile + 17, side="right")))
    if k > RLD_TILE:
        pos.update({RLD_TILE, (k - 1) // RLD_TILE * RLD_TILE})
    return sorted(pos)


def m1_bad_index(blk, run, value):
    """an index >= sigma in a run of count >= 1: DS.index out of range"""
    assert blk["run_count"][run] >= 1 and value >= blk["sigma"]
    out = _copy(blk)
    out["run_value"][run] = value
    assert ref_outcome(out) == ("throw", "mtf")
    return out


def m2_no_nothing(name, n):
    """the Nothing replaced by a byte of the alphabet, `primary` left as it was: the reference answers the empty text"""
    sym = base_sym(name, n).copy()
    p = int(np.nonzero(sym < 0)[0][0])
    sym[p] = sym[p - 1] if p else sym[1]
    out = block_of(sym, np.unique(base_sym(name, n)))
    out["primary"] = p      # the header still names the row: on sigma = 257 the split's check has to refuse the stream
    assert ref_outcome(out) == ("short", b"")
    return out


def m2_second_nothing(name, n, row):
    """a second Nothing on `row`; the reference throws only where the row is on the walk"""
    sym = base_sym(name, n).copy()
    assert sym[row] >= 0
    sym[row] = -1
    out = block_of(sym, np.unique(base_sym(name, n)))
    assert ref_outcome(out)[0] != "text"      # on the walk: fromJust throws; off it: the cycle misses a row, the text is short
    return out


def m2_rows(name, n, k=20):
    sym = base_sym(name, n)
    rows = np.nonzero(sym >= 0)[0]
    return np.random.default_rng([n, 2]).permutation(rows)[:k].tolist()


M3_SWAPS = 40
# Seeds whose swap still decodes to a full-length (different) text, found by scanning seeds on the CPU: one swap in ten to
# a hundred does, so forty consecutive seeds would not hold the five per alphabet the tests ask for.
M3_FULL = {("acgtn", 4096): [13, 15, 35, 39, 41, 49], ("acgtn", 70001): [15, 25, 33, 65, 81, 87],
           ("s12", 4097): [11, 14, 21, 33, 49, 59], ("s12", 70001): [11, 27, 33, 35, 65, 87],
           ("s40", 70001): [15, 30, 55, 93, 135, 195], ("s100", 70001): [45, 83, 85, 145, 147, 163],
           ("s150", 70001): [101, 145, 229, 239, 361, 456], ("s200", 70001): [30, 209, 285, 295, 368, 483],
           ("s255", 70001): [43, 61, 94, 95, 128, 163], ("b256", 4097): [0, 18, 26, 30, 32, 43],
           ("b256", 70001): [137, 188, 215, 244, 302, 444], ("late", 70001): [11, 15, 29, 61, 76, 79]}


def m3_seeds(name, n):
    full = M3_FULL.get((name, n), [])
    return full + [s for s in range(M3_SWAPS) if s not in full][:M3_SWAPS - len(full)]


def m3_swap(name, n, seed):
    """two rows of the last column that hold different symbols, swapped: any two rows (even seeds), or two rows at most
    eight apart (odd seeds)"""
    sym = base_sym(name, n).copy()
    rng = np.random.default_rng([seed, n, 3])
    while True:
        i = int(rng.integers(0, len(sym)))
        j = int(rng.integers(0, len(sym))) if seed % 2 == 0 else min(i + int(rng.integers(1, 9)), len(sym) - 1)
        if sym[i] != sym[j]:
            break
    sym[i], sym[j] = sym[j], sym[i]
    out = block_of(sym, np.unique(sym))
    kind, text = ref_outcome(out)
    assert kind in ("text", "short") or (kind, text) == ("throw", "bwt")
    assert kind != "text" or text != base_text(name, n)
    return out


def m3_bases():
    """per alphabet: the n = 4096 / 4097 text where there is one, and the n = 70001 text"""
    out = []
    for name, ns in BASES.items():
        out.append((name, [n for n in ns if n in SELECTOR_LENGTHS]))
    return out


def m4_lengths(blk):
    """[(id, block)]: every one of them malformed for the reference (the lengths do not add up)"""
    out = []
    n = int(blk["n"])
    k = len(blk["run_count"])
    for name, d in (("sum_n", -1), ("sum_n_plus_2", 1)):
        b = _copy(blk)
        r = int(np.argmax(b["run_count"])) if d < 0 else k // 2
        b["run_count"][r] = int(b["run_count"][r]) + d
        out.append((name, b))
    b = _copy(blk)
    b["run_count"][k // 2] = 0xffffffff
    out.append(("count_ffffffff", b))
    out.append(("huge_runs", _copy(blk, run_count=np.full(70000, RLE_HUGE, np.uint32),
                                   run_value=(np.arange(70000) % max(int(blk["sigma"]), 1)).astype(np.uint16))))
    out.append(("n_too_small", _copy(blk, n=n - 1)))
    out.append(("n_too_large", _copy(blk, n=n + 1)))
    for _, b in out:
        assert ref_outcome(b) == ("throw", "length")
    return out


def m5_lists(blk):
    """[(id, block, "arg" | MALFORMED)].  Entries outside -1..255 are no Maybe Word8: an argument error, the reference has
    no such value.  sigma = 0 with n > 0: seqFromMTF of an empty list is the empty sequence, so the text is empty."""
    out = []
    for name, v in (("entry_minus_2", -2), ("entry_256", 256)):
        b = _copy(blk)
        b["final_list"][len(b["final_list"]) // 2] = v
        out.append((name, b, "arg"))
    b = _copy(blk, sigma=0, final_list=np.zeros(0, np.int16))
    assert ref_outcome(b) == ("short", b"")
    out.append(("sigma_0", b, MALFORMED))
    fl = np.resize(blk["final_list"], 257).astype(np.int16)
    out.append(("sigma_258", _copy(blk, sigma=258, final_list=fl), "arg"))
    return out


# ------------------------------------------------------------------ the cases, by family
def _bad_values(sigma):
    return [257, 65535] if sigma == 257 else [v for v in dict.fromkeys([sigma, 255, 256, 65535]) if v >= sigma]


@functools.lru_cache(maxsize=None)
def cases(family, name, n):
    """[(id, block, expectation)] of one family on one base text; expectation = decode_block_ref (bytes or MALFORMED)"""
    blk, text = base_block(name, n), base_text(name, n)
    sigma = int(blk["sigma"])
    out = []
    if family == "T1":
        out.append(("cut", t1_cut(blk, text, 11)))
        out.append(("zero_foreign", t1_cut(blk, text, 12, zero_values=[sigma, 255, 256, 65535])))
        out.append(("split", t1_split_only(blk, text, 13)))
    elif family == "T2":
        out.append(("rev", t2_list(blk, text, "rev")))
        out.append(("perm", t2_list(blk, text, "perm", 21)))
    elif family == "T3":
        for total in {"acgtn": (9, 17), "s40": (257,)}.get(name, ()):
            if sigma in (6, 41):
                out.append(("dups%d" % total, t3_dups(blk, text, total, 31)))
    elif family == "T4":
        if name == "acgtn":
            out += [("over" + k, t4_over(name, n, l)) for k, l in t4_lists().items()]
        elif name == "s12":
            out.append(("over257", t4_over(name, n, list(range(-1, 256)))))
    elif family == "T5":
        wide = sigma == 257
        out += [("p%d" % p, t5_primary(blk, text, p)) for p in t5_values(blk, wide)]
        if name in ("acgtn", "s12"):      # the T4 sigma-257 blocks
            b = t4_over(name, n, list(range(-1, 256)))
            out += [("over257_p%d" % p, t5_primary(b, text, p)) for p in t5_values(b, True)]
    elif family == "M1":
        for r in m1_positions(blk):
            out += [("run%d_v%d" % (r, v), m1_bad_index(blk, r, v)) for v in _bad_values(sigma)]
    elif family == "M2":
        out.append(("no_nothing", m2_no_nothing(name, n)))
        if n > 1:
            out += [("second_at_%d" % r, m2_second_nothing(name, n, r)) for r in m2_rows(name, n)]
    elif family == "M3":
        out += [("swap%d" % s, m3_swap(name, n, s)) for s in m3_seeds(name, n)]
    elif family == "M4":
        out += m4_lengths(blk)
    else:
        raise KeyError(family)
    return [(i, b, decode_block_ref(b)) for i, b in out]


FAMILY_BASES = {
    "T1": all_bases(), "T2": all_bases(), "T3": [("acgtn", n) for n in ACGTN_LENGTHS if n >= 255] + [("s40", 70001)],
    "T4": [("acgtn", n) for n in ACGTN_LENGTHS] + [("s12", 4097), ("s12", 70001)],
    "T5": [(a, n) for a, n in all_bases() if a in ("acgtn", "s12", "s40", "b256", "late")],
    "M1": all_bases(), "M2": all_bases(),
    "M3": [(a, n) for a, ns in m3_bases() for n in ns],
    "M4": [("acgtn", 4096), ("s12", 4097), ("s100", 70001), ("b256", 4097)],
}
