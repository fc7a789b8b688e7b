"""CPU reference, models and inputs for the segmented sort of a doubling round (seg_sort_pairs in csrc/tc_sa_host.hpp,
kernels in csrc/tc_seg.hpp) and for tied_small_kernel, as the debug entries tc_dbg_seg_sort / tc_dbg_tied_small of
include/textcomp_debug.h run them.  Nothing here needs the library or a GPU.

  seg_sort_ref / seg_sort_mismatch   the operation: inside every run of equal grp the members ordered by rank
  levels_ref                         the partition levels (seg_init_kernel / seg_scan_kernel) as a plain model
  windows_ref                        what every 3072-slot window of seg_small_kernel finds (mid, tiny, merge, lw)
  CASES                              seeded, named inputs; each says what it is for, tests/test_seg_ref.py asserts that
                                     from the two models, tests/test_gpu_seg_sort.py runs them on the device
  tied_small_ref, TIED_CASES         the same for tied_small_kernel
"""
import collections
import functools

import numpy as np

# ---- the geometry, restated from csrc/tc_seg.hpp
SEG_W = 4096          # slots of a window's image
SEG_CAP = 1024        # runs up to this length are sorted in LDS
SEG_SPAN = SEG_W - SEG_CAP   # slots a window is responsible for
SEG_PT = 4096         # members of a tile of a partition level
SEG_TINY = 15         # runs of 2 .. 15 members count in LDS instead of going through the network
SEG_LEVELS = 8        # levels seg_sort_pairs runs before it gives up
VOID = 0xffffffff


# ---- the operation ---------------------------------------------------------------------------------------------------
def seg_sort_ref(keys, vals):
    """the pairs ordered by (key, val): keys are grp << 32 | rank with grp non-decreasing, so this is the sort inside
    every run of equal grp; the order of values inside a stretch of equal keys is the reference's own choice"""
    o = np.lexsort((vals, keys))
    return keys[o], vals[o]


def seg_sort_mismatch(keys, vals, out_keys, out_vals):
    """None if (out_keys, out_vals) is an accepted result for the input (keys, vals), else the first slot at which it
    is not.  Accepted: the keys are the sorted keys, slot by slot, and the pairs, put into (key, val) order, are the
    reference's -- every stretch of equal keys holds the same values, in any order.  Every slot is compared."""
    rk, rv = seg_sort_ref(keys, vals)
    if out_keys.shape != rk.shape or out_vals.shape != rv.shape:
        return 0
    bad = np.nonzero(out_keys != rk)[0]
    if len(bad):
        return int(bad[0])
    o = np.lexsort((out_vals, out_keys))
    bad = np.nonzero(out_vals[o] != rv)[0]   # (out_keys[o] == rk already: the keys are sorted)
    if len(bad):
        # a slot of the stretch of equal keys whose values differ
        k = rk[bad[0]]
        lo = int(np.searchsorted(rk, k, "left"))
        hi = int(np.searchsorted(rk, k, "right"))
        want = set(rv[lo:hi].tolist())
        for i in range(lo, hi):
            if int(out_vals[i]) not in want:
                return i
        return lo
    return None


def runs_of(keys):
    """(starts, sizes) of the runs of equal grp"""
    grp = (keys >> np.uint64(32)).astype(np.uint64)
    heads = np.ones(len(keys), bool)
    heads[1:] = grp[1:] != grp[:-1]
    starts = np.nonzero(heads)[0]
    sizes = np.diff(np.append(starts, len(keys)))
    return starts, sizes


# ---- the partition levels --------------------------------------------------------------------------------------------
Levels = collections.namedtuple("Levels", "st splits relists relist_events unlisted heads overflow")


def levels_ref(keys, rbits):
    """The levels seg_sort_pairs runs for these keys.
    st             [(S, T)] per level with S > 0: listed runs, and tiles = sum of ceil(size / 4096)
    splits[i]      how often slot i changed buffers (its parity says which buffer holds it at the end)
    relists[i]     how often the run that holds slot i was listed again in place with a new shift
    relist_events  such re-listings, counted per run
    unlisted       children above 1024 members that a split with shift 0 left off the next list (they hold equal ranks)
    heads[i]       slot i starts a run when seg_small_kernel looks (the groups' heads and every child's)
    overflow       runs were still listed after 8 levels (the library answers TC_ERR_INTERNAL)"""
    m = len(keys)
    rank = (keys & np.uint64(0xffffffff)).astype(np.uint64)
    starts, sizes = runs_of(keys)
    heads = np.zeros(m, bool)
    heads[starts] = True
    splits = np.zeros(m, np.int32)
    relists = np.zeros(m, np.int32)
    # the members of a listed run as a multiset of ranks: a level is unstable, only the children's contents are defined
    listed = [(int(s), np.sort(rank[s:s + z]), max(rbits - 8, 0)) for s, z in zip(starts, sizes) if z > SEG_CAP]
    st, events, unlisted = [], 0, 0
    for _ in range(SEG_LEVELS):
        if not listed:
            break
        st.append((len(listed), sum(-(-len(r) // SEG_PT) for _, r, _ in listed)))
        nxt = []
        for start, r, shift in listed:
            rmin, rmax = int(r.min()), int(r.max())
            if rmin == rmax:
                continue
            digit = (r >> np.uint64(shift)) & np.uint64(255)
            if int(digit.min()) == int(digit.max()):
                hb = (rmin ^ rmax).bit_length() - 1
                nxt.append((start, r, max(hb - 7, 0)))
                relists[start:start + len(r)] += 1
                events += 1
                continue
            splits[start:start + len(r)] += 1
            o = np.argsort(digit, kind="stable")
            cnt = np.bincount(digit[o].astype(np.int64), minlength=256)
            pos = start
            at = 0
            for c in cnt:
                c = int(c)
                if c:
                    heads[pos] = True
                    if c > SEG_CAP and shift > 0:
                        nxt.append((pos, r[o[at:at + c]], max(shift - 8, 0)))
                    elif c > SEG_CAP:
                        unlisted += 1
                pos += c
                at += c
        listed = nxt
    else:
        return Levels(st, splits, relists, events, unlisted, heads, bool(listed))
    return Levels(st, splits, relists, events, unlisted, heads, False)


def levels_words(lv):
    """the 16 words tc_dbg_seg_sort reports"""
    out = [0] * (2 * SEG_LEVELS)
    for L, (s, t) in enumerate(lv.st):
        out[2 * L], out[2 * L + 1] = s, t
    return out


# ---- the windows of seg_small_kernel -----------------------------------------------------------------------------------
Window = collections.namedtuple("Window", "mid tiny merge lw last_end")


def windows_ref(keys, heads=None):
    """Per 3072-slot window: members of its mid runs (16 .. 1024), of its tiny runs (2 .. 15), whether the tiny ones
    join the network (both kinds present and one power of two holds mid and mid + tiny alike), lw = log2 of the network's
    size (None: no network), and the image slot behind its last run of 2 .. 1024 members (None: no such run).  From
    the run sizes alone; heads: the run heads after the partition levels (levels_ref), default the groups' own."""
    m = len(keys)
    if heads is None:
        starts, sizes = runs_of(keys)
    else:
        starts = np.nonzero(heads)[0]
        sizes = np.diff(np.append(starts, m))
    out = []
    for w in range(-(-m // SEG_SPAN)):
        sel = (starts >= w * SEG_SPAN) & (starts < (w + 1) * SEG_SPAN) & (sizes <= SEG_CAP)
        sz = sizes[sel]
        nm = int(sz[sz > SEG_TINY].sum())
        nt = int(sz[(sz >= 2) & (sz <= SEG_TINY)].sum())
        la = lb = 4
        while (1 << la) < nm:
            la += 1
        while (1 << lb) < nm + nt:
            lb += 1
        merge = nm > 0 and nt > 0 and la == lb
        nmid = nm + (nt if merge else 0)
        lw = None
        if nmid:
            lw = 4
            while (1 << lw) < nmid:
                lw += 1
        sel &= sizes >= 2
        last_end = int((starts[sel] + sizes[sel]).max()) - w * SEG_SPAN if sel.any() else None
        out.append(Window(nm, nt, merge, lw, last_end))
    return out


# ---- inputs ----------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name family keys vals rbits what")

PATTERNS = ("rand", "equal", "two", "asc", "desc", "small4", "ends", "bit0", "bit31")


def ranks_of(pattern, size, rng, rbits=32):
    """`size` ranks below 2^rbits"""
    top = 1 << rbits
    if pattern == "rand":
        r = rng.integers(0, top, size, dtype=np.uint64)
    elif pattern == "equal":
        r = np.full(size, rng.integers(0, top), np.uint64)
    elif pattern == "two":
        a, b = rng.choice(top, 2, replace=False) if top <= 1 << 20 else rng.integers(0, top, 2)
        r = np.where(rng.integers(0, 2, size) == 1, np.uint64(a), np.uint64(b)).astype(np.uint64)
        if size >= 2:
            r[0], r[-1] = a, b
    elif pattern in ("asc", "desc"):
        r = np.sort(rng.integers(0, top, size, dtype=np.uint64))
        if pattern == "desc":
            r = r[::-1].copy()
    elif pattern == "small4":
        r = rng.integers(0, min(4, top), size, dtype=np.uint64)
    elif pattern == "ends":
        r = rng.integers(0, top, size, dtype=np.uint64)
        if size >= 2:
            i, j = rng.choice(size, 2, replace=False)
            r[i], r[j] = 0, top - 1
    elif pattern in ("bit0", "bit31"):
        bit = np.uint64(0 if pattern == "bit0" else min(31, rbits - 1))
        base = rng.integers(0, top, dtype=np.uint64) & ~(np.uint64(1) << bit)
        r = base | (rng.integers(0, 2, size, dtype=np.uint64) << bit)
        if size >= 2:
            r[0], r[-1] = base, base | (np.uint64(1) << bit)
    else:
        raise ValueError(pattern)
    return r.astype(np.uint64)


def _grps(nruns, rng):
    """strictly increasing 32-bit group values: the first 0, the last 0xffffffff, most neighbours 1 apart"""
    if nruns == 1:
        return np.array([int(rng.choice([0, VOID, 0x80000000]))], np.uint64)
    steps = rng.choice(np.array([1, 1, 1, 50021], np.uint64), nruns - 1)
    g = np.concatenate([[0], np.cumsum(steps)]).astype(np.uint64)
    assert int(g[-2]) < VOID
    g[-1] = VOID
    return g


def assemble(runs, rng, rbits=32):
    """runs: a list of rank arrays, one per group, in slot order -> (keys, vals); vals a permutation of 0 .. m - 1"""
    g = _grps(len(runs), rng)
    keys = np.concatenate([(g[i] << np.uint64(32)) | r.astype(np.uint64) for i, r in enumerate(runs)]).astype(np.uint64)
    vals = rng.permutation(len(keys)).astype(np.uint32)
    return keys, vals


def _singles(count, rng, rbits=32):
    return [ranks_of("rand", 1, rng, rbits) for _ in range(count)]


CASES = collections.OrderedDict()


def _add(name, family, runs, rng, what, rbits=32):
    assert name not in CASES, name
    keys, vals = assemble(runs, rng, rbits)
    assert 1 <= len(keys) <= 1 << 17
    keys.setflags(write=False)
    vals.setflags(write=False)
    CASES[name] = Case(name, family, keys, vals, rbits, what)


def _rng(*tag):
    return np.random.default_rng([0x5E6] + [int(t) for t in tag])


# -- ladder: every size class on both sides of 15 / 16, 1024 / 1025 and the 4096-member tile
LADDER = [1, 2, 3, 14, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1026, 2047, 2048, 4095, 4096,
          4097, 8191, 8192, 8193]
LADDER_LEADS = (0, 1, 37, 63)
for _d, _sizes in (("up", LADDER), ("down", LADDER[::-1])):
    for _lead in LADDER_LEADS:
        _r = _rng(1, _d == "down", _lead)
        _add("ladder_%s_lead%d" % (_d, _lead), "ladder",
             _singles(_lead, _r) + [ranks_of("rand", z, _r) for z in _sizes], _r,
             "runs of every ladder size back to back, random 32-bit ranks, behind %d singletons" % _lead)

# -- rank patterns
PATTERN_SIZES = [2, 15, 16, 17, 1024, 1025, 5000]
for _p in PATTERNS[1:]:
    _r = _rng(2, PATTERNS.index(_p))
    _add("pat_" + _p, "patterns", [ranks_of(_p, z, _r) for z in PATTERN_SIZES], _r,
         "runs of 2, 15, 16, 17, 1024, 1025 and 5000 members with '%s' ranks" % _p)
RBITS = (1, 8, 9, 17)
for _b in RBITS:
    _r = _rng(3, _b)
    _add("rbits_%d" % _b, "patterns", [ranks_of("rand", z, _r, _b) for z in (1025, 5000)], _r,
         "runs of 1025 and 5000 members, random ranks below 2^%d, rbits = %d" % (_b, _b), rbits=_b)

# -- window edges
EDGE_HEADS = (3070, 3071, 3072, 3073)
EDGE_SIZES = (2, 15, 16, 1023, 1024)
for _w in (0, 1):
    for _h in EDGE_HEADS:
        for _z in EDGE_SIZES:
            _r = _rng(4, _w, _h, _z)
            _add("edge_w%d_h%d_s%d" % (_w, _h, _z), "edges",
                 _singles(_w * SEG_SPAN + _h, _r) + [ranks_of("rand", _z, _r)] + _singles(3, _r) + [ranks_of("rand", 7, _r)], _r,
                 "singletons up to a head on slot %d of window %d, a run of %d there, then three singletons and a run of 7"
                 % (_h, _w, _z))
_r = _rng(5)
_add("edge_full_window", "edges", [ranks_of("rand", z, _r) for z in (1024, 1024, 1023, 1024)] + _singles(5, _r), _r,
     "runs of 1024, 1024, 1023 and 1024 from slot 0: the fourth is headed at slot 3071; 4095 mid members in window 0")
TOTALS = (1, 2, 63, 64, 65, 3071, 3072, 3073, 4096, 4097)
TOTAL_LASTS = (2, 16, 1024)
for _m in TOTALS:
    for _z in TOTAL_LASTS if _m > 1 else (1,):
        if _z > _m:
            continue
        _r = _rng(6, _m, _z)
        _add("total_m%d_last%d" % (_m, _z), "edges", _singles(_m - _z, _r) + [ranks_of("rand", _z, _r)], _r,
             "%d members in all: singletons, then a run of %d that ends on the last slot" % (_m, _z))
TAIL_MODS = (0, 1, 63)
TAIL_LONGS = (1025, 4097)
for _mod in TAIL_MODS:
    for _z in TAIL_LONGS:
        _r = _rng(7, _mod, _z)
        _lead = 200 + (_mod - (200 + _z)) % 64
        _add("tail_mod%d_long%d" % (_mod, _z), "edges",
             _singles(_lead - 40, _r) + [ranks_of("rand", 40, _r)] + [ranks_of("rand", _z, _r)], _r,
             "m %% 64 = %d with a last run of %d members" % (_mod, _z))

# -- network size and merge: window 0 holds exactly nm mid and nt tiny members
NETWORK = [(16, 0), (17, 0), (0, 15), (0, 45), (17, 15), (17, 16), (32, 14), (33, 30), (1024, 15), (2048, 1000), (2049, 2000),
           # (added so that every network size occurs: lw = 7, 8 and 9)
           (65, 0), (129, 100), (300, 200)]
TINY_LONGEST = (2, 7, 15)


def _partition(total, lo, hi, rng):
    """sizes in lo .. hi that sum to total"""
    out = []
    while total:
        if total <= hi and total >= lo:
            z = total if total < 2 * lo or rng.integers(0, 2) else int(rng.integers(lo, min(hi, total - lo) + 1))
        else:
            z = int(rng.integers(lo, min(hi, total - lo) + 1))
        out.append(z)
        total -= z
    return out


def _tiny_sizes(nt, longest, rng):
    """tiny run sizes (2 .. longest) that sum to nt, one of them `longest` where the sum allows it"""
    if nt == 0:
        return []
    longest = min(longest, nt)
    if longest == 2 and nt % 2:
        return [3] + [2] * ((nt - 3) // 2)          # (an odd count cannot be made of pairs: one run of 3)
    if nt - longest == 1:
        return [longest - 1, 2]                      # (no run of 1 member is tiny)
    return [longest] + _partition(nt - longest, 2, longest, rng)


for _nm, _nt in NETWORK:
    for _t in TINY_LONGEST if _nt else (0,):
        _r = _rng(8, _nm, _nt, _t)
        if _nm + _nt > SEG_SPAN:                    # every head inside the window: a run of 1024 carries the excess
            _mid = [SEG_CAP] + _partition(_nm - SEG_CAP, 16, SEG_CAP, _r)
        else:
            _mid = _partition(_nm, 16, SEG_CAP, _r) if _nm else []
        _tiny = _tiny_sizes(_nt, _t, _r)
        assert sum(_mid) == _nm and sum(_tiny) == _nt and all(2 <= z <= SEG_TINY for z in _tiny)
        _runs = [("m", z) for z in sorted(_mid)[:-1]] + [("t", z) for z in _tiny]
        _runs = [_runs[i] for i in _r.permutation(len(_runs))]
        if _mid:
            _runs.append(("m", max(_mid)))           # the longest mid run last: it may reach over the window's own slots
        _arr = [ranks_of("rand", z, _r) if k == "m" else ranks_of("small4", z, _r) for k, z in _runs]
        _used = _nm + _nt
        _fill = max(SEG_SPAN - _used, 0) + 10        # singletons up to the window's end and a few into the next
        _add("net_m%d_t%d_l%d" % (_nm, _nt, _t), "network", _arr + _singles(_fill, _r), _r,
             "window 0 holds %d mid and %d tiny members (longest tiny run %d, ranks of tiny runs from {0, 1, 2, 3})"
             % (_nm, _nt, max(_tiny) if _tiny else 0))


# -- depth of the partition levels
def _depth_a(rng, size=9000):
    abc = rng.integers(0, 2, (3, size), dtype=np.uint64)
    return (abc[0] << np.uint64(24)) | (abc[1] << np.uint64(16)) | (abc[2] << np.uint64(8)) | rng.integers(0, 256, size, dtype=np.uint64)


def _depth_b(rng, size=9000):
    return np.uint64(0x12345000) + rng.integers(0, 4096, size, dtype=np.uint64)


def _depth_c(rng, size=3000):
    return np.uint64(0x12000000) + (rng.integers(0, 2, size, dtype=np.uint64) << np.uint64(20)) + rng.integers(0, 16, size, dtype=np.uint64)


def _depth_e(rng):
    """level-0 digits 3, 4 and 5 hold exactly 1024, 1025 and 700 members"""
    d = np.repeat(np.array([3, 4, 5], np.uint64), [1024, 1025, 700])
    r = (d << np.uint64(24)) | rng.integers(0, 1 << 24, len(d), dtype=np.uint64)
    return r[rng.permutation(len(r))]


_r = _rng(9, 1)
_add("depth_a", "depth", [_depth_a(_r)], _r, "9000 members, ranks a<<24 | b<<16 | c<<8 | d with a, b, c in {0, 1}: three levels list children, four splits")
_r = _rng(9, 2)
_add("depth_b", "depth", [_depth_b(_r)], _r, "9000 members, ranks 0x12345000 + rand(4096): level 0 re-lists, level 1 splits, done")
_r = _rng(9, 3)
_add("depth_c", "depth", [_depth_c(_r)], _r, "3000 members, ranks base + (j << 20) + rand(16): re-list, split, re-list, split")
_r = _rng(9, 4)
_add("depth_d", "depth", _singles(37, _r) + [_depth_a(_r), _depth_b(_r), _depth_c(_r), ranks_of("rand", 1025, _r)], _r,
     "depth_a, _b, _c and a 1025-member run back to back behind 37 singletons: starts off the 64-slot words, neighbours in other buffers")
_r = _rng(9, 5)
_add("depth_e", "depth", _singles(11, _r) + [_depth_e(_r)] + _singles(3, _r), _r,
     "a run whose level-0 children have exactly 1024, 1025 and 700 members: only the 1025 is listed again")
TILE_K = (1, 2, 3)
for _k in TILE_K:
    for _x in (0, 1):
        _r = _rng(9, 6, _k, _x)
        _add("depth_f_%d" % (SEG_PT * _k + _x), "depth", _singles(5, _r) + [ranks_of("rand", SEG_PT * _k + _x, _r)] + _singles(2, _r), _r,
             "a long run of %d members: %d tiles" % (SEG_PT * _k + _x, _k + _x))

# -- mix
MIX_SEEDS = range(20)
MIX_MEANS = (3, 40, 700, 3000)
for _s in MIX_SEEDS:
    _r = _rng(10, _s)
    _arr, _tot, _i = [], 0, 0
    while _tot < 30000:
        _z = int(min(_r.geometric(1.0 / MIX_MEANS[_i % 4]), 20000))
        _arr.append(ranks_of(PATTERNS[int(_r.integers(0, len(PATTERNS)))], _z, _r))
        _tot += _z
        _i += 1
    _add("mix_%02d" % _s, "mix", _arr, _r, "run lengths geometric with means 3, 40, 700, 3000 in turn, rank patterns drawn per run")

@functools.lru_cache(maxsize=None)
def model(name):
    """(levels_ref, windows_ref after the levels) of a case, computed once"""
    c = CASES[name]
    lv = levels_ref(c.keys, c.rbits)
    return lv, windows_ref(c.keys, lv.heads)


FAMILIES = ("ladder", "patterns", "edges", "network", "depth", "mix")
FAMILY_LAST = {f: [n for n, c in CASES.items() if c.family == f][-1] for f in FAMILIES}


# ---- tied_small_kernel -------------------------------------------------------------------------------------------------
def tied_small_ref(mode, slot, idx, grp):
    """mode 0: (slot, idx, grp) ordered by slot, void entries (slot = 0xffffffff) last, in any order among themselves;
    mode 1: (t_idx, t_rank, tpos): idx sorted, the group of the member at each row, the row of each member"""
    if mode == 0:
        o = np.argsort(slot, kind="stable")
        return slot[o], idx[o], grp[o]
    o = np.argsort(idx, kind="stable")
    tpos = np.empty(len(idx), np.uint32)
    tpos[o] = np.arange(len(idx), dtype=np.uint32)
    return idx[o], grp[o], tpos


def tied_small_mismatch(mode, slot, idx, grp, out):
    """None if the three arrays `out` are an accepted result, else a description of the first difference"""
    ref = tied_small_ref(mode, slot, idx, grp)
    if mode == 1:
        for nm, a, b in zip(("t_idx", "t_rank", "tpos"), out, ref):
            bad = np.nonzero(a != b)[0]
            if len(bad):
                return "%s differs first at %d: %d, expected %d" % (nm, bad[0], a[bad[0]], b[bad[0]])
        return None
    live = int((slot != VOID).sum())
    for nm, a, b in zip(("slot", "idx", "grp"), out, ref):
        bad = np.nonzero(a[:live] != b[:live])[0]
        if len(bad):
            return "%s differs first at %d: %d, expected %d" % (nm, bad[0], a[bad[0]], b[bad[0]])
    if not (out[0][live:] == VOID).all():
        return "a void entry is not among the last %d" % (len(slot) - live)
    got = sorted(zip(out[1][live:].tolist(), out[2][live:].tolist()))
    want = sorted(zip(ref[1][live:].tolist(), ref[2][live:].tolist()))
    return None if got == want else "the void entries' (idx, grp) differ as a multiset"


TiedCase = collections.namedtuple("TiedCase", "name mode slot idx grp what")
TIED_M = (1, 2, 15, 16, 17, 31, 32, 33, 127, 128, 129, 255, 256, 257, 2047, 2048, 2049, 4095, 4096)
TIED_CASES = collections.OrderedDict()


def _tied(m, mode, voids):
    rng = _rng(11, m, mode, voids)
    slot = rng.choice(1 << 32, m, replace=False).astype(np.uint64)
    slot[slot >= VOID - 1] = 12345                  # (0xfffffffe and 0xffffffff are placed below, nowhere else)
    slot = np.unique(slot)
    while len(slot) < m:
        slot = np.unique(np.append(slot, rng.integers(1, VOID - 1, m - len(slot))))
    slot = slot[rng.permutation(m)].astype(np.uint32)
    if mode == 0:
        slot[int(rng.integers(0, m))] = 0
        if m >= 2:
            j = int(rng.integers(0, m))
            while slot[j] == 0:
                j = (j + 1) % m
            slot[j] = VOID - 1
        if voids:
            free = np.nonzero((slot != 0) & (slot != VOID - 1))[0]
            slot[rng.choice(free, voids, replace=False)] = VOID
    idx = rng.choice(1 << 31, m, replace=False).astype(np.uint32)
    grp = rng.integers(0, 1 << 32, m, dtype=np.uint64).astype(np.uint32)
    for a in (slot, idx, grp):
        a.setflags(write=False)
    what = ("%d members with distinct slots, 0 and 0xfffffffe among them, %d void" % (m, voids)) if mode == 0 else \
        "%d members with distinct text positions" % m
    return TiedCase("tied%d_m%d" % (mode, m) + ("_v%d" % voids if voids else ""), mode, slot, idx, grp, what)


for _m in TIED_M:
    for _v in sorted({0, 1, 5, _m // 2}):
        if _v == 0 or _v <= _m - 2:
            _c = _tied(_m, 0, _v)
            TIED_CASES[_c.name] = _c
    _c = _tied(_m, 1, 0)
    TIED_CASES[_c.name] = _c
