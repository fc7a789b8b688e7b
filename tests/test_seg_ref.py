"""CPU-only: the reference and the models of tests/seg_ref.py checked on inputs small enough to work out by hand, and
every named case checked against what it says it is for -- from levels_ref / windows_ref alone, so that a case that
stops reaching its path fails here instead of passing on the device for nothing (tests/test_gpu_seg_sort.py)."""
import numpy as np
import pytest

import seg_ref as S

U64 = np.uint64


def _keys(grps, ranks):
    return (np.asarray(grps, U64) << U64(32)) | np.asarray(ranks, U64)


def _tiles(sizes):
    return sum(-(-z // S.SEG_PT) for z in sizes)


# ---- the reference itself ---------------------------------------------------------------------------------------------
def test_reference_sorts_inside_runs_only():
    keys = _keys([0, 0, 0, 7, 7, S.VOID], [5, 1, 3, 2, 0, 9])
    vals = np.arange(6, dtype=np.uint32)
    rk, rv = S.seg_sort_ref(keys, vals)
    assert (rk & U64(0xffffffff)).tolist() == [1, 3, 5, 0, 2, 9]
    assert rv.tolist() == [1, 2, 0, 4, 3, 5]
    assert S.seg_sort_mismatch(keys, vals, rk, rv) is None


def test_mismatch_accepts_any_order_of_equal_keys_and_nothing_else():
    keys = _keys([3, 3, 3, 3, 4], [8, 8, 1, 8, 0])
    vals = np.array([10, 11, 12, 13, 14], np.uint32)
    rk, rv = S.seg_sort_ref(keys, vals)
    assert rv.tolist() == [12, 10, 11, 13, 14]
    assert S.seg_sort_mismatch(keys, vals, rk, np.array([12, 13, 10, 11, 14], np.uint32)) is None
    assert S.seg_sort_mismatch(keys, vals, rk, np.array([10, 12, 11, 13, 14], np.uint32)) in (0, 1)   # a value under another key
    assert S.seg_sort_mismatch(keys, vals, rk, np.array([12, 10, 10, 13, 14], np.uint32)) in (1, 2)   # one twice, one lost
    assert S.seg_sort_mismatch(keys, vals, keys, vals) == 0                                           # unsorted keys
    wrong = rk.copy()
    wrong[4] ^= U64(1)
    assert S.seg_sort_mismatch(keys, vals, wrong, rv) == 4
    assert S.seg_sort_mismatch(keys, vals, rk[:4], rv[:4]) == 0


def test_levels_of_hand_made_runs():
    rng = np.random.default_rng(1)
    # no run above 1024: no level
    assert S.levels_ref(_keys([1] * 1024 + [2] * 1024, rng.integers(0, 1 << 32, 2048)), 32).st == []
    # 1025 equal ranks: listed once, dropped, never moved
    lv = S.levels_ref(_keys([1] * 1025, [77] * 1025), 32)
    assert lv.st == [(1, 1)] and lv.splits.max() == 0 and lv.relist_events == 0 and lv.heads.sum() == 1
    # two top digits, 2000 and 3000 members, distinct low bits below: split, both children listed with shift 16, split again
    r = np.concatenate([(U64(1) << U64(24)) | (rng.integers(0, 256, 2000).astype(U64) << U64(16)),
                        (U64(9) << U64(24)) | (rng.integers(0, 256, 3000).astype(U64) << U64(16))])
    lv = S.levels_ref(_keys([5] * 5000, rng.permutation(r)), 32)
    assert lv.st == [(1, 2), (2, 2)] and (lv.splits == 2).all() and lv.heads[2000] and lv.unlisted == 0
    # rbits = 8: level 0 has shift 0, its children of 2000 and 3000 equal ranks are not listed
    lv = S.levels_ref(_keys([5] * 5000, [3] * 2000 + [200] * 3000), 8)
    assert lv.st == [(1, 2)] and (lv.splits == 1).all() and lv.unlisted == 2
    # ranks that differ in bit 5 only: re-listed with shift 0 (hb = 5), then split, children not listed
    lv = S.levels_ref(_keys([5] * 4097, [0x40000000 | (32 * (i & 1)) for i in range(4097)]), 32)
    assert lv.st == [(1, 2), (1, 2)] and (lv.relists == 1).all() and (lv.splits == 1).all() and lv.unlisted == 2
    # hb = 20: shift 13
    lv = S.levels_ref(_keys([5] * 1100, [0x12000000 | ((i & 1) << 20) for i in range(1100)]), 32)
    assert lv.st == [(1, 1), (1, 1)] and lv.heads.sum() == 2 and lv.heads[550] and not lv.overflow
    assert S.levels_words(lv) == [1, 1, 1, 1] + [0] * 12


def test_windows_of_hand_made_runs():
    def sizes_keys(sizes):
        return _keys(np.repeat(np.arange(len(sizes)), sizes), np.zeros(sum(sizes), U64))
    w = S.windows_ref(sizes_keys([1, 15, 16, 1, 2]))
    assert w == [S.Window(16, 17, False, 4, 35)]              # 16 -> 2^4, 33 -> 2^6: the tiny runs count on their own
    w = S.windows_ref(sizes_keys([17, 15]))
    assert w == [S.Window(17, 15, True, 5, 32)]               # 17 and 32 both fit 2^5
    w = S.windows_ref(sizes_keys([3071, 1024, 1]))            # a long run, then a head on the window's last slot
    assert w[0] == S.Window(1024, 0, False, 10, 4095) and w[1] == S.Window(0, 0, False, None, None)
    w = S.windows_ref(sizes_keys([3072, 1024]))               # the same one slot later: the next window's
    assert w[0] == S.Window(0, 0, False, None, None) and w[1] == S.Window(1024, 0, False, 10, 1024)
    w = S.windows_ref(sizes_keys([1025, 14]))
    assert w == [S.Window(0, 14, False, None, 1039)]


# ---- every case: well-formed ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(S.CASES))
def test_case_is_well_formed(name):
    c = S.CASES[name]
    m = len(c.keys)
    assert 1 <= m <= 1 << 17 and c.keys.dtype == np.uint64 and c.vals.dtype == np.uint32 and len(c.vals) == m
    grp = c.keys >> U64(32)
    assert (grp[1:] >= grp[:-1]).all()
    assert 1 <= c.rbits <= 32 and int((c.keys & U64(0xffffffff)).max()) < 1 << c.rbits
    assert np.array_equal(np.sort(c.vals), np.arange(m, dtype=np.uint32))
    assert c.what and c.family in S.FAMILIES
    u = np.unique(grp)
    if len(u) > 1:
        assert int(u[0]) == 0 and int(u[-1]) == S.VOID
    if len(u) > 8:
        assert (np.diff(u) == 1).any()
    assert not S.model(name)[0].overflow


def test_cases_are_seeded():
    import importlib
    a = {n: (c.keys.copy(), c.vals.copy()) for n, c in S.CASES.items()}
    T = importlib.reload(S)
    assert list(T.CASES) == list(a)
    for n, (k, v) in a.items():
        assert np.array_equal(T.CASES[n].keys, k) and np.array_equal(T.CASES[n].vals, v)


# ---- what each family is for --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", ("up", "down"))
@pytest.mark.parametrize("lead", S.LADDER_LEADS)
def test_ladder(d, lead):
    name = "ladder_%s_lead%d" % (d, lead)
    _, sizes = S.runs_of(S.CASES[name].keys)
    ladder = S.LADDER if d == "up" else S.LADDER[::-1]
    assert sizes.tolist() == [1] * lead + ladder
    for a in (15, 1024, 4095, 4096, 8192):      # both sides of tiny / mid, mid / long and of the tile
        assert a in ladder and a + 1 in ladder
    lv, win = S.model(name)
    big = [z for z in ladder if z > S.SEG_CAP]
    assert len(big) == 10 and lv.st == [(10, _tiles(big))]      # random 32-bit ranks: one level, 256 small children each
    assert sorted(set(lv.splits.tolist())) == [0, 1] and int((lv.splits == 1).sum()) == sum(big)
    assert any(w.mid for w in win) and any(w.tiny for w in win)


def test_rank_patterns():
    for p in S.PATTERNS[1:]:
        c = S.CASES["pat_" + p]
        _, sizes = S.runs_of(c.keys)
        assert sizes.tolist() == S.PATTERN_SIZES
        assert S.model("pat_" + p)[0].st[0] == (2, 1 + 2)
    rank = {p: S.CASES["pat_" + p].keys & U64(0xffffffff) for p in S.PATTERNS[1:]}
    starts, sizes = S.runs_of(S.CASES["pat_equal"].keys)
    for p, r in rank.items():
        for s, z in zip(starts, sizes):
            x = r[s:s + z]
            d = int(np.bitwise_xor.reduce(np.unique(x))) if len(np.unique(x)) == 2 else None
            if p == "equal":
                assert len(np.unique(x)) == 1
            if p == "two":
                assert len(np.unique(x)) == 2
            if p == "asc":
                assert (x[1:] >= x[:-1]).all() and x[0] < x[-1]
            if p == "desc":
                assert (x[1:] <= x[:-1]).all() and x[0] > x[-1]
            if p == "small4":
                assert int(x.max()) <= 3
            if p == "ends":
                assert int(x.min()) == 0 and int(x.max()) == 0xffffffff
            if p == "bit0":
                assert d == 1
            if p == "bit31":
                assert d == 1 << 31
    # equal ranks: the runs are listed, found equal, and never touched
    lv = S.model("pat_equal")[0]
    assert lv.st == [(2, 3)] and lv.splits.max() == 0 and lv.relist_events == 0
    # a level with shift 0 whose children above 1024 are not listed again
    for n in ("pat_bit0", "pat_small4", "rbits_1"):
        assert S.model(n)[0].unlisted > 0, n
    assert S.model("pat_bit0")[0].st == [(2, 3), (2, 3)] and S.model("pat_bit0")[0].relist_events == 2
    # two values, far apart: children of ~2500 equal ranks ARE listed (shift 16) and dropped there
    assert S.model("pat_two")[0].st == [(2, 3), (2, 2)]
    for b in S.RBITS:
        c = S.CASES["rbits_%d" % b]
        assert c.rbits == b and S.runs_of(c.keys)[1].tolist() == [1025, 5000]
        assert int((c.keys & U64(0xffffffff)).max()).bit_length() == b       # the top bit of the width is used
        assert S.model(c.name)[0].st == [(2, 3)]
    assert S.model("rbits_8")[0].unlisted == 0 and S.model("rbits_1")[0].unlisted == 2   # (the halves of 5000)


@pytest.mark.parametrize("w", (0, 1))
@pytest.mark.parametrize("h", S.EDGE_HEADS)
@pytest.mark.parametrize("z", S.EDGE_SIZES)
def test_window_edge(w, h, z):
    name = "edge_w%d_h%d_s%d" % (w, h, z)
    starts, sizes = S.runs_of(S.CASES[name].keys)
    at = w * S.SEG_SPAN + h
    assert (sizes[:at] == 1).all() and starts[at] == at and sizes[at] == z and sizes[at + 1:].tolist() == [1, 1, 1, 7]
    lv, win = S.model(name)
    assert lv.st == []
    ww, hh = (w, h) if h < S.SEG_SPAN else (w + 1, h - S.SEG_SPAN)       # the window that owns the head
    mine = win[ww]
    if hh + z + 3 < S.SEG_SPAN:
        assert (mine.mid, mine.tiny) == ((z, 7) if z > S.SEG_TINY else (0, z + 7))
    else:
        assert (mine.mid, mine.tiny, mine.last_end) == ((z, 0, hh + z) if z > S.SEG_TINY else (0, z, hh + z))
    if h == 3071 and z == 1024:
        assert mine.last_end == S.SEG_W - 1        # the run fills the image up to its last slot
    for x in range(ww):
        assert win[x] == S.Window(0, 0, False, None, None)        # singletons only: nothing to sort there


def test_full_window():
    starts, sizes = S.runs_of(S.CASES["edge_full_window"].keys)
    assert sizes[:4].tolist() == [1024, 1024, 1023, 1024] and starts[3] == S.SEG_SPAN - 1
    assert S.model("edge_full_window")[1][0] == S.Window(4095, 0, False, 12, 4095)


def test_total_lengths():
    seen = set()
    for m in S.TOTALS:
        for z in S.TOTAL_LASTS if m > 1 else (1,):
            if z > m:
                continue
            c = S.CASES["total_m%d_last%d" % (m, z)]
            starts, sizes = S.runs_of(c.keys)
            assert len(c.keys) == m and sizes[-1] == z and starts[-1] + z == m and (sizes[:-1] == 1).all()
            seen.add((m, z))
    assert len(seen) == 1 + 1 + 3 * 2 + 5 * 3
    for mod in S.TAIL_MODS:
        for z in S.TAIL_LONGS:
            c = S.CASES["tail_mod%d_long%d" % (mod, z)]
            starts, sizes = S.runs_of(c.keys)
            assert len(c.keys) % 64 == mod and sizes[-1] == z >= 1025 and starts[-1] + z == len(c.keys)
            assert S.model(c.name)[0].st == [(1, -(-z // S.SEG_PT))]


# what the kernel's rule (la == lb) says of each pair.  (2049, 2000) merges: 2049 and 4049 both need 2^12 -- above 2048 mid
# members every window does
NETWORK_MERGES = {(17, 15): True, (17, 16): False, (32, 14): False, (33, 30): True, (1024, 15): False, (2048, 1000): False,
                  (2049, 2000): True, (129, 100): True, (300, 200): True}
NETWORK_LW = {(16, 0): 4, (17, 0): 5, (0, 15): None, (0, 45): None, (17, 15): 5, (17, 16): 5, (32, 14): 5, (33, 30): 6,
              (1024, 15): 10, (2048, 1000): 11, (2049, 2000): 12, (65, 0): 7, (129, 100): 8, (300, 200): 9}


def test_network_size_and_merge():
    lws, counted_ties = set(), 0
    assert set(NETWORK_LW) == set(S.NETWORK)
    for nm, nt in S.NETWORK:
        longest_seen = set()
        for t in S.TINY_LONGEST if nt else (0,):
            name = "net_m%d_t%d_l%d" % (nm, nt, t)
            c = S.CASES[name]
            lv, win = S.model(name)
            assert lv.st == []
            w = win[0]
            assert (w.mid, w.tiny) == (nm, nt), name
            assert w.merge == NETWORK_MERGES.get((nm, nt), False), name
            assert w.lw == NETWORK_LW[(nm, nt)], name
            assert all(x == S.Window(0, 0, False, None, None) for x in win[1:])
            lws.add(w.lw)
            starts, sizes = S.runs_of(c.keys)
            tiny = [(s, z) for s, z in zip(starts, sizes) if 2 <= z <= S.SEG_TINY]
            if tiny:
                longest_seen.add(max(z for _, z in tiny))
                ties = sum(len(np.unique(c.keys[s:s + z])) < z for s, z in tiny)
                if not w.merge:
                    counted_ties += ties       # equal ranks in a tiny run that counts in LDS: the j < p tie-break decides
        if nt >= 17:
            assert longest_seen == {2 + nt % 2, 7, 15}, (nm, nt, longest_seen)
    assert lws >= set(range(4, 13))
    assert counted_ties >= 100


def test_depth():
    lv, _ = S.model("depth_a")          # three levels list children (2, 4, 8 of them), four splits, no re-list
    assert len(S.CASES["depth_a"].keys) == 9000
    assert [s for s, _ in lv.st] == [1, 2, 4, 8] and (lv.splits == 4).all() and lv.relist_events == 0
    lv, _ = S.model("depth_b")          # level 0 re-lists, level 1 splits, done
    assert lv.st == [(1, 3), (1, 3)] and (lv.relists == 1).all() and (lv.splits == 1).all()
    lv, _ = S.model("depth_c")          # re-list, split, re-list, split
    assert lv.st == [(1, 1), (1, 1), (2, 2), (2, 2)] and (lv.relists == 2).all() and (lv.splits == 2).all()
    assert lv.relist_events == 3
    c = S.CASES["depth_d"]
    lv, _ = S.model("depth_d")
    starts, sizes = S.runs_of(c.keys)
    assert sizes[37:].tolist() == [9000, 9000, 3000, 1025] and all(s % 64 for s in starts[37:])
    assert len(lv.st) == 4 and lv.st[0] == (4, 3 + 3 + 1 + 1)
    par = lv.splits & 1
    assert [int(lv.splits[s]) for s in starts[37:]] == [4, 1, 2, 1]
    diff = np.nonzero(par[1:] != par[:-1])[0]
    assert len(diff) >= 3 and all(i // 64 == (i + 1) // 64 for i in diff)     # both buffers inside one 64-bit word
    lv, _ = S.model("depth_e")          # children of exactly 1024 and 1025: only the second is listed again
    assert lv.st == [(1, 1), (1, 1)] and lv.heads[11] and lv.heads[11 + 1024] and lv.heads[11 + 2049]
    assert set(lv.splits[11:11 + 1024].tolist()) == {1} and set(lv.splits[11 + 1024:11 + 2049].tolist()) == {2}
    for k in S.TILE_K:
        for x in (0, 1):
            z = S.SEG_PT * k + x
            assert S.runs_of(S.CASES["depth_f_%d" % z].keys)[1].tolist() == [1] * 5 + [z] + [1, 1]
            assert S.model("depth_f_%d" % z)[0].st == [(1, k + x)]


def test_mix():
    classes = set()
    deepest = 0
    for s in S.MIX_SEEDS:
        name = "mix_%02d" % s
        _, sizes = S.runs_of(S.CASES[name].keys)
        lv, win = S.model(name)
        assert lv.st and len(win) >= 9
        deepest = max(deepest, len(lv.st))
        classes |= {("single", "tiny", "mid", "long")[(z > 1) + (z > S.SEG_TINY) + (z > S.SEG_CAP)] for z in sizes.tolist()}
    assert classes == {"single", "tiny", "mid", "long"} and deepest >= 2


# ---- tied_small_kernel ---------------------------------------------------------------------------------------------------
def test_tied_reference():
    slot = np.array([9, S.VOID, 0, 4, S.VOID], np.uint32)
    idx = np.array([50, 51, 52, 53, 54], np.uint32)
    grp = np.array([7, 8, 9, 10, 11], np.uint32)
    rs, ri, rg = S.tied_small_ref(0, slot, idx, grp)
    assert rs.tolist() == [0, 4, 9, S.VOID, S.VOID] and ri[:3].tolist() == [52, 53, 50] and rg[:3].tolist() == [9, 10, 7]
    assert S.tied_small_mismatch(0, slot, idx, grp, (rs, ri, rg)) is None
    swapped = (rs, np.array([52, 53, 50, 54, 51], np.uint32), np.array([9, 10, 7, 11, 8], np.uint32))
    assert S.tied_small_mismatch(0, slot, idx, grp, swapped) is None            # void entries in the other order
    torn = (rs, np.array([52, 53, 50, 54, 51], np.uint32), rg)
    assert S.tied_small_mismatch(0, slot, idx, grp, torn) is not None           # ... but each keeps its own grp
    assert S.tied_small_mismatch(0, slot, idx, grp, (slot, idx, grp)) is not None
    idx = np.array([30, 10, 20], np.uint32)
    grp = np.array([1, 2, 3], np.uint32)
    t = S.tied_small_ref(1, None, idx, grp)
    assert t[0].tolist() == [10, 20, 30] and t[1].tolist() == [2, 3, 1] and t[2].tolist() == [2, 0, 1]
    assert S.tied_small_mismatch(1, None, idx, grp, t) is None
    assert S.tied_small_mismatch(1, None, idx, grp, (t[0], t[1], np.array([2, 1, 0], np.uint32))) is not None


def test_tied_cases():
    sizes = set()
    for name, c in S.TIED_CASES.items():
        m = len(c.idx)
        sizes.add(m)
        assert 1 <= m <= S.SEG_W and len(c.slot) == m and len(c.grp) == m
        assert len(np.unique(c.idx)) == m
        if c.mode == 0:
            live = c.slot[c.slot != S.VOID]
            assert len(np.unique(live)) == len(live) and 0 in live and (m < 2 or S.VOID - 1 in live)
            voids = m - len(live)
            assert name == "tied0_m%d" % m + ("_v%d" % voids if voids else "")
    assert sizes == set(S.TIED_M)
    for m in S.TIED_M:
        assert "tied1_m%d" % m in S.TIED_CASES and "tied0_m%d" % m in S.TIED_CASES
        for v in (1, 5, m // 2):
            if 1 <= v <= m - 2:
                assert "tied0_m%d_v%d" % (m, v) in S.TIED_CASES
