#!/usr/bin/env python3
"""FM-index matching statistics and maximal exact matches (tc_fm_match_stats_dev, tc_fm_mems_dev) on 2^28-byte texts.

  python scripts/fm_ms_bench.py --parent-lib OLD.so     # every step, one child process each
  python scripts/fm_ms_bench.py --step ms0              # one step, in this process

Texts: tc_generate_dev kind 0 (iid ACGTN, seed 0xC4: the text of scripts/fm_factorize_bench.py) and kind 2 (genome-like:
iid ACGT with copies of 300-bp families, whose repeats make large intervals).  Batches resident in HBM, 10^6 patterns of
100 bytes each:
  a   exact substrings of the text
  b   substrings with 1 .. 4 planted substitutions (pattern i gets 1 + i % 4; each byte replaced by another letter)
  c   random strings over the text's letters
Steps:
  build    the index with and without the LCP part (tc_fm_build_lcp_dev against tc_fm_build_dev / tc_fm_build_sampled_dev),
           full index and rate 32, both texts; the bytes of part 3
  ms0, ms2 on kind 0 / kind 2, full index and rate-32 index, batches a, b, c: tc_fm_match_stats_dev with ms_len only and
           with all three arrays, tc_fm_mems_dev at min_len 20; the lengths of the two indexes must agree, and on batch a
           every first entry must be the pattern's length
  count    on kind 0: tc_fm_count_dev on the default index and on one built with TC_FM_PAIRS=0 (the same single-symbol
           loop as the matching statistics), the sizes pass of factorize, and ms_len only on batch a, five repeats:
           ms_len-only / count_dev(no pairs), next to factorize sizes / count_dev
  parent   tc_fm_count_dev on batch a with another build of the library (--parent-lib: the parent commit's), five repeats:
           their spread is what "the same rate" means for the exact count, which this change does not touch
Times are wall clock around one call, which returns after the stream has drained; warm; the median of the repeats.

Every step runs in a child process of its own under a time limit; the first failure ends the run (nothing more is started
on a device that has just failed)."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "text-compression_amd"))

NPAT = 1_000_000
M = 100
SEED = {0: 0xC4, 2: 0xC5}
LETTERS = {0: b"ACGTN", 2: b"ACGT"}


def cut(d_text, npat, m, seed):
    import torch
    g = torch.Generator(device="cpu"); g.manual_seed(seed)
    starts = torch.randint(0, d_text.numel() - m, (npat,), generator=g).cuda()
    return d_text[(starts[:, None] + torch.arange(m, device="cuda")[None, :])]


def pack(pats):
    import torch
    npat, m = pats.shape
    flat = torch.cat([pats.reshape(-1), torch.zeros(16, dtype=torch.uint8, device="cuda")])
    offs = (torch.arange(npat + 1, dtype=torch.int64, device="cuda") * m).contiguous()
    return flat, offs


def batches(d_text, kind):
    """{name: (flat uint8 tensor, int64 offsets)} on the device"""
    import torch
    letters = LETTERS[kind]
    a = cut(d_text, NPAT, M, 0xFA00)
    b = cut(d_text, NPAT, M, 0xFB00).clone()
    g = torch.Generator(device="cpu"); g.manual_seed(0xFB01)
    order = torch.rand(NPAT, M, generator=g).cuda().argsort(dim=1)[:, :4]              # 4 distinct positions per pattern
    nxt = torch.arange(256, dtype=torch.uint8, device="cuda")
    for x, y in zip(letters, letters[1:] + letters[:1]):
        nxt[x] = y
    planted = 1 + torch.arange(NPAT, device="cuda") % 4
    old = b.gather(1, order)
    new = torch.where(torch.arange(4, device="cuda")[None, :] < planted[:, None], nxt[old.long()], old)
    b.scatter_(1, order, new)
    g = torch.Generator(device="cpu"); g.manual_seed(0xFC00)
    al = torch.tensor(list(letters), dtype=torch.uint8)
    c = al[torch.randint(0, len(letters), (NPAT, M), generator=g)].cuda()
    return {"a": pack(a), "b": pack(b), "c": pack(c)}


def timed(fn, reps):
    import torch
    ts = []
    for i in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t0
        if i:
            ts.append(dt * 1e3)
    return ts


def stat(ts):
    med = statistics.median(ts)
    return {"ms": [round(t, 3) for t in ts], "median_ms": round(med, 3), "spread_pct": round(100 * (max(ts) - min(ts)) / med, 2)}


def text_of(ctx, kind, n):
    import torch
    d_text = torch.empty(n, dtype=torch.uint8, device="cuda")
    assert ctx.lib.tc_generate_dev(ctx.handle, kind, SEED[kind], n, C.c_void_p(d_text.data_ptr())) == 0
    torch.cuda.synchronize()
    return d_text


def ms_call(ctx, fm, flat, offs, d_len, d_pos, d_occ):
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    ctx._check(ctx.lib.tc_fm_match_stats_dev(ctx.handle, fm._h, p(flat), p(offs), NPAT, p(d_len), p(d_pos), p(d_occ)))


def one(step, log2, reps):
    import torch
    import textcomp
    from textcomp import _lib
    if os.environ.get("TEXTCOMP_LIB"):      # another build may lack the newest entry points: bind what it has
        _lib._prefer_process_hip_runtime()
        probe = C.CDLL(_lib.LIB_PATH)
        _lib.SYMBOLS = [s for s in _lib.SYMBOLS if hasattr(probe, s[0])]
    n = 1 << log2
    ctx = textcomp.Context(0)
    res = {"step": step, "n": n, "patterns": NPAT, "len": M, "lib": os.environ.get("TEXTCOMP_LIB", "in-tree")}
    if step == "build":
        for kind in (0, 2):
            d_text = text_of(ctx, kind, n)
            for rate in (1, 32):
                for lcp in (False, True):
                    def build():
                        fm = ctx.fm_build_dev(d_text, sa_rate=rate, lcp=lcp)
                        b = (fm.device_bytes(0), fm.device_bytes(3))
                        fm.close()
                        return b
                    by = build()
                    row = stat(timed(build, 3))
                    row["bytes"], row["part3_bytes"] = by
                    res["kind%d_rate%d_%s" % (kind, rate, "lcp" if lcp else "plain")] = row
            del d_text
    if step in ("ms0", "ms2"):
        kind = int(step[2])
        d_text = text_of(ctx, kind, n)
        B = batches(d_text, kind)
        d_len = torch.zeros(NPAT * M, dtype=torch.int32, device="cuda")
        d_pos = torch.zeros(NPAT * M, dtype=torch.int64, device="cuda")
        d_occ = torch.zeros(NPAT * M, dtype=torch.int32, device="cuda")
        sums = {}
        for rate in (1, 32):
            fm = ctx.fm_build_dev(d_text, sa_rate=rate, lcp=True)
            for name, (flat, offs) in B.items():
                ms_call(ctx, fm, flat, offs, d_len, d_pos, d_occ)
                mo, ms, mp, ml = fm.mems_dev(flat, offs, NPAT, 20)      # sizes the MEM arrays (and warms up)
                total = ms.numel()
                row = {"mean_ms_len": round(float(d_len.float().mean()), 3), "mems20": total,
                       "len_only": stat(timed(lambda: ms_call(ctx, fm, flat, offs, d_len, None, None), reps)),
                       "all_three": stat(timed(lambda: ms_call(ctx, fm, flat, offs, d_len, d_pos, d_occ), reps)),
                       "mems20_dev": stat(timed(lambda: fm.mems_dev(flat, offs, NPAT, 20, cap=max(total, 1)), reps))}
                row["ns_per_symbol_len_only"] = round(row["len_only"]["median_ms"] * 1e6 / (NPAT * M), 3)
                sums.setdefault(name, []).append((int(d_len.sum()), int(d_pos.sum()), int(d_occ.sum()), int(mp.sum()), int(ml.sum())))
                if name == "a":
                    assert bool((d_len.view(NPAT, M)[:, 0] == M).all()), "a substring of the text matches whole"
                res["rate%d_%s" % (rate, name)] = row
            fm.close()
        for name, s in sums.items():
            assert s[0] == s[1], "the full and the sampled index do not agree on batch " + name
    if step in ("count", "parent"):
        d_text = text_of(ctx, 0, n)
        flat, offs = batches(d_text, 0)["a"]
        fm = ctx.fm_build_dev(d_text)
        res["count_dev"] = stat(timed(lambda: fm.count_dev(flat, offs, NPAT), 5))
        res["count_dev"]["checksum"] = int(fm.count_dev(flat, offs, NPAT).sum())
        if step == "count":
            d_foffs = torch.zeros(NPAT + 1, dtype=torch.int64, device="cuda")

            def sizes():
                nf = C.c_uint64(0)
                ctx._check(ctx.lib.tc_fm_factorize_dev(ctx.handle, fm._h, C.c_void_p(flat.data_ptr()), C.c_void_p(offs.data_ptr()),
                                                       NPAT, C.c_void_p(d_foffs.data_ptr()), None, None, C.byref(nf)))
            res["factor_sizes"] = stat(timed(sizes, 5))
            fm.close()
            os.environ["TC_FM_PAIRS"] = "0"
            fm = ctx.fm_build_dev(d_text, lcp=True)
            os.environ.pop("TC_FM_PAIRS")
            d_len = torch.zeros(NPAT * M, dtype=torch.int32, device="cuda")
            res["count_dev_nopairs"] = stat(timed(lambda: fm.count_dev(flat, offs, NPAT), 5))
            assert int(fm.count_dev(flat, offs, NPAT).sum()) == res["count_dev"]["checksum"]
            res["ms_len_only"] = stat(timed(lambda: ms_call(ctx, fm, flat, offs, d_len, None, None), 5))
            res["ms_len_only_over_count_nopairs"] = round(res["ms_len_only"]["median_ms"] / res["count_dev_nopairs"]["median_ms"], 3)
            res["sizes_over_count_dev"] = round(res["factor_sizes"]["median_ms"] / res["count_dev"]["median_ms"], 3)
        fm.close()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=("build", "ms0", "ms2", "count", "parent"))
    ap.add_argument("--log2", type=int, default=28)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lib")
    ap.add_argument("--parent-lib", help="libtextcomp.so of the parent commit (the `parent` step is skipped without it)")
    ap.add_argument("--timeout", type=int, default=420, help="seconds per step")
    a = ap.parse_args()
    if a.lib:
        os.environ["TEXTCOMP_LIB"] = os.path.abspath(a.lib)
    if a.step:
        one(a.step, a.log2, a.reps)
        return
    rows = {}
    for step in ("build", "ms0", "ms2", "count") + (("parent",) if a.parent_lib else ()):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--log2", str(a.log2), "--reps", str(a.reps)]
        if step == "parent":
            cmd += ["--lib", a.parent_lib]
        p = subprocess.run(["timeout", "-k", "10", str(a.timeout)] + cmd, capture_output=True, text=True)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-3000:])
            sys.exit("step %s failed (exit %d): nothing more is started" % (step, p.returncode))
        rows[step] = json.loads(p.stdout.strip().splitlines()[-1])
    b = rows["build"]
    for kind in (0, 2):
        for rate in (1, 32):
            pl, lc = b["kind%d_rate%d_plain" % (kind, rate)], b["kind%d_rate%d_lcp" % (kind, rate)]
            print("# kind %d rate %2d | build %8.3f ms, with the LCP part %8.3f ms | index %d bytes, part 3 %d bytes"
                  % (kind, rate, pl["median_ms"], lc["median_ms"], lc["bytes"], lc["part3_bytes"]))
    for kind in (0, 2):
        r = rows["ms%d" % kind]
        for name in "abc":
            f, s = r["rate1_" + name], r["rate32_" + name]
            print("# kind %d batch %s | mean ms_len %7.3f | full index: ms_len only %8.3f ms (%.3f ns / symbol), all three %8.3f ms, mems(20) %8.3f ms (%d MEMs) | rate 32: %8.3f / %8.3f / %8.3f ms"
                  % (kind, name, f["mean_ms_len"], f["len_only"]["median_ms"], f["ns_per_symbol_len_only"], f["all_three"]["median_ms"],
                     f["mems20_dev"]["median_ms"], f["mems20"], s["len_only"]["median_ms"], s["all_three"]["median_ms"],
                     s["mems20_dev"]["median_ms"]))
        print("# kind %d | batch b / batch a (the price of the shrinks), ms_len only on the full index: %.3f"
              % (kind, r["rate1_b"]["len_only"]["median_ms"] / r["rate1_a"]["len_only"]["median_ms"]))
    c = rows["count"]
    print("# batch a | count_dev %8.3f ms (spread %.2f %%), without pair vectors %8.3f ms | ms_len only %8.3f ms = %.3f x count_dev(no pairs) | factorize sizes / count_dev = %.3f"
          % (c["count_dev"]["median_ms"], c["count_dev"]["spread_pct"], c["count_dev_nopairs"]["median_ms"], c["ms_len_only"]["median_ms"],
             c["ms_len_only_over_count_nopairs"], c["sizes_over_count_dev"]))
    if "parent" in rows:
        par = rows["parent"]
        print("# batch a | parent count_dev %8.3f ms (five repeats %s, spread %.2f %%); this build / parent = %.3f"
              % (par["count_dev"]["median_ms"], par["count_dev"]["ms"], par["count_dev"]["spread_pct"],
                 c["count_dev"]["median_ms"] / par["count_dev"]["median_ms"]))
        if par["count_dev"]["checksum"] != c["count_dev"]["checksum"]:
            sys.exit("the two builds do not agree on the counts")


if __name__ == "__main__":
    main()
