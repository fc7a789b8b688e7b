#!/usr/bin/env python3
"""FM-index factorize / unfactorize (tc_fm_factorize_dev, tc_fm_unfactorize_dev) on a 2^28-byte iid ACGTN text.

  python scripts/fm_factorize_bench.py --parent-lib OLD.so     # every step, one child process each
  python scripts/fm_factorize_bench.py --step factorize        # one step, in this process

Text: tc_generate_dev kind 0, seed 0xC4 (the text of scripts/fm_locate_bench.py).  Batches resident in HBM, 10^6 patterns
of 100 bytes each:
  a   exact substrings of the text: one factor each
  b   substrings with 1 .. 4 planted substitutions (pattern i gets 1 + i % 4; each byte replaced by another letter)
  c   two substrings of 50 bytes joined
Steps:
  factorize    tc_fm_factorize_dev on a full index and on a rate-32 index, batches a, b, c: the sizes-only form and the whole
               call; the factors of the two indexes must agree
  unfactorize  tc_fm_unfactorize_dev of the factors of batches a, b, c on an index with text_rate 32; the bytes must be the
               patterns
  count        tc_fm_count_dev and tc_fm_count_mm_dev (k = 0) on batch a, five repeats, and the sizes pass of factorize on
               the same batch: the ratios sizes / count_dev and count_mm(k = 0) / count_dev
  parent       tc_fm_count_dev and tc_fm_count_mm_dev (k = 0) on batch a with another build of the library (--parent-lib:
               the parent commit's), five repeats: their spread is what "the same rate" means for the exact count, which
               this change does not touch
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


def batches(d_text):
    """{name: (flat uint8 tensor, int64 offsets)} on the device"""
    import torch
    a = cut(d_text, NPAT, M, 0xFA00)
    b = cut(d_text, NPAT, M, 0xFB00).clone()
    g = torch.Generator(device="cpu"); g.manual_seed(0xFB01)
    order = torch.rand(NPAT, M, generator=g).cuda().argsort(dim=1)[:, :4]              # 4 distinct positions per pattern
    nxt = torch.arange(256, dtype=torch.uint8, device="cuda")
    for x, y in zip(b"ACGTN", b"CGTAA"):
        nxt[x] = y
    planted = 1 + torch.arange(NPAT, device="cuda") % 4
    old = b.gather(1, order)
    new = torch.where(torch.arange(4, device="cuda")[None, :] < planted[:, None], nxt[old.long()], old)
    b.scatter_(1, order, new)
    c = torch.cat([cut(d_text, NPAT, M // 2, 0xFC00), cut(d_text, NPAT, M // 2, 0xFC01)], dim=1)
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


def sizes_only(ctx, fm, flat, offs, d_foffs):
    nf = C.c_uint64(0)
    ctx._check(ctx.lib.tc_fm_factorize_dev(ctx.handle, fm._h, C.c_void_p(flat.data_ptr()), C.c_void_p(offs.data_ptr()), NPAT,
                                           C.c_void_p(d_foffs.data_ptr()), None, None, C.byref(nf)))
    return int(nf.value)


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
    d_text = torch.empty(n, dtype=torch.uint8, device="cuda")
    assert ctx.lib.tc_generate_dev(ctx.handle, 0, 0xC4, n, C.c_void_p(d_text.data_ptr())) == 0
    torch.cuda.synchronize()
    res = {"step": step, "n": n, "patterns": NPAT, "len": M, "lib": os.environ.get("TEXTCOMP_LIB", "in-tree")}
    B = batches(d_text)
    d_foffs = torch.zeros(NPAT + 1, dtype=torch.int64, device="cuda")
    if step in ("count", "parent"):
        fm = ctx.fm_build_dev(d_text)
        flat, offs = B["a"]
        res["count_dev"] = stat(timed(lambda: fm.count_dev(flat, offs, NPAT), 5))
        res["count_dev"]["checksum"] = int(fm.count_dev(flat, offs, NPAT).sum())
        res["count_mm_k0"] = stat(timed(lambda: fm.count_mm_dev(flat, offs, NPAT, 0), 5))
        assert int(fm.count_mm_dev(flat, offs, NPAT, 0).sum()) == res["count_dev"]["checksum"]
        if step == "count":
            assert sizes_only(ctx, fm, flat, offs, d_foffs) == NPAT, "a substring of the text is one factor"
            res["factor_sizes"] = stat(timed(lambda: sizes_only(ctx, fm, flat, offs, d_foffs), 5))
            res["sizes_over_count_dev"] = round(res["factor_sizes"]["median_ms"] / res["count_dev"]["median_ms"], 3)
        res["k0_over_count_dev"] = round(res["count_mm_k0"]["median_ms"] / res["count_dev"]["median_ms"], 3)
        fm.close()
    if step == "factorize":
        sums = {}
        for rate in (1, 32):
            fm = ctx.fm_build_dev(d_text, sa_rate=rate)
            for name, (flat, offs) in B.items():
                foffs, fpos, flen = fm.factorize_dev(flat, offs, NPAT)        # sizes the factor arrays (and warms up)
                total = fpos.numel()
                row = {"factors": total, "per_pattern": round(total / NPAT, 3), "literals": int((flen == 0).sum()),
                       "sizes": stat(timed(lambda: sizes_only(ctx, fm, flat, offs, d_foffs), reps)),
                       "all": stat(timed(lambda: fm.factorize_dev(flat, offs, NPAT, cap=total), reps))}
                row["Mpatterns_per_s"] = round(NPAT / row["all"]["median_ms"] / 1e3, 2)
                sums.setdefault(name, []).append((int(foffs.sum()), int(fpos.sum()), int(flen.sum())))
                res["rate%d_%s" % (rate, name)] = row
            fm.close()
        for name, s in sums.items():
            assert s[0] == s[1], "the full and the sampled index do not agree on the factors of batch " + name
        assert res["rate1_a"]["factors"] == NPAT and res["rate1_a"]["literals"] == 0
    if step == "unfactorize":
        fm = ctx.fm_build_dev(d_text, sa_rate=32, text_rate=32)
        for name, (flat, offs) in B.items():
            foffs, fpos, flen = fm.factorize_dev(flat, offs, NPAT)
            ooffs, out = fm.unfactorize_dev(foffs, fpos, flen, NPAT, cap=NPAT * M)
            assert torch.equal(out, flat[:NPAT * M]) and torch.equal(ooffs, offs), "the round trip of batch %s is not the identity" % name
            row = stat(timed(lambda: fm.unfactorize_dev(foffs, fpos, flen, NPAT, cap=NPAT * M), reps))
            row["factors"] = fpos.numel()
            row["GB_per_s"] = round(NPAT * M / row["median_ms"] / 1e6, 2)
            res["text_rate32_%s" % name] = row
        fm.close()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=("factorize", "unfactorize", "count", "parent"))
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
    for step in ("factorize", "unfactorize", "count") + (("parent",) if a.parent_lib else ()):
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
    f, u, c = rows["factorize"], rows["unfactorize"], rows["count"]
    for name in "abc":
        print("# batch %s | %.3f factors / pattern | factorize_dev: full %8.3f ms (sizes %8.3f), rate 32 %8.3f ms | unfactorize_dev (text_rate 32) %8.3f ms"
              % (name, f["rate1_" + name]["per_pattern"], f["rate1_" + name]["all"]["median_ms"], f["rate1_" + name]["sizes"]["median_ms"],
                 f["rate32_" + name]["all"]["median_ms"], u["text_rate32_" + name]["median_ms"]))
    print("# batch a | count_dev %8.3f ms (spread %.2f %%) | count_mm k=0 / count_dev = %.3f | factorize sizes / count_dev = %.3f"
          % (c["count_dev"]["median_ms"], c["count_dev"]["spread_pct"], c["k0_over_count_dev"], c["sizes_over_count_dev"]))
    if "parent" in rows:
        par = rows["parent"]
        print("# batch a | parent count_dev %8.3f ms (five repeats %s, spread %.2f %%); this build / parent = %.3f; over the parent's count_dev: count_mm k=0 %.3f (parent's own %.3f), factorize sizes %.3f"
              % (par["count_dev"]["median_ms"], par["count_dev"]["ms"], par["count_dev"]["spread_pct"],
                 c["count_dev"]["median_ms"] / par["count_dev"]["median_ms"], c["count_mm_k0"]["median_ms"] / par["count_dev"]["median_ms"],
                 par["k0_over_count_dev"], c["factor_sizes"]["median_ms"] / par["count_dev"]["median_ms"]))
        if par["count_dev"]["checksum"] != c["count_dev"]["checksum"]:
            sys.exit("the two builds do not agree on the counts")


if __name__ == "__main__":
    main()
