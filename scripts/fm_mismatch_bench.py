#!/usr/bin/env python3
"""FM-index search with mismatches (tc_fm_count_mm_dev, tc_fm_locate_mm_dev) on a 2^28-byte iid ACGTN text.

  python scripts/fm_mismatch_bench.py --parent-lib OLD.so      # every step, one child process each
  python scripts/fm_mismatch_bench.py --step count             # one step, in this process

Text: tc_generate_dev kind 0, seed 0xC4 (the text of BASELINE configs[3]).  Batches resident in HBM: 10^6 patterns of 32 and
of 100 bytes cut from the text, with k planted substitutions (k distinct positions, each byte replaced by another letter).
Steps:
  count    tc_fm_count_mm_dev at k = 0 .. 3 on both lengths, and tc_fm_count_dev on the k = 0 batches (five repeats)
  locate   tc_fm_locate_mm_dev at k = 1 on a full index and on a rate-32 index
  parent   tc_fm_count_dev on the k = 0 batches with another build of the library (--parent-lib: the parent commit's),
           five repeats: their spread is what "the same rate" means for the exact count, which this change does not touch
Times are wall clock around one call, which returns after the stream has drained; warm; the median of the repeats.  A
search costs one dependent random 64-byte line per node visited: `Glines/s` is what the exact count of the same batch
reads (symbols / 2 with pair steps, from the second symbol on) over its time -- the yardstick of profiles/r03_fm_sweep.txt.

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
LENGTHS = (32, 100)


def cut(d_text, npat, m, k, seed):
    """npat substrings of length m with k planted substitutions -> (flat uint8 tensor, int64 offsets), on the device"""
    import torch
    g = torch.Generator(device="cpu"); g.manual_seed(seed)
    starts = torch.randint(0, d_text.numel() - m, (npat,), generator=g).cuda()
    pats = d_text[(starts[:, None] + torch.arange(m, device="cuda")[None, :])]
    if k:
        where = torch.rand(npat, m, generator=g).cuda().argsort(dim=1)[:, :k]          # k distinct positions per pattern
        nxt = torch.arange(256, dtype=torch.uint8, device="cuda")
        for a, b in zip(b"ACGTN", b"CGTAA"):
            nxt[a] = b
        pats.scatter_(1, where, nxt[pats.gather(1, where).long()])
    flat = torch.cat([pats.reshape(-1), torch.zeros(16, dtype=torch.uint8, device="cuda")])
    offs = (torch.arange(npat + 1, dtype=torch.int64, device="cuda") * m).contiguous()
    return flat, offs


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
    lib = ctx.lib
    d_text = torch.empty(n, dtype=torch.uint8, device="cuda")
    assert lib.tc_generate_dev(ctx.handle, 0, 0xC4, n, C.c_void_p(d_text.data_ptr())) == 0
    torch.cuda.synchronize()
    res = {"step": step, "n": n, "patterns": NPAT, "lib": os.environ.get("TEXTCOMP_LIB", "in-tree")}
    fm = ctx.fm_build_dev(d_text)
    for m in LENGTHS:
        row = {}
        flat0, offs0 = cut(d_text, NPAT, m, 0, 0xC4E0 + m)
        if step in ("count", "parent"):
            ts = timed(lambda: fm.count_dev(flat0, offs0, NPAT), 5)
            lines = NPAT * (1 + (m - 1) // 2 + (m - 1) % 2 - 1)          # the table step, then pair steps (and one single)
            row["count_dev"] = {"ms": [round(t, 3) for t in ts], "median_ms": round(statistics.median(ts), 3),
                                "spread_pct": round(100 * (max(ts) - min(ts)) / statistics.median(ts), 2),
                                "Glines_per_s": round(lines / statistics.median(ts) / 1e6, 1),
                                "checksum": int(fm.count_dev(flat0, offs0, NPAT).sum())}
        if step == "count":
            for k in range(4):
                flat, offs = (flat0, offs0) if k == 0 else cut(d_text, NPAT, m, k, 0xC4E0 + m + 1000 * k)
                out = fm.count_mm_dev(flat, offs, NPAT, k)
                assert int((out == 0).sum()) == 0, "a pattern cut from the text with k substitutions has a hit"
                ts = timed(lambda: fm.count_mm_dev(flat, offs, NPAT, k), reps if k < 3 else min(reps, 3))
                ms = statistics.median(ts)
                row["count_mm_k%d" % k] = {"median_ms": round(ms, 3), "min_ms": round(min(ts), 3),
                                           "Mpatterns_per_s": round(NPAT / ms / 1e3, 2), "hits": int(out.sum())}
            row["k0_over_count_dev"] = round(row["count_mm_k0"]["median_ms"] / row["count_dev"]["median_ms"], 3)
            assert row["count_mm_k0"]["hits"] == row["count_dev"]["checksum"]
        if step == "locate":
            flat, offs = cut(d_text, NPAT, m, 1, 0xC4E0 + m + 1000)
            for rate in (1, 32):
                f = fm if rate == 1 else ctx.fm_build_dev(d_text, sa_rate=rate)
                hoffs, hits, mm = f.locate_mm_dev(flat, offs, NPAT, 1)     # sizes the hit arrays (and warms up)
                total = hits.numel()
                ts = timed(lambda: f.locate_mm_dev(flat, offs, NPAT, 1, cap=total), reps)
                ms = statistics.median(ts)
                row["locate_mm_k1_rate%d" % rate] = {"median_ms": round(ms, 3), "min_ms": round(min(ts), 3), "hits": total,
                                                    "Mhits_per_s": round(total / ms / 1e3, 2),
                                                    "checksum": int(hits.sum()) + int(mm.sum())}
                if rate != 1:
                    f.close()
        res["len%d" % m] = row
    fm.close()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=("count", "locate", "parent"))
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
    for step in ("count", "locate") + (("parent",) if a.parent_lib else ()):
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
    for m in LENGTHS:
        c = rows["count"]["len%d" % m]
        print("# len %3d | count_dev %8.3f ms (spread %.2f %%, %.1f Glines/s) | count_mm k=0..3: %s ms | k=0 / count_dev = %.3f"
              % (m, c["count_dev"]["median_ms"], c["count_dev"]["spread_pct"], c["count_dev"]["Glines_per_s"],
                 "  ".join("%.3f" % c["count_mm_k%d" % k]["median_ms"] for k in range(4)), c["k0_over_count_dev"]))
        loc = rows["locate"]["len%d" % m]
        print("# len %3d | locate_mm k=1: full %8.3f ms, rate 32 %8.3f ms (%d hits)"
              % (m, loc["locate_mm_k1_rate1"]["median_ms"], loc["locate_mm_k1_rate32"]["median_ms"], loc["locate_mm_k1_rate1"]["hits"]))
        if loc["locate_mm_k1_rate1"]["checksum"] != loc["locate_mm_k1_rate32"]["checksum"]:
            sys.exit("the full and the sampled index do not agree on the hits")
        if "parent" in rows:
            par = rows["parent"]["len%d" % m]["count_dev"]
            print("# len %3d | parent count_dev %8.3f ms (five repeats %s, spread %.2f %%); this build / parent = %.3f; count_mm k=0 / parent = %.3f"
                  % (m, par["median_ms"], par["ms"], par["spread_pct"], c["count_dev"]["median_ms"] / par["median_ms"],
                     c["count_mm_k0"]["median_ms"] / par["median_ms"]))
            if par["checksum"] != c["count_dev"]["checksum"]:
                sys.exit("the two builds do not agree on the counts")


if __name__ == "__main__":
    main()
