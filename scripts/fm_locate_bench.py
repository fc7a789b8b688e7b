#!/usr/bin/env python3
"""FM-index locate from a sampled suffix array against the full one (tc_fm_build_sampled_dev, tc_fm_locate_dev).

  python scripts/fm_locate_bench.py                     # rates 1 4 16 32 64 128 on a 2^28-byte iid ACGTN text, one child each
  python scripts/fm_locate_bench.py --rate 32 --log2 28 # one rate, in this process
  python scripts/fm_locate_bench.py --build-only --lib OTHER.so   # build time of tc_fm_build_dev of another build

Text: tc_generate_dev kind 0, seed 0xC4 (the text of BASELINE configs[3]).  Two batches cut from the text, resident in
HBM: 10^6 patterns of length 14 (about one hit each) and 10^4 of length 6 (about 2^28 / 5^6 = 1.7e4 hits each).  Per
rate: device bytes of the index (all, locate part), build time, and for each batch the time of one tc_fm_locate_dev call
(wall clock around the call, which returns after the stream has drained; warm; median of 5), hits/s, and the mean number
of LF steps per hit -- not instrumented but read off the answers: a hit at 1-based position p took (p - 1) mod rate
steps (expected (rate - 1) / 2).  The call includes the backward search and the scan of the hit counts, which rate 1
pays too: `walk` is the time above rate 1 of the same run, and `model` what (3 lines per step x mean steps + 3 for the
sampled row) would take at 50 G random 64-byte lines/s (profiles/r03_fm_sweep.txt).

Every rate is measured in a child process of its own under a time limit; the first failure ends the run (nothing more is
started on a device that has just failed)."""
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

LINES_PER_S = 50e9


def cut(d_text, npat, m, seed):
    import torch
    g = torch.Generator(device="cpu"); g.manual_seed(seed)
    starts = torch.randint(0, d_text.numel() - m, (npat,), generator=g).cuda()
    pos = (starts[:, None] + torch.arange(m, device="cuda")[None, :]).reshape(-1)
    flat = torch.cat([d_text[pos], torch.zeros(16, dtype=torch.uint8, device="cuda")])
    offs = (torch.arange(npat + 1, dtype=torch.int64, device="cuda") * m).contiguous()
    return flat, offs


def one(rate, log2, reps, build_only):
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
    res = {"rate": rate, "n": n, "lib": os.environ.get("TEXTCOMP_LIB", "in-tree")}
    ts = []
    fm = None
    for i in range(4):                       # the first build also grows the workspace
        if fm is not None:
            fm.close()
        t0 = time.perf_counter()
        fm = ctx.fm_build_dev(d_text) if build_only else ctx.fm_build_dev(d_text, sa_rate=rate)
        if i:
            ts.append((time.perf_counter() - t0) * 1e3)
    res["build_ms"] = round(statistics.median(ts), 2)
    if build_only:
        print(json.dumps(res), flush=True)
        return
    res["index_bytes"], res["locate_bytes"] = fm.device_bytes(0), fm.device_bytes(1)
    res["locate_bytes_per_text_byte"] = round(fm.device_bytes(1) / n, 4)
    for name, npat, m in (("len14", 1_000_000, 14), ("len6", 10_000, 6)):
        flat, offs = cut(d_text, npat, m, 0xC4E0 + m)
        hoffs, hits = fm.locate_dev(flat, offs, npat)      # sizes the hit array (and warms up)
        total = hits.numel()
        cap = C.c_uint64()
        ts = []
        for i in range(reps + 1):
            torch.cuda.synchronize()
            cap.value = total
            t0 = time.perf_counter()
            rc = lib.tc_fm_locate_dev(ctx.handle, fm._h, C.c_void_p(flat.data_ptr()), C.c_void_p(offs.data_ptr()), npat,
                                      C.c_void_p(hoffs.data_ptr()), C.c_void_p(hits.data_ptr()), C.byref(cap))
            dt = time.perf_counter() - t0
            assert rc == 0 and cap.value == total
            if i:
                ts.append(dt * 1e3)
        ms = statistics.median(ts)
        steps = float(((hits - 1) % rate).double().mean()) if total else 0.0
        res[name] = {"patterns": npat, "hits": total, "locate_ms": round(ms, 3), "min_ms": round(min(ts), 3),
                     "Mhits_per_s": round(total / ms / 1e3, 1), "mean_lf_steps": round(steps, 3),
                     "model_walk_ms": round(total * (3 * steps + 3) / LINES_PER_S * 1e3, 3) if rate > 1 else 0.0,
                     "checksum": int(hits.sum())}
    fm.close()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rate", type=int)
    ap.add_argument("--log2", type=int, default=28)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--build-only", action="store_true")
    ap.add_argument("--lib")
    ap.add_argument("--rates", type=int, nargs="*", default=[1, 4, 16, 32, 64, 128])
    a = ap.parse_args()
    if a.lib:
        os.environ["TEXTCOMP_LIB"] = os.path.abspath(a.lib)
    if a.rate is not None or a.build_only:
        one(a.rate or 1, a.log2, a.reps, a.build_only)
        return
    rows = []
    for k in a.rates:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--rate", str(k), "--log2", str(a.log2), "--reps", str(a.reps)],
                           capture_output=True, text=True, timeout=300)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-3000:])
            sys.exit("rate %d failed (exit %d): nothing more is started" % (k, p.returncode))
        rows.append(json.loads(p.stdout.strip().splitlines()[-1]))
    base = {nm: rows[0][nm] for nm in ("len14", "len6")} if rows and rows[0]["rate"] == 1 else None
    print("# rate | locate part B/text B | index MB | build ms | len14: ms  Mhits/s  steps  walk ms (model) | len6: ms  Mhits/s  steps  walk ms (model)")
    for r in rows:
        cells = []
        for nm in ("len14", "len6"):
            b = r[nm]
            walk = (b["locate_ms"] - base[nm]["locate_ms"]) if base else float("nan")
            cells.append("%8.3f %8.1f %7.2f %8.3f (%7.3f)" % (b["locate_ms"], b["Mhits_per_s"], b["mean_lf_steps"], walk, b["model_walk_ms"]))
        print("# %4d | %6.4f | %8.1f | %7.1f | %s | %s" % (r["rate"], r["locate_bytes_per_text_byte"], r["index_bytes"] / 1e6, r["build_ms"], cells[0], cells[1]))
    if base and len({(r["len14"]["checksum"], r["len6"]["checksum"]) for r in rows}) != 1:
        sys.exit("the rates do not agree on the hits")
    print("# every rate returned the same hits (sum of positions per batch)")


if __name__ == "__main__":
    main()
