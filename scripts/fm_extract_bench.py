#!/usr/bin/env python3
"""FM-index extract: text ranges read back from the index (tc_fm_build_self_dev, tc_fm_extract_dev).

  python scripts/fm_extract_bench.py                        # text rates 16 32 64 (ranges) and 32 (whole text), one child each
  python scripts/fm_extract_bench.py --rate 32 --log2 28    # one rate, in this process
  python scripts/fm_extract_bench.py --rate 32 --whole      # the whole text as one query

Text: tc_generate_dev kind 0, seed 0xC4 on 2^28 bytes (the text of scripts/fm_locate_bench.py).  Queries resident in HBM:
10^6 ranges of 100 bytes at random starts, or the whole text as one query.  Per run: device bytes of the extract part, and
the time of one tc_fm_extract_dev call (wall clock around the call, which returns after the stream has drained; warm;
median of 5, min beside it), bytes/s, and the LF steps of the batch -- not instrumented but computed from the queries as
the kernel walks them: a segment [max(a, k r), min(e, (k + 1) r)) of a query [a, e) reads anchor - lo last-column bytes
(anchor = min((k + 1) r, n)) and takes one step fewer.  `ns_per_step` is the call (plan, two scans and the walk) over
those steps: the figure to hold against the locate walk's, walk ms over hits x mean steps of scripts/fm_locate_bench.py at
rate 32 in the same run.  The answer is compared with the text on the device.

Every run is a child process of its own under a time limit; the first failure ends the run (nothing more is started on
a device that has just failed)."""
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


def steps_of(starts0, lens, rate, n):
    """(last-column bytes read, LF steps taken) by the walks of the queries [a, a + len), as fm_extract_walk_kernel cuts them"""
    import torch
    a, e = starts0, starts0 + lens
    k0, k1 = a // rate, (e - 1) // rate
    segs = torch.where(lens > 0, k1 - k0 + 1, torch.zeros_like(a))
    # all segments but the last end at their own upper boundary; the last one's anchor is min((k1 + 1) r, n)
    last_anchor = torch.clamp((k1 + 1) * rate, max=n)
    reads = torch.where(lens > 0, last_anchor - a, torch.zeros_like(a))
    return int(reads.sum()), int((reads - segs).sum())


def one(rate, log2, reps, whole, nq, qlen):
    import torch
    import textcomp
    n = 1 << log2
    ctx = textcomp.Context(0)
    lib = ctx.lib
    d_text = torch.empty(n, dtype=torch.uint8, device="cuda")
    assert lib.tc_generate_dev(ctx.handle, 0, 0xC4, n, C.c_void_p(d_text.data_ptr())) == 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fm = ctx.fm_build_dev(d_text, sa_rate=32, text_rate=rate)
    res = {"text_rate": rate, "sa_rate": 32, "n": n, "mode": "whole" if whole else "ranges", "first_build_ms": round((time.perf_counter() - t0) * 1e3, 1),
           "index_bytes": fm.device_bytes(0), "extract_bytes": fm.device_bytes(2), "extract_bytes_per_text_byte": round(fm.device_bytes(2) / n, 4)}
    if whole:
        starts0 = torch.zeros(1, dtype=torch.int64, device="cuda"); lens = torch.full((1,), n, dtype=torch.int64, device="cuda")
    else:
        g = torch.Generator(device="cpu"); g.manual_seed(0xE7AC + rate)
        starts0 = torch.randint(0, n - qlen, (nq,), generator=g).cuda(); lens = torch.full((nq,), qlen, dtype=torch.int64, device="cuda")
    q = starts0.numel()
    total = int(lens.sum())
    d_starts = (starts0 + 1).contiguous()
    offs = torch.zeros(q + 1, dtype=torch.int64, device="cuda")
    out = torch.zeros(total, dtype=torch.uint8, device="cuda")
    cap = C.c_uint64()
    ts = []
    for i in range(reps + 1):
        torch.cuda.synchronize()
        cap.value = total
        t0 = time.perf_counter()
        rc = lib.tc_fm_extract_dev(ctx.handle, fm._h, C.c_void_p(d_starts.data_ptr()), C.c_void_p(lens.data_ptr()), q,
                                   C.c_void_p(offs.data_ptr()), C.c_void_p(out.data_ptr()), C.byref(cap))
        dt = time.perf_counter() - t0
        assert rc == 0 and cap.value == total, (rc, cap.value)
        if i:
            ts.append(dt * 1e3)
    ms = statistics.median(ts)
    # the answer against the text
    if whole:
        ok = bool(torch.equal(out, d_text))
    else:
        pos = (starts0[:, None] + torch.arange(qlen, device="cuda")[None, :]).reshape(-1)
        ok = bool(torch.equal(out, d_text[pos]))
    reads, steps = steps_of(starts0, lens, rate, n)
    res.update({"queries": q, "bytes": total, "extract_ms": round(ms, 3), "min_ms": round(min(ts), 3), "GB_per_s": round(total / ms / 1e6, 3),
                "L_reads": reads, "lf_steps": steps, "ns_per_step": round(ms * 1e6 / steps, 5), "ns_per_byte": round(ms * 1e6 / total, 5),
                "equal_to_text": ok})
    fm.close()
    print(json.dumps(res), flush=True)
    if not ok:
        sys.exit("the extracted bytes differ from the text")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rate", type=int)
    ap.add_argument("--log2", type=int, default=28)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--whole", action="store_true")
    ap.add_argument("--queries", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=100)
    ap.add_argument("--rates", type=int, nargs="*", default=[16, 32, 64])
    a = ap.parse_args()
    if a.rate is not None:
        one(a.rate, a.log2, a.reps, a.whole, a.queries, a.len)
        return
    rows = []
    for k, whole in [(k, False) for k in a.rates] + [(32, True)]:
        cmd = [sys.executable, os.path.abspath(__file__), "--rate", str(k), "--log2", str(a.log2), "--reps", str(a.reps),
               "--queries", str(a.queries), "--len", str(a.len)] + (["--whole"] if whole else [])
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-3000:])
            sys.exit("rate %d failed (exit %d): nothing more is started" % (k, p.returncode))
        rows.append(json.loads(p.stdout.strip().splitlines()[-1]))
    print("# text rate | mode   | extract part B/text B | queries |     bytes | ms (min) | GB/s | LF steps | ns/step | ns/byte")
    for r in rows:
        print("# %9d | %-6s | %6.4f | %7d | %9d | %8.3f (%8.3f) | %6.3f | %10d | %7.5f | %7.5f" % (
            r["text_rate"], r["mode"], r["extract_bytes_per_text_byte"], r["queries"], r["bytes"], r["extract_ms"], r["min_ms"], r["GB_per_s"],
            r["lf_steps"], r["ns_per_step"], r["ns_per_byte"]))
    print("# every run's bytes equal the text")


if __name__ == "__main__":
    main()
