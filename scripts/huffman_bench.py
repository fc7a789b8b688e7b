#!/usr/bin/env python3
"""Container size and time, packed against Huffman coding (tc_ctx_set_container_coding), per input class.

  python scripts/huffman_bench.py                       # iid ACGTN at 2^30 and the classes at 2^28, one child process each
  python scripts/huffman_bench.py --cls acgtn --log2 28 # one record, in this process
  python scripts/huffman_bench.py --cls acgtn --lib A.so --lib B.so   # packed coding of two builds, alternating (A/A first
                                                                      # shows the spread, then A/B)

Every record is measured in a child process of its own under a time limit; the first failure ends the run (nothing
more is started on a device that has just failed).  Times are HIP events on the context's stream (tc_ctx_stream), best
of 5 after a warm-up; sizes are container bytes per input byte."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "text-compression_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

KINDS = {"acgtn": 0, "ascii96": 1, "genome_like": 2, "zipf_words": 3, "runs": 4, "periodic": 5, "gaps": 6}


def one(cls, log2, reps):
    import numpy as np
    import torch
    import textcomp
    from textcomp import Block, _lib
    if os.environ.get("TEXTCOMP_LIB"):      # another build may lack the newest entry points: bind what it has
        _lib._prefer_process_hip_runtime()
        probe = C.CDLL(_lib.LIB_PATH)
        _lib.SYMBOLS = [s for s in _lib.SYMBOLS if hasattr(probe, s[0])]
    n = 1 << log2
    ctx = textcomp.Context(0)
    lib = ctx.lib
    d_text = torch.empty(n, dtype=torch.uint8, device="cuda")
    if cls == "bytes256":
        import classgen
        d_text.copy_(torch.from_numpy(classgen.bytes256(n)))
    else:
        assert lib.tc_generate_dev(ctx.handle, KINDS[cls], 0xC2, n, C.c_void_p(d_text.data_ptr())) == 0
    cap = int(lib.tc_container_bound(n + 2, 257))
    buf = torch.empty(cap, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.ExternalStream(lib.tc_ctx_stream(ctx.handle))
    torch.cuda.synchronize()
    res = {"cls": cls, "n": n, "lib": os.environ.get("TEXTCOMP_LIB", "in-tree")}
    codings = ("packed", "huffman") if hasattr(lib, "tc_ctx_set_container_coding") else ("packed",)

    def timed(fn):
        best = None
        for i in range(reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            b.synchronize()
            if i:
                best = a.elapsed_time(b) if best is None else min(best, a.elapsed_time(b))
        return best
    for coding in codings:
        if len(codings) > 1:
            ctx.set_container_coding(coding)
        used = [0]

        def enc():
            used[0] = ctx.encode_container_dev(d_text.data_ptr(), n, buf.data_ptr(), cap)
        ms_enc = timed(enc)
        st = ctx.stats()
        hdr = buf[:64].cpu().numpy().tobytes()
        nruns = int(np.frombuffer(hdr, "<u8", 1, 24)[0])
        o_c = torch.empty(nruns + 1, dtype=torch.int32, device="cuda")
        o_v = torch.empty(nruns + 1, dtype=torch.int16, device="cuda")
        blk = Block()

        def dec():
            blk.nruns, blk.run_count, blk.run_value = nruns, o_c.data_ptr(), o_v.data_ptr()
            assert lib.tc_container_to_block_dev(ctx.handle, C.c_void_p(buf.data_ptr()), used[0], C.byref(blk)) == 0
        ms_dec = timed(dec)
        back = torch.empty(n, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert lib.tc_decode_dev(ctx.handle, C.byref(blk), C.c_void_p(back.data_ptr())) == 0
        assert torch.equal(back, d_text), "round trip"
        del back, o_c, o_v
        res[coding] = {"bytes": used[0], "bytes_per_byte": round(used[0] / n, 4), "format": int(np.frombuffer(hdr, "<u4", 1, 60)[0]),
                       "runs": nruns, "encode_container_ms": round(ms_enc, 3), "container_to_block_ms": round(ms_dec, 3),
                       "ms_mtf_plus_rle": round(st.ms_mtf + st.ms_rle, 3), "ms_sa": round(st.ms_sa, 3)}
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cls")
    ap.add_argument("--log2", type=int, default=28)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lib", action="append", default=[])
    ap.add_argument("--limit", type=int, default=280, help="seconds per child process")
    a = ap.parse_args()
    if a.cls and not a.lib:
        return one(a.cls, a.log2, a.reps)
    if a.lib:     # packed coding of two builds: A, A, B, A, B
        jobs = [(a.cls or "acgtn", a.log2, lib) for lib in (a.lib[0], a.lib[0], a.lib[1], a.lib[0], a.lib[1])]
    else:
        jobs = [("acgtn", 30, None)] + [(c, 28, None) for c in ("ascii96", "bytes256", "zipf_words", "genome_like", "runs", "gaps")]
    for cls, log2, lib in jobs:
        env = dict(os.environ)
        if lib:
            env["TEXTCOMP_LIB"] = os.path.abspath(lib)
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--cls", cls, "--log2", str(log2),
               "--reps", str(a.reps)]
        rc = subprocess.call(cmd, env=env)
        if rc != 0:
            print("stopped: %s at 2^%d ended with status %d" % (cls, log2, rc), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
