"""CPU-only: register / scratch budgets of the mismatch-search kernel, read from hipcc's resource-usage remarks (a
cross-compile, no GPU), in the manner of tests/test_fm_extract_budgets.py.  fm_mm_kernel is a chain of dependent random
64-byte line reads per lane, like the count kernel and the walks: what hides their latency is the number of waves a SIMD
holds, so every instance must stay at 8 waves per SIMD (at most 64 VGPRs; its frames in LDS must leave room for 8
workgroups of 4 waves per CU) and must not spill.  The kernels it stands beside keep the budgets they had."""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "text-compression_amd")

# mangled-name fragment -> (max VGPRs, max scratch bytes per lane, min waves per SIMD)
BUDGETS = {
    "fm_mm_kernelILb0ELb0EE": (64, 0, 8),
    "fm_mm_kernelILb0ELb1EE": (64, 0, 8),
    "fm_mm_kernelILb1ELb0EE": (64, 0, 8),
    "fm_mm_kernelILb1ELb1EE": (64, 0, 8),
    "fm_count_kernelILb0EE": (64, 0, 8),        # untouched: the budgets the existing budget tests give them
    "fm_count_kernelILb1EE": (64, 0, 8),
    "21fm_locate_walk_kernel": (64, 0, 8),
    "22fm_extract_walk_kernel": (64, 0, 8),
}


def test_mismatch_kernel_budgets():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as d:
        out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-pthread",
                              "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "csrc"),
                              "-Rpass-analysis=kernel-resource-usage", "-o", os.path.join(d, "libtextcomp_budget.so"),
                              os.path.join(PKG, "csrc", "textcomp.hip")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    seen = {}
    for blk in out.stderr.split("Function Name: ")[1:]:
        name = blk.split()[0]
        v = int(re.search(r"VGPRs: (\d+)", blk).group(1))
        s = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blk).group(1))
        o = int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", blk).group(1))
        for frag in BUDGETS:
            if frag in name:
                seen[frag] = (v, s, o)
    for frag, (mv, ms, mo) in BUDGETS.items():
        assert frag in seen, "kernel not found: " + frag
        v, s, o = seen[frag]
        assert v <= mv and s <= ms and o >= mo, (frag, "VGPRs %d (<= %d), scratch %d (<= %d), waves/SIMD %d (>= %d)" % (v, mv, s, ms, o, mo))
