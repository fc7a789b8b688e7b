"""CPU-only: register / scratch budgets of the kernels of the two-text comparison (csrc/tc_tm.hpp), read from hipcc's
resource-usage remarks (a cross-compile, no GPU), in the manner of tests/test_kmer_budgets.py.  Both instances of
tm_row_kernel -- a lane per Q row: two range minima and, in the instance that also answers positions and counts, two row
searches -- stay within 64 VGPRs without scratch, so 8 waves per SIMD hide their dependent line reads; the flag,
compaction and MEM passes are streaming: every tm_* kernel is in the listing and none spills.  The kernels of the other ESA
consumers keep the budgets their own tests give them."""
import re

import kernel_resources

# mangled-name fragment -> (max VGPRs, max scratch bytes per lane, min waves per SIMD)
BUDGETS = {
    "13tm_row_kernelILb0EE": (64, 0, 8),
    "13tm_row_kernelILb1EE": (64, 0, 8),
    "13lz_lpf_kernel": (64, 0, 8),              # untouched: the budgets their own tests give them
    "14rep_row_kernelILb0EE": (64, 0, 8),
    "14rep_row_kernelILb1EE": (64, 0, 8),
    "fm_ms_kernelILb0EE": (64, 0, 8),
    "fm_ms_kernelILb1EE": (64, 0, 8),
}
TM_KERNELS = ("13tm_row_kernelILb0EE", "13tm_row_kernelILb1EE", "14tm_flag_kernel", "17tm_compact_kernel", "19tm_mem_count_kernel",
              "18tm_mem_fill_kernel")


def test_tm_kernel_budgets():
    res = kernel_resources.resources()
    seen = {}
    for name, vso in res.items():
        for frag in BUDGETS:
            if frag in name:
                seen[frag] = vso
    for frag, (mv, ms, mo) in BUDGETS.items():
        assert frag in seen, "kernel not found: " + frag
        v, s, o = seen[frag]
        assert v <= mv and s <= ms and o >= mo, (frag, "VGPRs %d (<= %d), scratch %d (<= %d), waves/SIMD %d (>= %d)" % (v, mv, s, ms, o, mo))


def test_no_tm_kernel_spills():
    res = kernel_resources.resources()
    tm = {name: vso for name, vso in res.items() if re.search(r"\d+tm_[a-z_]+kernel", name)}
    for frag in TM_KERNELS:                         # every kernel of tc_tm.hpp is in the listing ...
        assert any(frag in name for name in tm), "kernel not found: " + frag
    assert len(tm) == len(TM_KERNELS), sorted(tm)   # ... and the listing holds no tm_* kernel this test does not name
    for name, (_, scratch, _) in tm.items():
        assert scratch == 0, (name, "scratch %d" % scratch)
