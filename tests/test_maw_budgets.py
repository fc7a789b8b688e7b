"""CPU-only: register / scratch budgets of the minimal-absent-word kernels (csrc/tc_maw.hpp), read from hipcc's resource-usage
remarks (a cross-compile, no GPU), in the manner of tests/test_pal_budgets.py.  maw_row_kernel is a chain of dependent random
reads per lane -- up to four searches over the min tree and three range ORs over the OR tree -- like rep_row_kernel and
pal_centre_kernel: what hides their latency is the number of waves a SIMD holds, so every instance (two set widths, each as the
count, the fill and the histogram pass) must stay at 8 waves per SIMD (at most 64 VGPRs) and must not spill.  No other maw_*
kernel may spill, and the older row kernels, whose headers tc_maw.hpp uses unchanged, keep the budgets their own tests give them."""
import re

import kernel_resources

# mangled-name fragment -> (max VGPRs, max scratch bytes per lane, min waves per SIMD)
BUDGETS = {
    "14maw_row_kernelILb0ELi0EE": (64, 0, 8),   # one u64 per set: count, fill, histogram
    "14maw_row_kernelILb0ELi1EE": (64, 0, 8),
    "14maw_row_kernelILb0ELi2EE": (64, 0, 8),
    "14maw_row_kernelILb1ELi0EE": (64, 0, 8),   # four u64 per set
    "14maw_row_kernelILb1ELi1EE": (64, 0, 8),
    "14maw_row_kernelILb1ELi2EE": (64, 0, 8),
    "17pal_centre_kernel": (64, 0, 8),          # untouched: the budgets their own tests give them
    "14tr_cand_kernel": (64, 0, 8),
    "fm_ms_kernelILb0EE": (64, 0, 8),
    "fm_ms_kernelILb1EE": (64, 0, 8),
    "13lz_lpf_kernel": (64, 0, 8),
    "14rep_row_kernelILb0EE": (64, 0, 8),
    "14rep_row_kernelILb1EE": (64, 0, 8),
    "13tm_row_kernelILb0EE": (64, 0, 8),
    "13tm_row_kernelILb1EE": (64, 0, 8),
}
MAW_KERNELS = tuple(f for f in BUDGETS if "maw_" in f) + ("15maw_tree_kernelILb0EE", "15maw_tree_kernelILb1EE")


def test_maw_kernel_budgets():
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


def test_no_maw_kernel_spills():
    res = kernel_resources.resources()
    maw = {name: vso for name, vso in res.items() if re.search(r"\d+maw_[a-z_]+kernel", name)}
    for frag in MAW_KERNELS:                        # every kernel of tc_maw.hpp is in the listing ...
        assert any(frag in name for name in maw), "kernel not found: " + frag
    assert len(maw) == len(MAW_KERNELS), sorted(maw)    # ... and the listing holds no maw_* kernel this test does not name
    for name, (_, scratch, _) in maw.items():
        assert scratch == 0, (name, "scratch %d" % scratch)
