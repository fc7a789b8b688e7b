"""CPU-only: register / scratch budgets of the unique-substring kernels (csrc/tc_sus.hpp), read from hipcc's resource-usage
remarks (a cross-compile, no GPU), in the manner of tests/test_maw_budgets.py.  sus_point_kernel is a chain of dependent random
reads per lane -- two scan entries, a range minimum and a search over the min tree -- like rep_row_kernel: what hides their latency
is the number of waves a SIMD holds, so it must stay at 8 waves per SIMD (at most 64 VGPRs) and must not spill.  No other sus_*
kernel may spill, and the older row kernels, whose headers tc_sus.hpp uses unchanged, keep the budgets their own tests give them."""
import re

import kernel_resources

# mangled-name fragment -> (max VGPRs, max scratch bytes per lane, min waves per SIMD)
BUDGETS = {
    "16sus_point_kernel": (64, 0, 8),
    "14maw_row_kernelILb0ELi0EE": (64, 0, 8),   # untouched: the budgets their own tests give them
    "14maw_row_kernelILb0ELi1EE": (64, 0, 8),
    "14maw_row_kernelILb0ELi2EE": (64, 0, 8),
    "14maw_row_kernelILb1ELi0EE": (64, 0, 8),
    "14maw_row_kernelILb1ELi1EE": (64, 0, 8),
    "14maw_row_kernelILb1ELi2EE": (64, 0, 8),
    "17pal_centre_kernel": (64, 0, 8),
    "14tr_cand_kernel": (64, 0, 8),
    "fm_ms_kernelILb0EE": (64, 0, 8),
    "fm_ms_kernelILb1EE": (64, 0, 8),
    "13lz_lpf_kernel": (64, 0, 8),
    "14rep_row_kernelILb0EE": (64, 0, 8),
    "14rep_row_kernelILb1EE": (64, 0, 8),
    "13tm_row_kernelILb0EE": (64, 0, 8),
    "13tm_row_kernelILb1EE": (64, 0, 8),
}
SUS_KERNELS = ("16sus_point_kernel", "17sus_prefix_kernel", "15sus_mark_kernelILi0EE", "15sus_mark_kernelILi1EE", "15sus_mark_kernelILi2EE",
               "17sus_reduce_kernel", "16sus_spine_kernel", "15sus_scan_kernel")


def test_sus_kernel_budgets():
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


def test_no_sus_kernel_spills():
    res = kernel_resources.resources()
    sus = {name: vso for name, vso in res.items() if re.search(r"\d+sus_[a-z_]+kernel", name)}
    for frag in SUS_KERNELS:                        # every kernel of tc_sus.hpp is in the listing ...
        assert any(frag in name for name in sus), "kernel not found: " + frag
    assert len(sus) == len(SUS_KERNELS), sorted(sus)    # ... and the listing holds no sus_* kernel this test does not name
    for name, (_, scratch, _) in sus.items():
        assert scratch == 0, (name, "scratch %d" % scratch)
