"""CPU-only: register / scratch budgets of the palindrome kernels (csrc/tc_pal.hpp), read from hipcc's resource-usage remarks
(a cross-compile, no GPU), in the manner of tests/test_tr_budgets.py.  pal_centre_kernel is a chain of dependent random reads per
lane -- up to 17 extensions, each a few bytes compared and then a range minimum over a min tree -- like tr_cand_kernel,
fm_ms_kernel, lz_lpf_kernel, rep_row_kernel and tm_row_kernel: what hides their latency is the number of waves a SIMD holds, so it
must stay at 8 waves per SIMD (at most 64 VGPRs) and must not spill.  No other pal_* kernel may spill, and the kernels whose
headers tc_pal.hpp uses -- it takes an instance of lz_range_min of its own so that they compile as they were -- keep the budgets
their own tests give them."""
import re

import kernel_resources

# mangled-name fragment -> (max VGPRs, max scratch bytes per lane, min waves per SIMD)
BUDGETS = {
    "17pal_centre_kernel": (64, 0, 8),
    "14tr_cand_kernel": (64, 0, 8),             # untouched: the budgets their own tests give them
    "fm_ms_kernelILb0EE": (64, 0, 8),
    "fm_ms_kernelILb1EE": (64, 0, 8),
    "13lz_lpf_kernel": (64, 0, 8),
    "14rep_row_kernelILb0EE": (64, 0, 8),
    "14rep_row_kernelILb1EE": (64, 0, 8),
    "13tm_row_kernelILb0EE": (64, 0, 8),
    "13tm_row_kernelILb1EE": (64, 0, 8),
}
PAL_KERNELS = ("17pal_centre_kernel", "16pal_joint_kernel", "16pal_count_kernel", "15pal_fill_kernel", "18pal_longest_kernel")


def test_pal_kernel_budgets():
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


def test_no_pal_kernel_spills():
    res = kernel_resources.resources()
    pal = {name: vso for name, vso in res.items() if re.search(r"\d+pal_[a-z_]+kernel", name)}
    for frag in PAL_KERNELS:                        # every kernel of tc_pal.hpp is in the listing ...
        assert any(frag in name for name in pal), "kernel not found: " + frag
    assert len(pal) == len(PAL_KERNELS), sorted(pal)    # ... and the listing holds no pal_* kernel this test does not name
    for name, (_, scratch, _) in pal.items():
        assert scratch == 0, (name, "scratch %d" % scratch)
