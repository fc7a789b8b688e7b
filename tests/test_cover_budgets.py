"""CPU-only: register / scratch budgets of the repeat-cover kernels (csrc/tc_cov.hpp), read from hipcc's resource-usage remarks (a
cross-compile, no GPU), in the manner of tests/test_sus_budgets.py.  cov_seed_kernel is a chain of dependent random reads per lane
-- two row searches and, for LATER, a range minimum over the min trees -- like rep_row_kernel: what hides their latency is the number
of waves a SIMD holds, so both instances must stay at 8 waves per SIMD (at most 64 VGPRs) and must not spill.  No other cov_* kernel
may spill, and the older row kernels, whose headers tc_cov.hpp uses unchanged, keep the budgets tests/test_sus_budgets.py lists."""
import re

import kernel_resources
import test_sus_budgets

# mangled-name fragment -> (max VGPRs, max scratch bytes per lane, min waves per SIMD)
BUDGETS = {
    "15cov_seed_kernelILb0EE": (64, 0, 8),
    "15cov_seed_kernelILb1EE": (64, 0, 8),
}
BUDGETS.update(test_sus_budgets.BUDGETS)            # untouched: the budgets their own tests give them
COV_KERNELS = ("15cov_seed_kernelILb0EE", "15cov_seed_kernelILb1EE", "17cov_reduce_kernel", "16cov_spine_kernel", "16cov_count_kernel",
               "15cov_fill_kernel", "14cov_len_kernel", "15cov_mask_kernel", "16cov_dedup_kernel")


def test_cov_kernel_budgets():
    res = kernel_resources.resources()
    seen = {}
    for name, vso in res.items():
        for frag in BUDGETS:
            if frag in name:
                seen[frag] = vso
    assert len(BUDGETS) == len(test_sus_budgets.BUDGETS) + 2
    for frag, (mv, ms, mo) in BUDGETS.items():
        assert frag in seen, "kernel not found: " + frag
        v, s, o = seen[frag]
        assert v <= mv and s <= ms and o >= mo, (frag, "VGPRs %d (<= %d), scratch %d (<= %d), waves/SIMD %d (>= %d)" % (v, mv, s, ms, o, mo))


def test_no_cov_kernel_spills():
    res = kernel_resources.resources()
    cov = {name: vso for name, vso in res.items() if re.search(r"\d+cov_[a-z_]+kernel", name)}
    for frag in COV_KERNELS:                        # every kernel of tc_cov.hpp is in the listing ...
        assert any(frag in name for name in cov), "kernel not found: " + frag
    assert len(cov) == len(COV_KERNELS), sorted(cov)    # ... and the listing holds no cov_* kernel this test does not name
    for name, (_, scratch, _) in cov.items():
        assert scratch == 0, (name, "scratch %d" % scratch)
