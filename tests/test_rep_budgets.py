"""CPU-only: register / scratch budgets of the repeats kernels (csrc/tc_rep.hpp), read from hipcc's resource-usage remarks (a
cross-compile, no GPU), in the manner of tests/test_lz_budgets.py.  rep_row_kernel is a chain of dependent random reads per
lane -- up to three row searches over the min tree -- like fm_ms_kernel and lz_lpf_kernel: what hides their latency is the
number of waves a SIMD holds, so both its kinds must stay at 8 waves per SIMD (at most 64 VGPRs) and must not spill; the
256-bit set of left bytes of the supermaximal kind is four registers, not an indexed array.  No other rep_* kernel may spill,
and the kernels whose header tc_rep.hpp uses keep the budgets their own tests give them."""
import re

import kernel_resources

# mangled-name fragment -> (max VGPRs, max scratch bytes per lane, min waves per SIMD)
BUDGETS = {
    "14rep_row_kernelILb0EE": (64, 0, 8),
    "14rep_row_kernelILb1EE": (64, 0, 8),
    "fm_ms_kernelILb0EE": (64, 0, 8),           # untouched: the budgets their own tests give them
    "fm_ms_kernelILb1EE": (64, 0, 8),
    "fm_count_kernelILb0EE": (64, 0, 8),
    "fm_count_kernelILb1EE": (64, 0, 8),
    "13lz_lpf_kernel": (64, 0, 8),
}
REP_KERNELS = ("14rep_row_kernelILb0EE", "14rep_row_kernelILb1EE", "15rep_left_kernel", "16rep_count_kernel", "15rep_fill_kernel")


def test_rep_kernel_budgets():
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


def test_no_rep_kernel_spills():
    res = kernel_resources.resources()
    rep = {name: vso for name, vso in res.items() if re.search(r"\d+rep_[a-z_]+kernel", name)}
    for frag in REP_KERNELS:                        # every kernel of tc_rep.hpp is in the listing ...
        assert any(frag in name for name in rep), "kernel not found: " + frag
    assert len(rep) == len(REP_KERNELS), sorted(rep)    # ... and the listing holds no rep_* kernel this test does not name
    for name, (_, scratch, _) in rep.items():
        assert scratch == 0, (name, "scratch %d" % scratch)
