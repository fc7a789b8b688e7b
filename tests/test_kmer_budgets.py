"""CPU-only: register / scratch budgets of the k-mer kernels (csrc/tc_kmer.hpp), read from hipcc's resource-usage remarks (a
cross-compile, no GPU), in the manner of tests/test_rep_budgets.py.  The passes are streaming: every km_* kernel is in the
listing and none spills; km_pass_kernel (all three modes: the spectrum's 16 KB of LDS counters included) and
km_profile_kernel (its two histograms are 33 KB: 512 lanes per workgroup make four workgroups fill a CU) keep at least 8
waves per SIMD.  The kernels of the other ESA consumers keep the budgets their own tests give them."""
import re

import kernel_resources

# mangled-name fragment -> (max VGPRs, max scratch bytes per lane, min waves per SIMD)
BUDGETS = {
    "14km_pass_kernelILi0EE": (64, 0, 8),
    "14km_pass_kernelILi1EE": (64, 0, 8),
    "14km_pass_kernelILi2EE": (64, 0, 8),
    "17km_profile_kernel": (64, 0, 8),
    "14rep_row_kernelILb0EE": (64, 0, 8),       # untouched: the budgets their own tests give them
    "14rep_row_kernelILb1EE": (64, 0, 8),
    "13lz_lpf_kernel": (64, 0, 8),
    "fm_ms_kernelILb0EE": (64, 0, 8),
    "fm_ms_kernelILb1EE": (64, 0, 8),
    "fm_count_kernelILb0EE": (64, 0, 8),
    "fm_count_kernelILb1EE": (64, 0, 8),
}
KM_KERNELS = ("14km_pass_kernelILi0EE", "14km_pass_kernelILi1EE", "14km_pass_kernelILi2EE", "14km_tile_kernel", "15km_carry_kernel",
              "17km_profile_kernel")
PROFILE_LDS_MAX = 33 * 1024


def test_km_kernel_budgets():
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


def test_no_km_kernel_spills():
    res = kernel_resources.resources()
    km = {name: vso for name, vso in res.items() if re.search(r"\d+km_[a-z_]+kernel", name)}
    for frag in KM_KERNELS:                         # every kernel of tc_kmer.hpp is in the listing ...
        assert any(frag in name for name in km), "kernel not found: " + frag
    assert len(km) == len(KM_KERNELS), sorted(km)   # ... and the listing holds no km_* kernel this test does not name
    for name, (_, scratch, _) in km.items():
        assert scratch == 0, (name, "scratch %d" % scratch)


def test_profile_histograms_fit_their_lds():
    lds = [r["lds"] for name, r in kernel_resources.remarks().items() if "17km_profile_kernel" in name]
    assert len(lds) == 1 and lds[0] <= PROFILE_LDS_MAX, lds
