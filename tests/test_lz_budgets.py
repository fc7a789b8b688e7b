"""CPU-only: register / scratch budgets of the LZ77 kernels (csrc/tc_lz.hpp), read from hipcc's resource-usage remarks (a
cross-compile, no GPU), in the manner of tests/test_fm_match_stats_budgets.py.  lz_lpf_kernel is a chain of dependent random
reads per lane -- two row searches and two range minima over the min trees -- like fm_ms_kernel: what hides their latency is
the number of waves a SIMD holds, so it must stay at 8 waves per SIMD (at most 64 VGPRs) and must not spill.  No other lz_*
kernel may spill, and the kernels whose header tc_lz.hpp includes keep the budgets their own tests give them."""
import re

import kernel_resources

# mangled-name fragment -> (max VGPRs, max scratch bytes per lane, min waves per SIMD)
BUDGETS = {
    "13lz_lpf_kernel": (64, 0, 8),
    "fm_ms_kernelILb0EE": (64, 0, 8),           # untouched: the budgets tests/test_fm_match_stats_budgets.py gives them
    "fm_ms_kernelILb1EE": (64, 0, 8),
    "fm_count_kernelILb0EE": (64, 0, 8),
    "fm_count_kernelILb1EE": (64, 0, 8),
}
LZ_KERNELS = ("13lz_lpf_kernel", "16lz_unpack_kernel", "14lz_tile_kernelILi0EE", "14lz_tile_kernelILi1EE", "14lz_tile_kernelILi2EE",
              "15lz_chain_kernel", "16lz_un_len_kernel", "18lz_un_check_kernel", "19lz_un_parent_kernel", "17lz_un_jump_kernel",
              "19lz_un_gather_kernel")


def test_lz_kernel_budgets():
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


def test_no_lz_kernel_spills():
    res = kernel_resources.resources()
    lz = {name: vso for name, vso in res.items() if re.search(r"\d+lz_[a-z_]+kernel", name)}
    for frag in LZ_KERNELS:                         # every kernel of tc_lz.hpp is in the listing ...
        assert any(frag in name for name in lz), "kernel not found: " + frag
    assert len(lz) == len(LZ_KERNELS), sorted(lz)   # ... and the listing holds no lz_* kernel this test does not name
    for name, (_, scratch, _) in lz.items():
        assert scratch == 0, (name, "scratch %d" % scratch)
