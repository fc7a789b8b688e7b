"""CPU-only: register / scratch budgets of the mismatch-search kernel, read from hipcc's resource-usage remarks (a
cross-compile, no GPU), in the manner of tests/test_fm_extract_budgets.py.  fm_mm_kernel is a chain of dependent random
64-byte line reads per lane, like the count kernel and the walks: what hides their latency is the number of waves a SIMD
holds, so every instance must stay at 8 waves per SIMD (at most 64 VGPRs; its frames in LDS must leave room for 8
workgroups of 4 waves per CU) and must not spill.  The kernels it stands beside keep the budgets they had."""
import kernel_resources

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
    seen = {}
    for name, vso in kernel_resources.resources().items():
        for frag in BUDGETS:
            if frag in name:
                seen[frag] = vso
    for frag, (mv, ms, mo) in BUDGETS.items():
        assert frag in seen, "kernel not found: " + frag
        v, s, o = seen[frag]
        assert v <= mv and s <= ms and o >= mo, (frag, "VGPRs %d (<= %d), scratch %d (<= %d), waves/SIMD %d (>= %d)" % (v, mv, s, ms, o, mo))
