"""CPU-only: register / scratch budgets of the matching-statistics kernels, read from hipcc's resource-usage remarks (a
cross-compile, no GPU), in the manner of tests/test_fm_factorize_budgets.py.  fm_ms_kernel is a chain of dependent random
64-byte line reads per lane, like the count kernel it extends: what hides their latency is the number of waves a SIMD
holds, so every instance must stay at 8 waves per SIMD (at most 64 VGPRs) and must not spill -- the two row searches of a
shrink included.  The small kernels (the tree levels, the MEM count and fill) must not spill, and the kernels they stand
beside keep the budgets they had."""
import kernel_resources

# mangled-name fragment -> (max VGPRs, max scratch bytes per lane, min waves per SIMD)
BUDGETS = {
    "fm_ms_kernelILb0EE": (64, 0, 8),
    "fm_ms_kernelILb1EE": (64, 0, 8),
    "fm_count_kernelILb0EE": (64, 0, 8),        # untouched: the budgets the existing budget tests give them
    "fm_count_kernelILb1EE": (64, 0, 8),
    "fm_mm_kernelILb0ELb0EE": (64, 0, 8),
    "fm_mm_kernelILb0ELb1EE": (64, 0, 8),
    "fm_mm_kernelILb1ELb0EE": (64, 0, 8),
    "fm_mm_kernelILb1ELb1EE": (64, 0, 8),
    "fm_factor_kernelILb0ELb0EE": (64, 0, 8),
    "fm_factor_kernelILb0ELb1EE": (64, 0, 8),
    "fm_factor_kernelILb1ELb0EE": (64, 0, 8),
    "fm_factor_kernelILb1ELb1EE": (64, 0, 8),
    "21fm_factor_walk_kernel": (64, 0, 8),      # the walk that turns the rows of ms_pos / mem_pos into positions
    "21fm_locate_walk_kernel": (64, 0, 8),
}
NO_SPILL = ("14fm_lmin_kernel", "19fm_mem_count_kernel", "18fm_mem_fill_kernel")


def test_match_stats_kernel_budgets():
    seen = {}
    for name, vso in kernel_resources.resources().items():
        for frag in tuple(BUDGETS) + NO_SPILL:
            if frag in name:
                seen[frag] = vso
    for frag, (mv, ms, mo) in BUDGETS.items():
        assert frag in seen, "kernel not found: " + frag
        v, s, o = seen[frag]
        assert v <= mv and s <= ms and o >= mo, (frag, "VGPRs %d (<= %d), scratch %d (<= %d), waves/SIMD %d (>= %d)" % (v, mv, s, ms, o, mo))
    for frag in NO_SPILL:
        assert frag in seen, "kernel not found: " + frag
        assert seen[frag][1] == 0, (frag, "scratch %d" % seen[frag][1])
