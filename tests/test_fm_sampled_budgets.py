"""CPU-only: register / scratch budgets of the sampled-locate kernels, read from hipcc's resource-usage remarks (a
cross-compile, no GPU), in the manner of tests/test_kernel_budgets.py.  The walk is a chain of dependent random 64-byte
reads per lane: what hides their latency is the number of waves a SIMD holds, so the kernel must stay at 8 waves per SIMD
(at most 64 VGPRs) and must not spill."""
import kernel_resources

# mangled-name fragment -> (max VGPRs, max scratch bytes per lane, min waves per SIMD)
BUDGETS = {
    "21fm_locate_walk_kernel": (64, 0, 8),
    "21fm_locate_rows_kernel": (32, 0, 8),
    "15fm_marks_kernel": (32, 0, 8),
    "17fm_samples_kernel": (32, 0, 8),
    "fm_count_kernelILb1EE": (64, 0, 8),      # untouched by the sampled index: the budget it has in test_kernel_budgets.py
}


def test_sampled_locate_kernel_budgets():
    seen = {}
    for name, vso in kernel_resources.resources().items():
        for frag in BUDGETS:
            if frag in name:
                seen[frag] = vso
    for frag, (mv, ms, mo) in BUDGETS.items():
        assert frag in seen, "kernel not found: " + frag
        v, s, o = seen[frag]
        assert v <= mv and s <= ms and o >= mo, (frag, "VGPRs %d (<= %d), scratch %d (<= %d), waves/SIMD %d (>= %d)" % (v, mv, s, ms, o, mo))
