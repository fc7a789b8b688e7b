"""CPU-only: register / scratch budgets of the extract kernels, read from hipcc's resource-usage remarks (a cross-compile,
no GPU), in the manner of tests/test_fm_sampled_budgets.py.  The extract walk is, like the locate walk, a chain of
dependent random reads per lane (the last-column byte, then one 64-byte rank line): what hides their latency is the
number of waves a SIMD holds, so the kernel must stay at 8 waves per SIMD (at most 64 VGPRs) and must not spill."""
import kernel_resources

# mangled-name fragment -> (max VGPRs, max scratch bytes per lane, min waves per SIMD)
BUDGETS = {
    "22fm_extract_walk_kernel": (64, 0, 8),
    "22fm_extract_plan_kernel": (32, 0, 8),
    "13fm_isa_kernel": (32, 0, 8),
    "17fm_isa_max_kernel": (32, 0, 8),
    "21fm_locate_walk_kernel": (64, 0, 8),      # untouched by extract: the budgets tests/test_fm_sampled_budgets.py gives them
    "fm_count_kernelILb1EE": (64, 0, 8),
}


def test_extract_kernel_budgets():
    seen = {}
    for name, vso in kernel_resources.resources().items():
        for frag in BUDGETS:
            if frag in name:
                seen[frag] = vso
    for frag, (mv, ms, mo) in BUDGETS.items():
        assert frag in seen, "kernel not found: " + frag
        v, s, o = seen[frag]
        assert v <= mv and s <= ms and o >= mo, (frag, "VGPRs %d (<= %d), scratch %d (<= %d), waves/SIMD %d (>= %d)" % (v, mv, s, ms, o, mo))
