"""CPU-only: register / scratch budgets of the LCP kernels, read from hipcc's resource-usage remarks (a cross-compile,
no GPU), in the manner of tests/test_fm_factorize_budgets.py.  lcp_irreducible_kernel is a latency-bound chain of
random reads per lane (phi[i], then two places of the text), like fm_count_kernel: what hides the latency is the number
of waves a SIMD holds, so it gets the same budget -- at most 64 VGPRs, 8 waves per SIMD.  The other new kernels stream
or gather and are held to the same occupancy (DESIGN 4.5 states it); no new kernel may spill."""
import kernel_resources

# mangled-name fragment -> (max VGPRs, max scratch bytes per lane, min waves per SIMD)
BUDGETS = {
    "22lcp_irreducible_kernel": (64, 0, 8),
    "14lcp_phi_kernel": (64, 0, 8),
    "15lcp_long_kernel": (64, 0, 8),
    "22lcp_scan_reduce_kernel": (64, 0, 8),
    "21lcp_scan_tiles_kernel": (64, 0, 8),
    "21lcp_scan_apply_kernel": (64, 0, 8),
    "17lcp_gather_kernel": (64, 0, 8),
    "18lcp_summary_kernel": (64, 0, 8),
}
NO_SPILL = ()


def test_lcp_kernel_budgets():
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
