"""CPU-only: register / scratch budgets of the tandem-repeat kernels (csrc/tc_tr.hpp), read from hipcc's resource-usage remarks
(a cross-compile, no GPU), in the manner of tests/test_rep_budgets.py.  tr_cand_kernel is a chain of dependent random reads
per lane -- two row searches over a min tree and up to four range minima -- like fm_ms_kernel, lz_lpf_kernel and
rep_row_kernel: what hides their latency is the number of waves a SIMD holds, so it must stay at 8 waves per SIMD (at most
64 VGPRs) and must not spill.  No other tr_* kernel may spill, and the kernels whose headers tc_tr.hpp uses -- it takes an
instance of lz_range_min of its own so that they compile as they were -- keep the budgets their own tests give them."""
import re

import kernel_resources

# mangled-name fragment -> (max VGPRs, max scratch bytes per lane, min waves per SIMD)
BUDGETS = {
    "14tr_cand_kernel": (64, 0, 8),
    "fm_ms_kernelILb0EE": (64, 0, 8),           # untouched: the budgets their own tests give them
    "fm_ms_kernelILb1EE": (64, 0, 8),
    "13lz_lpf_kernel": (64, 0, 8),
    "14rep_row_kernelILb0EE": (64, 0, 8),
    "14rep_row_kernelILb1EE": (64, 0, 8),
    "13tm_row_kernelILb0EE": (64, 0, 8),
    "13tm_row_kernelILb1EE": (64, 0, 8),
}
TR_KERNELS = ("14tr_cand_kernel", "17tr_reverse_kernel", "13tr_isa_kernel", "14tr_comp_kernel","15tr_count_kernel", "14tr_fill_kernel", "15tr_order_kernel")


def test_tr_kernel_budgets():
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


def test_no_tr_kernel_spills():
    res = kernel_resources.resources()
    tr = {name: vso for name, vso in res.items() if re.search(r"\d+tr_[a-z_]+kernel", name)}
    for frag in TR_KERNELS:                         # every kernel of tc_tr.hpp is in the listing ...
        assert any(frag in name for name in tr), "kernel not found: " + frag
    assert len(tr) == len(TR_KERNELS), sorted(tr)       # ... and the listing holds no tr_* kernel this test does not name
    for name, (_, scratch, _) in tr.items():
        assert scratch == 0, (name, "scratch %d" % scratch)
