"""CPU-only: register / scratch budgets of the kernels of the document collections on the kept enhanced suffix array
(csrc/tc_esa_docs.hpp), read from hipcc's resource-usage remarks (a cross-compile, no GPU), in the manner of tests/test_esa_budgets.py.
Both instances of esd_doc_kernel are chains of dependent random reads per lane -- two row searches over the tree of lcp, then one search
over the tree of pv per document found -- so, like every kernel over these trees, they must stay at 8 waves per SIMD (at most 64 VGPRs)
and must not spill.  The tile kernels of the k-mer document frequency are held to the same budget.  The build's kernels stream and
must not spill.  The query kernels of tc_esa.hpp, whose headers
tc_esa_docs.hpp uses unchanged, keep the budgets tests/test_esa_budgets.py lists."""
import re

import kernel_resources
import test_esa_budgets

# mangled-name fragment -> (max VGPRs, max scratch bytes per lane, min waves per SIMD)
DOC_BUDGETS = {
    "14esd_doc_kernelILb0EE": (64, 0, 8),
    "14esd_doc_kernelILb1EE": (64, 0, 8),
}
BUILD_KERNELS = ("13esd_da_kernelILb0EE", "13esd_da_kernelILb1EE", "21esd_sort_count_kernelILb0EE", "21esd_sort_count_kernelILb1EE",
                 "23esd_sort_scatter_kernelILb0EE", "23esd_sort_scatter_kernelILb1EE", "13esd_pv_kernel")
# the tile kernels of the k-mer document frequency stream over lcp and pv, 16 rows a lane, as km_pass_kernel of tc_kmer.hpp does, and
# have its occupancy: at most 64 VGPRs, no scratch, 8 waves per SIMD (the fill instance stages one word per k-mer, 16 KB of LDS)
KMER_KERNELS = ("15kmd_flag_kernel", "15kmd_pass_kernelILi0EE", "15kmd_pass_kernelILi1EE", "15kmd_pass_kernelILi2EE")


def test_doc_kernel_budgets():
    test_esa_budgets._check(DOC_BUDGETS)


def test_no_esd_kernel_spills():
    res = kernel_resources.resources()
    esd = {name: vso for name, vso in res.items() if re.search(r"\d+esd_[a-z_]+kernel", name)}
    for frag in list(DOC_BUDGETS) + list(BUILD_KERNELS):    # every kernel of tc_esa_docs.hpp is in the listing ...
        assert any(frag in name for name in esd), "kernel not found: " + frag
    assert len(esd) == len(DOC_BUDGETS) + len(BUILD_KERNELS), sorted(esd)   # ... and the listing holds no esd_* kernel this test does not name
    for name, (_, scratch, _) in esd.items():
        assert scratch == 0, (name, "scratch %d" % scratch)


def test_kmd_kernel_budgets():
    res = kernel_resources.resources()
    kmd = {name: vso for name, vso in res.items() if re.search(r"\d+kmd_[a-z_]+kernel", name)}
    for frag in KMER_KERNELS:                               # every kmd_* kernel of tc_esa_docs.hpp is in the listing, and no other
        assert any(frag in name for name in kmd), "kernel not found: " + frag
    assert len(kmd) == len(KMER_KERNELS), sorted(kmd)
    test_esa_budgets._check({frag: (64, 0, 8) for frag in KMER_KERNELS})


def test_older_esa_budgets_are_unchanged_and_still_met():
    assert test_esa_budgets.ESA_BUDGETS == {"14esa_lce_kernel": (64, 0, 8), "15esa_find_kernel": (64, 0, 8), "18esa_compare_kernel": (64, 0, 8)}
    test_esa_budgets._check(test_esa_budgets.ESA_BUDGETS)
