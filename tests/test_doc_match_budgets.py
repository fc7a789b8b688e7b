"""CPU-only: register / scratch budgets of the kernels of the cross-document matches on the kept enhanced suffix array
(csrc/tc_esa_xdoc.hpp), read from hipcc's resource-usage remarks (a cross-compile, no GPU), in the manner of
tests/test_esa_docs_budgets.py.  Both instances of esx_match_kernel are chains of dependent random reads per lane -- the neighbours
(for EARLIER two searches over the tree of da), then two range minima over the tree of lcp -- so, like every kernel over these trees,
they must stay at 8 waves per SIMD (at most 64 VGPRs) and must not spill; the scans and the per-document kernels are held to the same
budget.  The kernels of tc_esa_docs.hpp and tc_cov.hpp, which tc_esa_xdoc.hpp uses unchanged, keep the budgets their own tests list."""
import re

import kernel_resources
import test_cover_budgets
import test_esa_budgets
import test_esa_docs_budgets

ESX_KERNELS = ("16esx_match_kernelILi0EE", "16esx_match_kernelILi1EE", "17esx_reduce_kernel", "16esx_heads_kernel", "19esx_tile_sum_kernel",
               "21esx_doc_prefix_kernel", "19esx_doc_diff_kernel", "14esx_seg_kernelILi0EE", "14esx_seg_kernelILi1EE",
               "20esx_seg_spine_kernel")
# mangled-name fragment -> (max VGPRs, max scratch bytes per lane, min waves per SIMD)
ESX_BUDGETS = {frag: (64, 0, 8) for frag in ESX_KERNELS}


def test_every_esx_kernel_is_listed_and_no_other():
    res = kernel_resources.resources()
    esx = {name for name in res if re.search(r"\d+esx_[a-z_]+", name)}
    for frag in ESX_KERNELS:
        assert any(frag in name for name in esx), "kernel not found: " + frag
    assert len(esx) == len(ESX_KERNELS), sorted(esx)


def test_esx_kernel_budgets():
    test_esa_budgets._check(ESX_BUDGETS)


def test_older_budgets_are_still_met():
    test_esa_docs_budgets.test_doc_kernel_budgets()
    test_esa_docs_budgets.test_no_esd_kernel_spills()
    test_esa_docs_budgets.test_kmd_kernel_budgets()
    test_esa_docs_budgets.test_older_esa_budgets_are_unchanged_and_still_met()
    test_cover_budgets.test_cov_kernel_budgets()
    test_cover_budgets.test_no_cov_kernel_spills()
