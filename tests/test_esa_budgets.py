"""CPU-only: register / scratch budgets of the query kernels of the kept enhanced suffix array (csrc/tc_esa.hpp), read from hipcc's
resource-usage remarks (a cross-compile, no GPU), in the manner of tests/test_cover_budgets.py.  Each of the three kernels is a chain
of dependent random reads per lane -- two reads of isa and a range minimum, or two row searches and a range minimum -- so what hides
their latency is the number of waves a SIMD holds: all three must stay at 8 waves per SIMD (at most 64 VGPRs) and must not spill.
The older row kernels, whose headers tc_esa.hpp uses unchanged, keep the budgets tests/test_cover_budgets.py lists."""
import re

import kernel_resources
import test_cover_budgets

# mangled-name fragment -> (max VGPRs, max scratch bytes per lane, min waves per SIMD)
ESA_BUDGETS = {
    "14esa_lce_kernel": (64, 0, 8),
    "15esa_find_kernel": (64, 0, 8),
    "18esa_compare_kernel": (64, 0, 8),
}
# the older kernels' budgets, as their own tests state them: re-asserted here, entry by entry, so that a change of that dict shows
OLDER = {
    "15cov_seed_kernelILb0EE": (64, 0, 8),
    "15cov_seed_kernelILb1EE": (64, 0, 8),
}


def _check(budgets):
    res = kernel_resources.resources()
    for frag, (mv, ms, mo) in budgets.items():
        hits = [vso for name, vso in res.items() if frag in name]
        assert hits, "kernel not found: " + frag
        for v, s, o in hits:
            assert v <= mv and s <= ms and o >= mo, (frag, "VGPRs %d (<= %d), scratch %d (<= %d), waves/SIMD %d (>= %d)" % (v, mv, s, ms, o, mo))


def test_esa_kernel_budgets():
    _check(ESA_BUDGETS)


def test_no_esa_kernel_spills():
    res = kernel_resources.resources()
    esa = {name: vso for name, vso in res.items() if re.search(r"\d+esa_[a-z_]+kernel", name)}
    for frag in ESA_BUDGETS:                        # every kernel of tc_esa.hpp is in the listing ...
        assert any(frag in name for name in esa), "kernel not found: " + frag
    assert len(esa) == len(ESA_BUDGETS), sorted(esa)    # ... and the listing holds no esa_* kernel this test does not name
    for name, (_, scratch, _) in esa.items():
        assert scratch == 0, (name, "scratch %d" % scratch)


def test_older_budgets_are_unchanged_and_still_met():
    for frag, b in OLDER.items():
        assert test_cover_budgets.BUDGETS[frag] == b
    assert not any("esa_" in frag for frag in test_cover_budgets.BUDGETS)
    _check(test_cover_budgets.BUDGETS)
