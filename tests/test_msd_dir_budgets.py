"""CPU-only: the kernels of the aligned MSD level with the directory of live parents (csrc/tc_msd.hpp:
msd_partition_dir_kernel) against the budgets of the instances they stand beside -- msd_partition_kernel<false, false> and
msd_partition_kernel<false, true> (tests/test_kernel_budgets.py) -- and their asm-issued loads (the prefetch, and the next
parent's digit rows behind it) against the rule of scripts/check_asm_prefetch.py, in the default build and with
-DMSD_PROFILE."""
import importlib.util
import os

import pytest

import kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("check_asm_prefetch", os.path.join(ROOT, "scripts", "check_asm_prefetch.py"))
_mod = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_mod)

# mangled-name fragment -> (max VGPRs, max scratch bytes per lane, min waves per SIMD)
BUDGETS = {
    "msd_partition_dir_kernelILb0EE": (128, 0, 4),
    "msd_partition_dir_kernelILb1EE": (128, 0, 4),
}
LDS_BYTES = 160 * 1024


def test_dir_kernels_meet_their_neighbours_budgets():
    seen = {}
    for name, r in kernel_resources.remarks().items():
        for frag in BUDGETS:
            if frag in name:
                seen[frag] = r
    for frag, (mv, ms, mo) in BUDGETS.items():
        assert frag in seen, "kernel not found: " + frag
        r = seen[frag]
        assert r["vgprs"] <= mv and r["scratch"] <= ms and r["waves"] >= mo and r["lds"] <= LDS_BYTES, (frag, r)


def test_old_instances_are_still_built():
    """TC_MSD_DIR=0 runs them"""
    names = list(kernel_resources.resources())
    for frag in _mod.KERNELS:
        assert any(frag in n for n in names), frag


@pytest.mark.parametrize("defs", [[], ["-DMSD_PROFILE"]], ids=["default", "MSD_PROFILE"])
def test_dir_prefetch_destinations_are_untouched_until_they_land(defs):
    assert _mod.check(defs, kernels=list(BUDGETS)) >= len(BUDGETS)
