"""CPU-only: the kernels of the split key layout (csrc/tc_msd.hpp: level 1 writes the keys as two arrays of 32-bit halves,
the joint count reads the high halves, level 2 reads both) against the budgets of the kernels they stand beside
(tests/test_kernel_budgets.py), and their asm-issued prefetch against the rule of scripts/check_asm_prefetch.py, in the
default build and with -DMSD_PROFILE (whose cycle stamps change the register allocation of the partition kernels)."""
import importlib.util
import os

import pytest

import kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("check_asm_prefetch", os.path.join(ROOT, "scripts", "check_asm_prefetch.py"))
_mod = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_mod)

# mangled-name fragment -> (max VGPRs, max scratch bytes per lane, min waves per SIMD): the figures of
# msd_partition_kernel<false, false>, msd_partition_kernel<true, false> and msd_count_kernel<false, true>
BUDGETS = {
    "msd_partition_split_kernelILb0EE": (128, 0, 4),
    "msd_partition_split_kernelILb1EE": (128, 16, 4),
    "msd_count_hi_kernel": (64, 0, 4),
}
SPLIT_PARTITION = ["msd_partition_split_kernelILb0EE", "msd_partition_split_kernelILb1EE"]


def test_split_kernels_meet_their_neighbours_budgets():
    seen = {}
    for name, vso in kernel_resources.resources().items():
        for frag in BUDGETS:
            if frag in name:
                seen[frag] = vso
    for frag, (mv, ms, mo) in BUDGETS.items():
        assert frag in seen, "kernel not found: " + frag
        v, s, o = seen[frag]
        assert v <= mv and s <= ms and o >= mo, (frag, "VGPRs %d (<= %d), scratch %d (<= %d), waves/SIMD %d (>= %d)" % (v, mv, s, ms, o, mo))


def test_old_instances_are_still_built():
    """TC_MSD_SPLIT=0 runs them: the four partition instances and the joint count of 64-bit keys"""
    names = list(kernel_resources.resources())
    for frag in _mod.KERNELS + ["msd_count_kernelILb0ELb1EE"]:
        assert any(frag in n for n in names), frag


@pytest.mark.parametrize("defs", [[], ["-DMSD_PROFILE"]], ids=["default", "MSD_PROFILE"])
def test_split_prefetch_destinations_are_untouched_until_they_land(defs):
    assert _mod.check(defs, kernels=SPLIT_PARTITION) >= len(SPLIT_PARTITION)
