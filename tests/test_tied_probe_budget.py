"""CPU-only: the resources of tied_probe_w_kernel<S> (csrc/tc_sa.hpp), read from the code object's resource-usage remarks
as tests/test_kernel_budgets.py does.  The launch is sized for three workgroups of 256 threads per CU (sa_keyonly_recover:
3 x CUs): that is 3 waves per SIMD, so at most 168 VGPRs (512 / 3, in granules of 8), and at most a third of a CU's
160 KiB of LDS per workgroup -- the filter's 32 KiB and 4 x 65 x 80 bytes of raw text.  No scratch: the window, the next
turn's text and the dwords of the exact value are register arrays with constant indices.  S = 3 is the benchmark's
instance (ACGTN): 102 VGPRs when this was written, 137 for S = 8."""
import kernel_resources

LDS_PER_CU = 160 * 1024


def test_tied_probe_w_kernel_resources():
    res = {name: r for name, r in kernel_resources.remarks().items() if "tied_probe_w_kernelILi" in name}
    assert len(res) == 8, sorted(res)
    for name, r in sorted(res.items()):
        print(name, r)
        assert r["scratch"] == 0, (name, r)
        assert r["vgprs"] + r["agprs"] <= 168 and r["waves"] >= 3, (name, r)
        assert 3 * r["lds"] <= LDS_PER_CU, (name, r)
    s3 = next(r for name, r in res.items() if "tied_probe_w_kernelILi3E" in name)
    assert s3["vgprs"] <= 136, s3
