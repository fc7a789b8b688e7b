"""CPU-only helper of the budget tests: one cross-compile of csrc/textcomp.hip for gfx950 with hipcc's resource-usage
remarks (no GPU), parsed once per process.  resources() gives {mangled kernel name: (VGPRs, scratch bytes per lane,
waves per SIMD)}; run as a script it prints every kernel with all the remarks' figures, one line each, sorted -- the
listing to diff when a change must leave every kernel as it was."""
import functools
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "text-compression_amd")

FIELDS = (("vgprs", r"VGPRs: (\d+)"), ("agprs", r"AGPRs: (\d+)"), ("sgprs", r"SGPRs: (\d+)"),
          ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("waves", r"Occupancy \[waves/SIMD\]: (\d+)"),
          ("lds", r"LDS Size \[bytes/block\]: (\d+)"))


@functools.lru_cache(maxsize=None)
def remarks():
    """{mangled kernel name: {field: value}} for every kernel of the library."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as d:
        out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-pthread",
                              "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "csrc"),
                              "-Rpass-analysis=kernel-resource-usage", "-o", os.path.join(d, "libtextcomp_budget.so"),
                              os.path.join(PKG, "csrc", "textcomp.hip")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    res = {}
    for blk in out.stderr.split("Function Name: ")[1:]:
        res[blk.split()[0]] = {f: int(re.search(rx, blk).group(1)) for f, rx in FIELDS}
    return res


def resources():
    return {name: (r["vgprs"], r["scratch"], r["waves"]) for name, r in remarks().items()}


if __name__ == "__main__":
    for name, r in sorted(remarks().items()):
        print(name, " ".join("%s=%d" % (f, r[f]) for f, _ in FIELDS))
