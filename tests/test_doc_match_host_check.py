"""The lanes of the cross-document matches on the kept enhanced suffix array (csrc/tc_esa_xdoc.hpp) need no device to be walked:
host/check/esx_kernels.cpp compiles both instances of esx_match_kernel, with the row searches of csrc/tc_fm_ms.hpp and the range minimum
of csrc/tc_lz.hpp, and the lane bodies of the run-head scans, of the per-document sums and of the segmented maximum with the host
compiler under ASan + UBSan, builds sa, lcp, da and the min trees of lcp and da at fan-outs 4 and 64 naively in heap blocks of the exact
sizes, and compares every length, partner and document, every up / dn, every shared count and longest match with loops over the bytes
on unary, periodic, Fibonacci and random texts in 1 .. n documents.  The program itself asserts what no device test can see: both da
searches and the range minima reached every level of a five-level tree, the "no qualifying row" outcome on each side and on both, a
run longer than two tiles, a run head in an earlier tile, the clamp fired, empty documents first, last and adjacent, and a da, an up /
dn and trees of arbitrary contents keep every access in bounds.  It is a plain executable; nothing of it is loaded into this process."""
import os
import shutil
import subprocess


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "text-compression_amd")


def test_esx_kernels_host_check(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "esx_kernels")
    # (-Wno-unused-function, as the library's own build: the headers also define kernels this program does not call)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(PKG, "csrc"), os.path.join(PKG, "host", "check", "esx_kernels.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok: the cross-document matches of" in r.stdout and "every tree level reached at fan-out 4" in r.stdout
