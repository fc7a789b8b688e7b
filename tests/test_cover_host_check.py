"""The lanes of the repeat-cover calls (csrc/tc_cov.hpp) need no device to be walked: host/check/cover_kernels.cpp compiles both
instances of cov_seed_kernel, the per-lane bodies of the cover core (cov_reach, cov_lane_bits), the range minimum of csrc/tc_lz.hpp
and the row searches of csrc/tc_fm_ms.hpp with the host compiler under ASan + UBSan, builds the suffix array, the LCP array, the two
min trees at fan-outs 4 and 64, the tiles' maxima and the spine naively in heap blocks of the library's sizes, and compares every
seed, cover and span with brute force on unary, periodic, Fibonacci, random and text + copy texts of 1 .. 2200 bytes, and the
general form on arrays no text produces.  The program itself asserts what no device test can see: both searches and the range
minimum reached every level of a fan-out-4 tree, a group of exactly q and of q - 1 rows, a leftmost occurrence refused under LATER,
a reach clamped to n, a reach carried over a tile with no seed.  It is a plain executable; nothing of it is loaded into this
process."""
import os
import shutil
import subprocess


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "text-compression_amd")


def test_cover_kernels_host_check(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "cover_kernels")
    # (-Wno-unused-function, as the library's own build: tc_fm_ms.hpp also defines the kernels this program does not call)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(PKG, "csrc"), os.path.join(PKG, "host", "check", "cover_kernels.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok: the repeat cover of" in r.stdout and "every tree level reached at fan-out 4" in r.stdout
