"""The lanes of the unique-substring calls (csrc/tc_sus.hpp) need no device to be walked: host/check/sus_kernels.cpp compiles the
lanes of sus_prefix_kernel, sus_mark_kernel and sus_point_kernel, the range minimum of csrc/tc_lz.hpp and the row search of
csrc/tc_fm_ms.hpp with the host compiler under ASan + UBSan, builds the suffix array, the LCP array, the two scans and the min tree
at fan-outs 4 and 64 naively in heap blocks of the library's sizes, and compares every up, every MUS and every point answer with
brute force on unary, periodic, Fibonacci, random and text + copy texts, on a long MUS with a short one at its end and on a
staircase.  The program itself asserts what no device test can see: the range minimum and the leftmost search reached every level
of a fan-out-4 tree, an answer of each of the three kinds, a tie resolved to the left, an interior minimum, a position no MUS
covers, positions with up = 0, p = 0 and p = n - 1.  It is a plain executable; nothing of it is loaded into this process."""
import os
import shutil
import subprocess


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "text-compression_amd")


def test_sus_kernels_host_check(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "sus_kernels")
    # (-Wno-unused-function, as the library's own build: tc_fm_ms.hpp also defines the kernels this program does not call)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(PKG, "csrc"), os.path.join(PKG, "host", "check", "sus_kernels.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok: the unique substrings of" in r.stdout and "every tree level reached at fan-out 4" in r.stdout
