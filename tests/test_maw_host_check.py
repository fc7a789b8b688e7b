"""The lanes of the minimal absent words (csrc/tc_maw.hpp) need no device to be walked: host/check/maw_kernels.cpp compiles the
body of maw_row_kernel at both set widths, the range OR and the two row searches of csrc/tc_fm_ms.hpp with the host compiler
under ASan + UBSan, builds the suffix array, the LCP array, the last column, the change counts, the min tree and the OR tree at
fan-outs 4 and 64 naively in heap blocks of the library's sizes, and compares every row's words, in order, with a stack walk
(itself held against the definition on the short texts) on unary, periodic, Fibonacci, random and text + copy texts under several
length windows.  The program itself asserts what no device test can see: a range OR reached every level of a fan-out-4 tree, the
dropped first child, a child of the primary row alone, the chg exit, the lb = k - 1 shortcut, a lane with words for both its
children, and a wide set with members in all four words.  It is a plain executable; nothing of it is loaded into this process."""
import os
import shutil
import subprocess


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "text-compression_amd")


def test_maw_kernels_host_check(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "maw_kernels")
    # (-Wno-unused-function, as the library's own build: tc_fm_ms.hpp also defines the kernels this program does not call)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(PKG, "csrc"), os.path.join(PKG, "host", "check", "maw_kernels.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok: the minimal absent words of" in r.stdout and "every tree level reached at fan-out 4" in r.stdout
