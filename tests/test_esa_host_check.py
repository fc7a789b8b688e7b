"""The query lanes of the kept enhanced suffix array (csrc/tc_esa.hpp) need no device to be walked: host/check/esa_kernels.cpp
compiles esa_lce_kernel, esa_find_kernel and esa_compare_kernel, the range minimum of csrc/tc_lz.hpp and the row searches of
csrc/tc_fm_ms.hpp with the host compiler under ASan + UBSan, builds the text, sa, isa, lcp and the two min trees at fan-outs 4 and 64
naively in heap blocks of the library's exact sizes, and compares every answer with loops over the bytes on unary, periodic,
Fibonacci, random and text + copy texts of 0 .. 2601 bytes.  The program itself asserts what no device test can see: both searches
and the range minimum reached every level of a fan-out-4 tree, the direct compare and the range minimum each decided an extension,
the clamp fired, a lane took all m + 1 turns, positions 0, n - 1 and n, a == b, len = 0 and len = n were asked, and every query
that leaves the text raised the flag with every access in bounds.  It is a plain executable; nothing of it is loaded into this
process."""
import os
import shutil
import subprocess


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "text-compression_amd")


def test_esa_kernels_host_check(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "esa_kernels")
    # (-Wno-unused-function, as the library's own build: tc_fm_ms.hpp also defines the kernels this program does not call)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(PKG, "csrc"), os.path.join(PKG, "host", "check", "esa_kernels.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok: the queries on the kept ESA of" in r.stdout and "every tree level reached at fan-out 4" in r.stdout
