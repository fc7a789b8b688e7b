"""The centre kernel of the palindromes (csrc/tc_pal.hpp) needs no device to be walked: host/check/pal_kernels.cpp compiles its
body -- and the range minimum of csrc/tc_lz.hpp it calls -- with the host compiler under ASan + UBSan, builds the joint text, its
suffix, inverse and LCP arrays and the min tree at fan-outs 4 and 64 naively in heap blocks of the library's sizes, and compares
every centre's word with brute force on unary, periodic, Fibonacci, random, planted-hairpin and whole-text-palindrome texts, under
the identity and the DNA complement, for the budgets 0, 1, 3 and 16.  The program itself asserts what no device test can see: the
range minimum climbed to every level of a fan-out-4 tree, the clamp fired, some lane used all m + 1 turns, some lane's trim
dropped a trailing mismatch, and the direct compare and the range minimum each decided some extension.  It is a plain
executable; nothing of it is loaded into this process."""
import os
import shutil
import subprocess


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "text-compression_amd")


def test_pal_kernels_host_check(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "pal_kernels")
    # (-Wno-unused-function, as the library's own build: tc_fm_ms.hpp also defines the kernels this program does not call)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(PKG, "csrc"), os.path.join(PKG, "host", "check", "pal_kernels.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok: the palindromes of" in r.stdout and "every tree level reached at fan-out 4" in r.stdout
