"""The row kernel of the two-text comparison (csrc/tc_tm.hpp) needs no device to be walked: host/check/tm_kernels.cpp
compiles its body -- and the range minimum of csrc/tc_lz.hpp and the two row searches of csrc/tc_fm_ms.hpp it calls -- with
the host compiler under ASan + UBSan, builds the enhanced suffix array of Q T, the min tree at fan-outs 4 and 64, the T-row
counts and the two row lists naively in heap blocks of the library's sizes, and runs both instances of tm_row_kernel per Q
row against brute force on the two texts alone: unary, periodic, Fibonacci and random pairs, Q = T, Q a suffix of T's
period, a nearest T row thousands of rows away.  The program itself asserts what no device test can see: the clamp to the
query's end fired, and both row searches climbed to every level of a fan-out-4 tree.  It is a plain
executable; nothing of it is loaded into this process."""
import os
import shutil
import subprocess


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "text-compression_amd")


def test_tm_kernels_host_check(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "tm_kernels")
    # (-Wno-unused-function, as the library's own build: tc_fm_ms.hpp also defines the kernels this program does not call)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(PKG, "csrc"), os.path.join(PKG, "host", "check", "tm_kernels.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok: the matching statistics of" in r.stdout and "cut at the query's end" in r.stdout
