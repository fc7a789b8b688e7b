"""The candidate kernel of the tandem repeats (csrc/tc_tr.hpp) needs no device to be walked: host/check/tr_kernels.cpp compiles
its body -- and the range minimum of csrc/tc_lz.hpp and the upward row search of csrc/tc_fm_ms.hpp it calls -- with the host
compiler under ASan + UBSan, builds the suffix, inverse and LCP arrays of the text and of its reverse and the four min trees at
fan-outs 4 and 64 naively in heap blocks of the library's sizes, and compares both candidate words of every position with brute
force: the rule evaluated by scanning the text, and the runs of the definition as a whole (every run once, nothing else), on
unary, periodic, edited, Fibonacci, random and skewed texts.  The program itself asserts what no device test can see: both
searches and both range minima climbed to every level of a fan-out-4 tree.  It is a plain executable; nothing of it is loaded
into this process."""
import os
import shutil
import subprocess


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "text-compression_amd")


def test_tr_kernels_host_check(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "tr_kernels")
    # (-Wno-unused-function, as the library's own build: tc_fm_ms.hpp also defines the kernels this program does not call)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(PKG, "csrc"), os.path.join(PKG, "host", "check", "tr_kernels.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok: the runs of" in r.stdout and "every tree level reached at fan-out 4" in r.stdout
