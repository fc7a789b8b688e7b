"""The repeats kernel (csrc/tc_rep.hpp) needs no device to be walked: host/check/rep_kernels.cpp compiles its body -- and the
two row searches of csrc/tc_fm_ms.hpp it calls -- with the host compiler under ASan + UBSan, builds the suffix array, the LCP
array, the last column, the change counts and the min tree naively at fan-outs 4 and 64 in heap blocks of the library's
sizes, and compares every row's packed word, for both kinds and several filters, with one stack walk over the LCP array, on
unary, periodic, Fibonacci and random texts of 1 to 2200 bytes and on the two 257-occurrence texts.  It is a plain
executable; nothing of it is loaded into this process."""
import os
import shutil
import subprocess


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "text-compression_amd")


def test_rep_kernels_host_check(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "rep_kernels")
    # (-Wno-unused-function, as the library's own build: tc_fm_ms.hpp also defines the kernels this program does not call)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(PKG, "csrc"), os.path.join(PKG, "host", "check", "rep_kernels.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok: the repeats of" in r.stdout and "supermaximal" in r.stdout
