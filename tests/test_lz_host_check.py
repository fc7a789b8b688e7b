"""The LPF kernel and its range minimum (csrc/tc_lz.hpp) need no device to be walked: host/check/lz_kernels.cpp compiles
their bodies -- and the two row searches of csrc/tc_fm_ms.hpp they call -- with the host compiler under ASan + UBSan, builds
the suffix array, the LCP array and the two min trees naively at fan-outs 4 and 64 in heap blocks of the library's sizes,
and runs lz_range_min against a running minimum and lz_lpf_kernel per row against brute force over all j < i, on unary,
periodic, Fibonacci and random texts.  The program itself asserts what no device test can see: the range minimum climbed to
every level of a fan-out-4 tree at least once.  It is a plain executable; nothing of it is loaded into this process."""
import os
import shutil
import subprocess


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "text-compression_amd")


def test_lz_kernels_host_check(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "lz_kernels")
    # (-Wno-unused-function, as the library's own build: tc_fm_ms.hpp also defines the kernels this program does not call)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(PKG, "csrc"), os.path.join(PKG, "host", "check", "lz_kernels.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok: " in r.stdout and "range minima; the LPF array of" in r.stdout
