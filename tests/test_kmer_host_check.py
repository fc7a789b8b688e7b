"""The per-lane bodies of the k-mer kernels (csrc/tc_kmer.hpp) need no device to be walked: host/check/kmer_kernels.cpp
compiles them with the host compiler under ASan + UBSan and plays the kernels around them one lane after another over heap
blocks of exactly N entries -- the boundary masks, the groups closed from the lanes' and the tiles' carries, the spectrum bins
and the profile's two histograms -- against a naive scan, on unary, periodic, Fibonacci and random texts of 1 to 2200 bytes
and on arrays no text has (random lcp and sa words, values above n).  The workgroup scans and the atomics are checked on
the device only (tests/test_gpu_kmers.py).  It is a plain executable; nothing of it is loaded into this process."""
import os
import shutil
import subprocess


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "text-compression_amd")


def test_kmer_kernels_host_check(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "kmer_kernels")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(PKG, "csrc"), os.path.join(PKG, "host", "check", "kmer_kernels.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok: the k-mers of" in r.stdout and "arrays no text has" in r.stdout
