"""The lanes of the document queries on the kept enhanced suffix array (csrc/tc_esa_docs.hpp) need no device to be walked:
host/check/esa_docs_kernels.cpp compiles esd_doc_of and both instances of esd_doc_kernel with the row searches of csrc/tc_fm_ms.hpp
with the host compiler under ASan + UBSan, builds sa, isa, lcp, da, pv and the min trees of lcp and pv at fan-outs 4 and 64 naively in
heap blocks of the library's exact sizes, and compares every count and list (order and hit positions included) with loops over the bytes
on unary, periodic, Fibonacci and random texts of 0 .. 2601 bytes in 1 .. n documents.  The program itself asserts what no device test
can see: the search over pv reached every level of a fan-out-4 tree, the loop ended at hi, at limit, after ndocs steps and at the end of
its segment, len = 0, rows 1 and N - 1 and empty documents first, last and adjacent were asked, a pv and a tree of arbitrary contents
keep every access in bounds and the loop finite, and every query that leaves the text raised the flag on null arrays.  It is a plain
executable; nothing of it is loaded into this process."""
import os
import shutil
import subprocess


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "text-compression_amd")


def test_esa_docs_kernels_host_check(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "esa_docs_kernels")
    # (-Wno-unused-function, as the library's own build: the headers also define kernels this program does not call)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(PKG, "csrc"), os.path.join(PKG, "host", "check", "esa_docs_kernels.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok: the document queries on the kept ESA of" in r.stdout and "every tree level reached at fan-out 4" in r.stdout
