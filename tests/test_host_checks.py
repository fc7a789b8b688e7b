"""The stand-alone host checks of text-compression_amd/host/check/: each compiles the lane bodies of one kernel header as plain
C++ with the host compiler under ASan + UBSan, runs them in heap blocks of exact size against brute force, and asserts what no
device test can see (every tree level reached, the clamp fired, arbitrary array contents stay in bounds); each program's head
comment says what it walks.  They are plain executables: nothing of them is loaded into this process.  A new check is one
more row here."""
import os
import shutil
import subprocess

import pytest


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "text-compression_amd")
# (-Wno-unused-function: the kernel headers and the shared check headers also define what a program does not call)
FLAGS = ["-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unused-function", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all"]

# source, extra flags, phrases that stdout must hold, what is checked
CHECKS = [
    ("cover_kernels.cpp", [], ("ok: the repeat cover of", "every tree level reached at fan-out 4"), "repeat-cover lanes, tc_cov.hpp"),
    ("esa_docs_kernels.cpp", [], ("ok: the document queries on the kept ESA of", "every tree level reached at fan-out 4"),
     "document queries on the kept ESA, tc_esa_docs.hpp"),
    ("esa_kernels.cpp", [], ("ok: the queries on the kept ESA of", "every tree level reached at fan-out 4"),
     "query lanes of the kept ESA, tc_esa.hpp"),
    ("esx_kernels.cpp", [], ("ok: the cross-document matches of", "every tree level reached at fan-out 4"),
     "cross-document matches, tc_esa_xdoc.hpp"),
    ("fm_count_kernels.cpp", [], ("ok: backward search of",), "FM-index backward search on damaged indexes, tc_fm_count.hpp"),
    ("fm_ms_kernels.cpp", [], ("ok: matching statistics of",), "matching statistics, MEMs and the row searches, tc_fm_ms.hpp"),
    ("kmer_kernels.cpp", [], ("ok: the k-mers of", "arrays no text has"), "k-mer lane bodies, tc_kmer.hpp"),
    # (csrc/tc_lcp.hpp carries a "#pragma unroll" the host compiler does not know)
    ("lcp_kernels.cpp", ["-Wno-unknown-pragmas"],
     ("400 texts x 3 caps exact", "runs of planted pairs exact", "malformed and wrong suffix arrays in bounds"),
     "LCP kernels on malformed suffix arrays, tc_lcp.hpp"),
    ("lz_kernels.cpp", [], ("ok: ", "range minima; the LPF array of"), "LPF kernel and the range minimum, tc_lz.hpp"),
    ("maw_kernels.cpp", [], ("ok: the minimal absent words of", "every tree level reached at fan-out 4"),
     "minimal-absent-word lanes, tc_maw.hpp"),
    ("msd_dir_walk.cpp", [], ("ok: directory walk of the aligned MSD level",), "directory walk of MSD level 3, tc_msd_dir.hpp"),
    ("pal_kernels.cpp", [], ("ok: the palindromes of", "every tree level reached at fan-out 4"), "palindrome kernel, tc_pal.hpp"),
    ("rep_kernels.cpp", [], ("ok: the repeats of", "supermaximal"), "repeats kernel, tc_rep.hpp"),
    ("sa_chain_policy.cpp", [], ("ok: chain-round policy",), "when a doubling round becomes a chain round, tc_sa_plan.hpp"),
    ("sus_kernels.cpp", [], ("ok: the unique substrings of", "every tree level reached at fan-out 4"),
     "unique-substring lanes, tc_sus.hpp"),
    ("tm_kernels.cpp", [], ("ok: the matching statistics of", "cut at the query's end"), "two-text comparison, tc_tm.hpp"),
    ("tr_kernels.cpp", [], ("ok: the runs of", "every tree level reached at fan-out 4"), "tandem-repeat kernel, tc_tr.hpp"),
]


@pytest.mark.parametrize("source,extra,phrases,what", CHECKS, ids=[c[0][:-len(".cpp")] for c in CHECKS])
def test_host_check(tmp_path, source, extra, phrases, what):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / source[:-len(".cpp")])
    subprocess.run([cxx] + FLAGS + extra + ["-I", os.path.join(PKG, "csrc"), os.path.join(PKG, "host", "check", source), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, what + "\n" + r.stdout + r.stderr
    for phrase in phrases:
        assert phrase in r.stdout, (what, phrase, r.stdout)
