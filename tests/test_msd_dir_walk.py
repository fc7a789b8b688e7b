"""The tile cursor of the aligned MSD level over its directory of live parents (csrc/tc_msd_dir.hpp) needs no device:
host/check/msd_dir_walk.cpp compares it, tile by tile, with a transcription of the walk over the parent tables that it
replaces (csrc/tc_msd.hpp: msd_cur_init / msd_cur_info) -- no live parent, one, parents at both ends only, counts around
a tile, runs of one-tile parents, more parents than the directory holds, refills that find nothing, capacity 1, random
tables -- built with the host compiler under ASan + UBSan."""
import os
import shutil
import subprocess


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "text-compression_amd")


def test_msd_dir_walk_host_check(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "msd_dir_walk")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(PKG, "csrc"), os.path.join(PKG, "host", "check", "msd_dir_walk.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok: directory walk of the aligned MSD level" in r.stdout
