"""The suffix sort's chain-round policy (csrc/tc_sa_plan.hpp: ChainPolicy) needs no device: host/check/sa_chain_policy.cpp
drives it through the sequences its comment promises, built with the host compiler under ASan + UBSan."""
import os
import shutil
import subprocess


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "text-compression_amd")


def test_chain_policy_host_check(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "sa_chain_policy")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(PKG, "csrc"), os.path.join(PKG, "host", "check", "sa_chain_policy.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok: chain-round policy" in r.stdout
