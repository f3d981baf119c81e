"""The share pick of the share-set calls (uplink_amd/csrc/share_pick.hpp)
against the oracle's Rebuild, under the sanitizers.  No device needed."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_share_pick_under_the_sanitizers(tmp_path):
    """tests/c/share_pick_test.cpp: a stand-alone program over share_pick.hpp
    (every subset of RS(2,4) and RS(3,7) in five orders, random lists of
    RS(4,10) and RS(29,80): the k picked are the k the oracle's or_rebuild reads,
    `missing` and the rest are as documented; the refused lists with the
    oracle's codes), compiled with the host compilers and
    -fsanitize=address,undefined, run directly."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    cc = os.environ.get("CC") or shutil.which("gcc") or shutil.which("cc")
    assert cxx and cc, "no host C / C++ compiler"
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    obj, binary = str(tmp_path / "infectious_oracle.o"), str(tmp_path / "share_pick_test")
    steps = [[cc, "-std=gnu11", *san, "-c", os.path.join(ROOT, "oracle", "infectious_oracle.c"), "-o", obj],
             [cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", *san, "-I" + os.path.join(ROOT, "uplink_amd", "csrc"),
              "-o", binary, os.path.join(HERE, "c", "share_pick_test.cpp"), obj, "-lpthread"]]
    for cmd in steps:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([binary], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "ok" and not r.stderr.strip(), r.stdout + r.stderr
