"""ec_repair_segments_sized from a plain C program (tests/c/repair_sized_test.c):
what a cgo binding sees -- include/uplink_ec.h and libuplink_ec.so, device
memory through ec_device_alloc / ec_copy, no Python or torch in the process --
three segments of three sizes in one call with the share check on, checked
against the CPU oracle."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "c", "repair_sized_test.c")


@pytest.mark.gpu
def test_c_client_repair_sized(tmp_path, oracle, native):
    lib = os.path.join(ROOT, "uplink_amd", "lib")
    orc = os.path.join(ROOT, "oracle", "build")
    binary = str(tmp_path / "repair_sized_test")
    cc = subprocess.run([os.environ.get("CC", "cc"), "-O2", "-std=gnu11", "-Wall", "-Werror",
                         "-I" + os.path.join(ROOT, "include"), "-o", binary, SRC, "-L" + lib, "-luplink_ec", "-L" + orc,
                         "-linfectious_oracle", "-Wl,-rpath," + lib, "-Wl,-rpath," + orc],
                        capture_output=True, text=True, timeout=120)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    env = dict(os.environ, UPLINK_EC_JIT_CACHE=str(tmp_path / "jit"))
    r = subprocess.run([binary], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1].startswith("ok")
