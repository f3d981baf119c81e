"""ec_gcm_seal_messages / ec_gcm_open_messages from a plain C program
(tests/c/gcm_messages_test.c): what a cgo binding sees -- include/uplink_ec.h and
libuplink_ec.so, device memory through ec_device_alloc / ec_copy, no Python or
torch in the process -- three messages (100 bytes aligned, a 32-byte key at odd
addresses, an empty one) sealed in one call, opened in one call and opened again
with one of them tampered.  The plaintexts are generated here and the sealed
bytes computed by the CPU oracle, both handed to the program as hex."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "c", "gcm_messages_test.c")

LENS = [100, 32, 0]  # as in gcm_messages_test.c


def _key(g):
    return bytes((g * 37 + i * 11 + 5) & 0xFF for i in range(32))


def _nonce(g):
    return bytes((g * 101 + i * 7 + 250) & 0xFF for i in range(12))


@pytest.mark.gpu
def test_c_client_messages(tmp_path, oracle, native):
    from oracle import aesgcm as ag

    lib = os.path.join(ROOT, "uplink_amd", "lib")
    binary = str(tmp_path / "gcm_messages_test")
    cc = subprocess.run([os.environ.get("CC", "cc"), "-O2", "-std=gnu11", "-Wall", "-Werror",
                         "-I" + os.path.join(ROOT, "include"), "-o", binary, SRC, "-L" + lib, "-luplink_ec",
                         "-Wl,-rpath," + lib], capture_output=True, text=True, timeout=120)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    rng = np.random.default_rng(20261024)
    args = []
    for g, n in enumerate(LENS):
        plain = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        sealed = bytes(ag.seal(_key(g), _nonce(g), plain))
        assert len(sealed) == n + 16 and bytes(ag.open_(_key(g), _nonce(g), sealed))[:n] == plain
        args += [plain.hex() or "-", sealed.hex()]
    env = dict(os.environ, UPLINK_EC_JIT_CACHE=str(tmp_path / "jit"))
    r = subprocess.run([binary] + args, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1].startswith("ok")
