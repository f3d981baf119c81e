"""ec_gcm_open_ranges_sized from a plain C program (tests/c/gcm_ranged_test.c): what
a cgo binding sees -- include/uplink_ec.h and libuplink_ec.so, device memory
through ec_device_alloc / ec_copy, no Python or torch in the process -- three
ranges of three segments opened in one call, at aligned and at odd addresses.
The covered blocks' ciphertext and the expected plaintext of each range are
computed here, by the CPU oracle over generated plaintexts, keys and nonces, and
handed to the program as hex."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "c", "gcm_ranged_test.c")

IN_BLOCK = 7408
# (first block, covered blocks, head, length) as in gcm_ranged_test.c
RANGES = [(0, 2, 0, 2 * IN_BLOCK), (3, 3, 6608, 10000), (1, 1, 17, 1)]


def _key(g):
    return bytes((g * 37 + i * 11 + 5) & 0xFF for i in range(32))


def _nonce(g):
    return bytes((g * 101 + i * 7 + 250) & 0xFF for i in range(12))


@pytest.mark.gpu
def test_c_client_ranged_open(tmp_path, oracle, native):
    from oracle import aesgcm as ag
    from uplink_amd.streams import calc_encompassing_blocks

    lib = os.path.join(ROOT, "uplink_amd", "lib")
    binary = str(tmp_path / "gcm_ranged_test")
    cc = subprocess.run([os.environ.get("CC", "cc"), "-O2", "-std=gnu11", "-Wall", "-Werror",
                         "-I" + os.path.join(ROOT, "include"), "-o", binary, SRC, "-L" + lib, "-luplink_ec",
                         "-Wl,-rpath," + lib], capture_output=True, text=True, timeout=120)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    rng = np.random.default_rng(20261023)
    args = []
    for g, (fb, nb, head, length) in enumerate(RANGES):
        assert calc_encompassing_blocks(head, length, IN_BLOCK) == (0, nb)
        start = ag.increment(_nonce(g), fb)
        cipher = ag.encrypt_blocks(_key(g), start, rng.integers(0, 256, nb * IN_BLOCK, dtype=np.uint8), IN_BLOCK)
        plain, bad = ag.decrypt_blocks(_key(g), start, cipher, IN_BLOCK)
        assert bad == -1
        args += [cipher.tobytes().hex(), plain[head:head + length].tobytes().hex()]
    env = dict(os.environ, UPLINK_EC_JIT_CACHE=str(tmp_path / "jit"))
    r = subprocess.run([binary] + args, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1].startswith("ok")
