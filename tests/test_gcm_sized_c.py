"""ec_gcm_seal_segments_sized and ec_gcm_open_segments_sized from a plain C
program (tests/c/gcm_sized_test.c): what a cgo binding sees -- include/uplink_ec.h
and libuplink_ec.so, device memory through ec_device_alloc / ec_copy, no Python or
torch in the process -- three segments of three sizes sealed in one call and
opened in another.  The expected ciphertexts are computed here, by the CPU
oracle over the same generated plaintexts, keys and nonces, and handed to the
program as hex."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "c", "gcm_sized_test.c")

IN_BLOCK = 7408
NBLOCKS = [1, 3, 4]  # as in gcm_sized_test.c


def _segment(g, nbytes):
    """gcm_sized_test.c seg_byte"""
    i = np.arange(nbytes, dtype=np.uint64)
    return (((i * np.uint64(2654435761) + np.uint64(g * 40503)) >> np.uint64(11)) & np.uint64(0xFF)).astype(np.uint8)


def _key(g):
    return bytes((g * 37 + i * 11 + 5) & 0xFF for i in range(32))


def _nonce(g):
    return bytes((g * 101 + i * 7 + 250) & 0xFF for i in range(12))


@pytest.mark.gpu
def test_c_client_sized_cipher(tmp_path, oracle, native):
    from oracle import aesgcm as ag

    lib = os.path.join(ROOT, "uplink_amd", "lib")
    binary = str(tmp_path / "gcm_sized_test")
    cc = subprocess.run([os.environ.get("CC", "cc"), "-O2", "-std=gnu11", "-Wall", "-Werror",
                         "-I" + os.path.join(ROOT, "include"), "-o", binary, SRC, "-L" + lib, "-luplink_ec",
                         "-Wl,-rpath," + lib], capture_output=True, text=True, timeout=120)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    want = [ag.encrypt_blocks(_key(g), _nonce(g), _segment(g, nb * IN_BLOCK), IN_BLOCK).tobytes().hex()
            for g, nb in enumerate(NBLOCKS)]
    env = dict(os.environ, UPLINK_EC_JIT_CACHE=str(tmp_path / "jit"))
    r = subprocess.run([binary] + want, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1].startswith("ok")
