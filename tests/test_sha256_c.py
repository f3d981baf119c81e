"""ec_sha256_segments_sized and ec_sha256_pieces_list from a plain C program
(tests/c/sha256_test.c): what a cgo binding sees -- include/uplink_ec.h and
libuplink_ec.so, device memory through ec_device_alloc / ec_copy, no Python or
torch in the process -- the SHA-256 piece hashes of three segments of three sizes
in one call, and a list of three pieces, one of them empty.  The expected
digests are computed here, by hashlib over the oracle's pieces of the same
generated segments, and handed to the program."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "c", "sha256_test.c")

K, N, ESS = 29, 80, 256
STRIPES = [3, 1025, 41]          # as in sha256_test.c
LIST = [(0, 4096), (4097, 3000), (0, 0)]  # (offset, length) windows of segment 0


def _segment(g, nbytes):
    """sha256_test.c seg_byte"""
    i = np.arange(nbytes, dtype=np.uint64)
    return (((i * np.uint64(2654435761) + np.uint64(g * 40503)) >> np.uint64(11)) & np.uint64(0xFF)).astype(np.uint8)


@pytest.mark.gpu
def test_c_client_sha256(tmp_path, oracle, native):
    lib = os.path.join(ROOT, "uplink_amd", "lib")
    binary = str(tmp_path / "sha256_test")
    cc = subprocess.run([os.environ.get("CC", "cc"), "-O2", "-std=gnu11", "-Wall", "-Werror",
                         "-I" + os.path.join(ROOT, "include"), "-o", binary, SRC, "-L" + lib, "-luplink_ec",
                         "-Wl,-rpath," + lib], capture_output=True, text=True, timeout=120)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    f = oracle.FEC(K, N)
    segs = [_segment(g, s * K * ESS) for g, s in enumerate(STRIPES)]
    seg_hashes = b"".join(hashlib.sha256(row.tobytes()).digest()
                          for sg in segs for row in f.encode_segment(sg, ESS, threads=8))
    list_hashes = b"".join(hashlib.sha256(segs[0][o:o + ln].tobytes()).digest() for o, ln in LIST)
    env = dict(os.environ, UPLINK_EC_JIT_CACHE=str(tmp_path / "jit"))
    r = subprocess.run([binary, seg_hashes.hex(), list_hashes.hex()], capture_output=True, text=True, timeout=120,
                       env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1].startswith("ok")
