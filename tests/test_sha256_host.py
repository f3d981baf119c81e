"""Host side of the SHA-256 piece hash (include/uplink_ec.h ec_sha256_*;
uplink_amd/piecehash.py): the exports and their binding, and the pure geometry
header (uplink_amd/csrc/sha_list_geom.hpp) with the kernel's own rounds and tail
builder (sha256_device.hpp) compiled for the host, under the sanitizers, over
tests/golden/sha256_vectors.json.  No device needed."""
import ctypes
import hashlib
import json
import os
import shutil
import subprocess

import pytest

from uplink_amd import _native, eestream, piecehash

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "sha256_vectors.json")

EXPORTS = ("ec_sha256_pieces_list", "ec_sha256_segments_sized", "ec_sha256_pieces", "ec_sha256_host",
           "ec_sha256_set_launch_blocks", "ec_sha256_list_stats")


def test_exports_exist_and_reject_null_arguments(native):
    for name in EXPORTS:
        assert name in _native.SIGNATURES
        assert hasattr(native, name)
    ptr = (ctypes.c_void_p * 1)(16)
    ln = (ctypes.c_size_t * 1)(1)
    bad = _native.EC_ERR_INVALID_ARG
    assert native.ec_sha256_pieces_list(None, 1, ptr, ln, 16, None) == bad
    assert native.ec_sha256_pieces_list(None, 1, None, ln, 16, None) == bad
    assert native.ec_sha256_pieces_list(None, 1, ptr, None, 16, None) == bad
    assert native.ec_sha256_pieces_list(None, 1, ptr, ln, None, None) == bad
    assert native.ec_sha256_pieces_list(None, 0, None, None, None, None) == bad  # (no context)
    assert native.ec_sha256_segments_sized(None, 1, ptr, ln, ptr, 0, 16, None) == bad
    assert native.ec_sha256_segments_sized(None, 1, ptr, None, ptr, 0, 16, None) == bad
    assert native.ec_sha256_segments_sized(None, 1, ptr, ln, None, 0, 16, None) == bad
    assert native.ec_sha256_segments_sized(None, 1, ptr, ln, ptr, 0, None, None) == bad
    assert native.ec_sha256_segments_sized(None, 1, None, ln, ptr, _native.EC_FLAG_PARITY_ONLY, 16, None) == bad
    # the uniform and the host form take no context: NULL hashes, NULL data with bytes to read
    assert native.ec_sha256_pieces(16, 1, 64, 64, 0, 0, None, None) == bad
    assert native.ec_sha256_pieces(None, 1, 64, 64, 0, 0, 16, None) == bad
    assert native.ec_sha256_pieces(None, 0, 64, 64, 0, 0, 16, None) == _native.EC_OK  # nothing to hash
    assert native.ec_sha256_pieces(16, 1, 0, 1 << 61, 0, 0, 16, None) == _native.EC_ERR_UNSUPPORTED  # 2^64 bits
    assert native.ec_sha256_host(None, 1, 64, 64, (ctypes.c_uint8 * 32)()) == bad
    assert native.ec_sha256_host((ctypes.c_uint8 * 64)(), 1, 64, 64, None) == bad
    assert native.ec_sha256_set_launch_blocks(None, 2) == bad
    assert native.ec_sha256_list_stats(None, None, None, None) == bad
    with open(_native.HEADER) as fh:
        text = fh.read()
    for want in [name + "(" for name in EXPORTS] + ["SHA-256 piece hashes (pb.PieceHashAlgorithm_SHA256, hash.go:15-26)",
                                                    "#define EC_HASH_SHA256 0", "#define EC_HASH_BLAKE3 1"]:
        assert want in text, want
    assert int(piecehash.PieceHashAlgorithm.SHA256) == 0 and int(piecehash.PieceHashAlgorithm.BLAKE3) == 1


def test_bindings_take_sha256_and_reject_mismatched_lists():
    class S:
        ctx = None
        _lib = None

    sha = piecehash.PieceHashAlgorithm.SHA256
    assert piecehash.DEFAULT_ALGORITHM == piecehash.PieceHashAlgorithm.BLAKE3  # hash.go:25
    for name in ("hash_pieces_list", "hash_host", "hash_device", "blake3_pieces_list", "blake3_host", "blake3_device"):
        assert callable(getattr(piecehash, name)), name
    # the list-length errors come before the algorithm matters, and SHA256 does not raise NotImplementedError
    with pytest.raises(ValueError):
        piecehash.hash_segments_sized(S(), [16], [1, 2], [32], 64, algo=sha)
    with pytest.raises(ValueError):
        piecehash.hash_segments_sized(S(), [16], [1], [32, 48], 64, algo=sha)
    with pytest.raises(ValueError):
        piecehash.hash_segments_sized(S(), [16, 16], [1], [32], 64, algo=sha)
    with pytest.raises(ValueError):
        piecehash.hash_segments_sized(S(), [16], [-1], [32], 64, algo=sha)
    with pytest.raises(ValueError):
        piecehash.hash_segments_sized(S(), None, [1], [32], 64, parity_only=True, algo=sha)
    with pytest.raises(ValueError):
        eestream.SegmentCodec(S()).hash_segments_sized([16], [1, 2], [32], 64, algo=sha)
    with pytest.raises(ValueError):  # not a value of pb.PieceHashAlgorithm
        piecehash.hash_segments_sized(S(), [16], [1], [32], 64, algo=7)
    torch = pytest.importorskip("torch")
    t = torch.zeros(8, dtype=torch.uint8)
    for call in (piecehash.hash_pieces_list, piecehash.blake3_pieces_list):
        with pytest.raises(ValueError):  # a hash buffer of another size than npieces*32
            call(S(), [t, t], hashes=torch.zeros(32, dtype=torch.uint8), algo=sha)
        with pytest.raises(ValueError):
            call(S(), [t.to(torch.int32)], algo=sha)
        with pytest.raises(ValueError):
            call(S(), [torch.zeros((4, 4), dtype=torch.uint8)[:, 1]], algo=sha)


def test_golden_vectors_are_hashlibs():
    with open(GOLDEN) as fh:
        cases = json.load(fh)["cases"]
    assert [c["length"] for c in cases] == [0, 3, 56, 112, 1000000]
    for c in cases:
        msg = bytes.fromhex(c["unit_hex"]) * c["repeat"]
        assert len(msg) == c["length"]
        assert hashlib.sha256(msg).hexdigest() == c["sha256"], c["name"]


def test_sha_list_geom_and_rounds_under_the_sanitizers(tmp_path):
    """tests/c/sha_list_geom_test.cpp: a stand-alone program over sha_list_geom.hpp (block counts at
    0, 55, 56, 63, 64, 119, 120 and 2^32 + 5 bytes; the classes; the lane order a permutation,
    sorted within a class, no wave of two classes; the pass split at kPassPieces +- 1; the launch
    counts) and over sha256_device.hpp compiled for the host (the golden messages through the
    kernel's rounds and tail builder, also with the state carried between launches; the tail's
    length field at 2^29, 2^32 + 5 and 2^61 - 1 bytes from an injected state), compiled with the
    host compiler and -fsanitize=address,undefined, run directly."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    binary = str(tmp_path / "sha_list_geom_test")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "uplink_amd", "csrc"), "-o", binary,
                         os.path.join(HERE, "c", "sha_list_geom_test.cpp")], capture_output=True, text=True,
                        timeout=300)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    with open(GOLDEN) as fh:
        cases = json.load(fh)["cases"]
    args = [f"{c['repeat']}:{c['unit_hex']}:{c['sha256']}" for c in cases]
    r = subprocess.run([binary] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "ok" and not r.stderr.strip(), r.stdout + r.stderr
    # and a digest that is not the message's is told
    wrong = f"1:616263:{hashlib.sha256(b'abd').hexdigest()}"
    r = subprocess.run([binary, wrong], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "digest differs" in r.stderr, r.stdout + r.stderr
