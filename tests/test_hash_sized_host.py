"""Host side of the list form of the piece hash (ec_blake3_pieces_list,
ec_hash_segments_sized; uplink_amd/piecehash.py): the exports and their binding,
and the pure geometry header (uplink_amd/csrc/b3_list_geom.hpp) under the
sanitizers.  No device needed."""
import ctypes
import os
import shutil
import subprocess

import pytest

from uplink_amd import _native, eestream, piecehash

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_exports_exist_and_reject_null_arguments(native):
    for name in ("ec_blake3_pieces_list", "ec_hash_segments_sized", "ec_hash_list_stats"):
        assert name in _native.SIGNATURES
        assert hasattr(native, name)
    ptr = (ctypes.c_void_p * 1)(16)
    ln = (ctypes.c_size_t * 1)(1)
    bad = _native.EC_ERR_INVALID_ARG
    assert native.ec_blake3_pieces_list(None, 1, ptr, ln, 16, None) == bad
    assert native.ec_blake3_pieces_list(None, 1, None, ln, 16, None) == bad
    assert native.ec_blake3_pieces_list(None, 1, ptr, None, 16, None) == bad
    assert native.ec_blake3_pieces_list(None, 1, ptr, ln, None, None) == bad
    assert native.ec_blake3_pieces_list(None, 0, None, None, None, None) == bad  # (no context)
    assert native.ec_hash_segments_sized(None, 1, ptr, ln, ptr, 0, 16, None) == bad
    assert native.ec_hash_segments_sized(None, 1, ptr, None, ptr, 0, 16, None) == bad
    assert native.ec_hash_segments_sized(None, 1, ptr, ln, None, 0, 16, None) == bad
    assert native.ec_hash_segments_sized(None, 1, ptr, ln, ptr, 0, None, None) == bad
    assert native.ec_hash_segments_sized(None, 1, None, ln, ptr, _native.EC_FLAG_PARITY_ONLY, 16, None) == bad
    assert native.ec_hash_list_stats(None, None, None, None, None) == bad
    with open(_native.HEADER) as fh:
        text = fh.read()
    for want in ("ec_blake3_pieces_list(", "ec_hash_segments_sized(", "ec_hash_list_stats(", "upload.go:133,155,270",
                 "single.go:233-238"):
        assert want in text, want


def test_bindings_reject_mismatched_lists():
    class S:
        ctx = None
        _lib = None

    with pytest.raises(ValueError):
        piecehash.hash_segments_sized(S(), [16], [1, 2], [32], 64)
    with pytest.raises(ValueError):
        piecehash.hash_segments_sized(S(), [16], [1], [32, 48], 64)
    with pytest.raises(ValueError):
        piecehash.hash_segments_sized(S(), [16, 16], [1], [32], 64)
    with pytest.raises(ValueError):
        piecehash.hash_segments_sized(S(), [16], [-1], [32], 64)
    with pytest.raises(ValueError):
        piecehash.hash_segments_sized(S(), None, [1], [32], 64, parity_only=True)
    with pytest.raises(ValueError):
        eestream.SegmentCodec(S()).hash_segments_sized([16], [1, 2], [32], 64)
    torch = pytest.importorskip("torch")
    t = torch.zeros(8, dtype=torch.uint8)
    with pytest.raises(ValueError):  # a hash buffer of another size than npieces*32
        piecehash.blake3_pieces_list(S(), [t, t], hashes=torch.zeros(32, dtype=torch.uint8))
    with pytest.raises(ValueError):
        piecehash.blake3_pieces_list(S(), [t.to(torch.int32)])
    with pytest.raises(ValueError):
        piecehash.blake3_pieces_list(S(), [torch.zeros((4, 4), dtype=torch.uint8)[:, 1]])


def test_b3_list_geom_under_the_sanitizers(tmp_path):
    """tests/c/b3_list_geom_test.cpp: a stand-alone program over b3_list_geom.hpp (groups and
    node slots at 0, 1, 1024, 1025, 256 KiB, 256 KiB + 1, 64 MiB and 64 MiB + 1 bytes, the last
    oversize; the workgroup -> piece map covering every workgroup exactly once for a list in both
    orders; fast / byte classification by alignment and run; the pass split), compiled with the
    host compiler and -fsanitize=address,undefined, run directly."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    binary = str(tmp_path / "b3_list_geom_test")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "uplink_amd", "csrc"), "-o", binary,
                         os.path.join(HERE, "c", "b3_list_geom_test.cpp")], capture_output=True, text=True,
                        timeout=300)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    r = subprocess.run([binary], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "ok" and not r.stderr.strip(), r.stdout + r.stderr
