"""Host side of AES-256-GCM with a size per segment (ec_gcm_seal_segments_sized,
ec_gcm_open_segments_sized; uplink_amd/encryption.py, uploads.py): the exports
and their binding, cipher_geometry, and the pure geometry header
(uplink_amd/csrc/gcm_sized_geom.hpp) under the sanitizers.  No device needed."""
import ctypes
import os
import shutil
import subprocess

import pytest

from uplink_amd import _native, encryption, uploads

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_exports_exist_and_reject_null_arguments(native):
    for name in ("ec_gcm_seal_segments_sized", "ec_gcm_open_segments_sized", "ec_gcm_sized_stats"):
        assert name in _native.SIGNATURES
        assert hasattr(native, name)
    ptr = (ctypes.c_void_p * 1)(16)
    nb = (ctypes.c_size_t * 1)(1)
    bad = _native.EC_ERR_INVALID_ARG
    assert native.ec_gcm_seal_segments_sized(None, 1, ptr, nb, None, 16, 16, 16, ptr, None) == bad
    assert native.ec_gcm_seal_segments_sized(None, 0, None, None, None, 16, None, None, None, None) == bad  # (no context)
    assert native.ec_gcm_open_segments_sized(None, 1, ptr, nb, 16, 16, 16, ptr, 16, None) == bad
    assert native.ec_gcm_open_segments_sized(None, 0, None, None, 16, None, None, None, None, None) == bad
    assert native.ec_gcm_sized_stats(None, None, None, None) == bad
    with open(_native.HEADER) as fh:
        text = fh.read()
    for want in ("ec_gcm_seal_segments_sized(", "ec_gcm_open_segments_sized(", "ec_gcm_sized_stats(",
                 "splitter.go:156,170", "store.go:347-382"):
        assert want in text, want


def test_bindings_reject_mismatched_lists():
    class S:
        ctx = None

    s = S()
    for ins, nb, outs in (([16], [1, 2], [32]), ([16], [1], [32, 48]), ([16, 16], [1], [32]), ([16], [-1], [32])):
        with pytest.raises(ValueError):
            encryption.seal_segments_sized(s, ins, nb, 16, 16, 16, outs)
        with pytest.raises(ValueError):
            encryption.open_segments_sized(s, ins, nb, 16, 16, 16, outs, 16)
    with pytest.raises(ValueError):
        encryption.seal_segments_sized(s, [16], [1], 16, 16, 16, [32], data_len=[1, 2])
    with pytest.raises(ValueError):
        encryption.seal_segments_sized(s, [16], [1], 16, 16, 16, [32], data_len=[-1])


def test_cipher_geometry_agrees_with_the_pipeline():
    from uplink_amd.pipeline import SegmentGeometry

    class Scheme:
        def stripe_size(self):
            return 29 * 256

        def erasure_share_size(self):
            return 256

    for size in (0, 1, 7403, 7404, 7405, 100000, 67108864):
        g = SegmentGeometry(size, Scheme())
        assert uploads.cipher_geometry(size) == (g.nblocks, g.plain_cap, g.enc_len), size
    assert uploads.cipher_geometry(7404) == (1, 7408, 7424)
    assert uploads.cipher_geometry(7405) == (2, 14816, 14848)
    assert uploads.cipher_geometry(100, 32) == (7, 112, 224)
    with pytest.raises(ValueError):
        uploads.cipher_geometry(-1)
    with pytest.raises(ValueError):
        uploads.cipher_geometry(1, 16)


def test_gcm_sized_geom_under_the_sanitizers(tmp_path):
    """tests/c/gcm_sized_geom_test.cpp: a stand-alone program over gcm_sized_geom.hpp (workgroups
    per segment at 0, 1, 3, 4, 5, 8 and 9 blocks; the capped regime with a grid of 8 and segments
    of 1, 5 and 1000 blocks; the workgroup -> segment map covering every workgroup exactly once
    for a list in both orders; the stride loop visiting every block of its segment exactly once;
    the pass split at 4096 / 4097; the data_len rule at every residue edge), compiled with the
    host compiler and -fsanitize=address,undefined, run directly."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    binary = str(tmp_path / "gcm_sized_geom_test")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "uplink_amd", "csrc"), "-o", binary,
                         os.path.join(HERE, "c", "gcm_sized_geom_test.cpp")], capture_output=True, text=True,
                        timeout=300)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    r = subprocess.run([binary], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "ok" and not r.stderr.strip(), r.stdout + r.stderr
