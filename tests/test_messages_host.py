"""Host side of the one-shot message cipher (ec_gcm_seal_messages /
ec_gcm_open_messages; uplink_amd/encryption.py seal_messages, open_messages): the
exports and their binding, and the two headers the kernel is built from, each
compiled into a stand-alone program under the sanitizers -- the arithmetic
(uplink_amd/csrc/gcm_msg_device.hpp) playing the 64 lanes of a wave in a loop
against the GCM specification's vectors and the CPU oracle, and the geometry
(gcm_msg_geom.hpp).  No device needed."""
import ctypes
import os
import shutil
import subprocess
import sys

import pytest

from uplink_amd import _native, encryption

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)


def test_exports_exist_and_reject_null_arguments(native):
    for name in ("ec_gcm_seal_messages", "ec_gcm_open_messages", "ec_gcm_messages_stats"):
        assert name in _native.SIGNATURES
        assert hasattr(native, name)
    ptr = (ctypes.c_void_p * 1)(16)
    one = (ctypes.c_size_t * 1)(1)
    bad = _native.EC_ERR_INVALID_ARG
    # no context: before anything else, whatever the other arguments are
    assert native.ec_gcm_seal_messages(None, 1, ptr, one, 16, 16, ptr, None) == bad
    assert native.ec_gcm_seal_messages(None, 0, None, None, None, None, None, None) == bad
    assert native.ec_gcm_open_messages(None, 1, ptr, one, 16, 16, ptr, 16, None) == bad
    assert native.ec_gcm_open_messages(None, 1, None, None, None, None, None, None, None) == bad
    assert native.ec_gcm_messages_stats(None, None, None, None, None) == bad
    with open(_native.HEADER) as fh:
        text = fh.read()
    for want in ("ec_gcm_seal_messages(", "ec_gcm_open_messages(", "ec_gcm_messages_stats(", "const uint8_t *dev_keys32",
                 "splitter.go:189", "store.go:360-375", "splitter.go:160", "ec_gcm_open_messages below"):
        assert want in text, want


def test_binding_rejects_mismatched_lists():
    class S:
        ctx = None

    s = S()
    for bufs, lens, outs in (([16, 16], [1], [32]), ([16], [1, 1], [32]), ([16], [1], [32, 48]), ([16], [-1], [32]),
                             ([], [1], [])):
        with pytest.raises(ValueError):
            encryption.seal_messages(s, bufs, lens, 16, 16, outs)
        with pytest.raises(ValueError):
            encryption.open_messages(s, bufs, lens, 16, 16, outs, 16)


def test_mirrors_follow_the_empty_and_short_rules_without_a_device():
    key, nonce = bytes(32), bytes(24)
    assert encryption.encrypt(b"", key, nonce) == b"" and encryption.decrypt(b"", key, nonce) == b""
    for short in (b"x", bytes(15)):
        with pytest.raises(encryption.DecryptionFailed) as e:
            encryption.decrypt(short, key, nonce)
        assert e.value.block == 0
    with pytest.raises(ValueError):
        encryption.encrypt_key(bytes(31), key, nonce)
    with pytest.raises(ValueError):
        encryption.encrypt(b"data", bytes(16), nonce)


def _build(tmp_path, name):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    binary = str(tmp_path / name)
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "uplink_amd", "csrc"), "-o", binary,
                         os.path.join(HERE, "c", name + ".cpp")], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    return binary


def test_arithmetic_under_the_sanitizers(tmp_path, oracle):
    """tests/c/gcm_msg_host_test.cpp: the kernel's arithmetic with the 64 lanes played in a loop,
    with each form of the multiply, seals and opens the three no-AAD AES-256 cases of the GCM
    specification (plaintexts of 0, 16 and 64 bytes) and a message of every boundary length
    (messages_checked_child.BOUNDARY_LENGTHS) sealed by oracle.aesgcm; a wrong key expansion,
    multiply or lane combination shows here."""
    import numpy as np

    from messages_checked_child import BOUNDARY_LENGTHS, spec_cases
    from oracle import aesgcm as ag

    binary = _build(tmp_path, "gcm_msg_host_test")
    rng = np.random.default_rng(20261027)
    cases = spec_cases()
    for n in BOUNDARY_LENGTHS:
        key = rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
        nonce = rng.integers(0, 256, 12, dtype=np.uint8).tobytes()
        plain = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        cases.append((key, nonce, plain, bytes(ag.seal(key, nonce, plain))))
    path = tmp_path / "messages.txt"
    path.write_text("".join(f"{k.hex()} {n.hex()} {p.hex() or '-'} {s.hex()}\n" for k, n, p, s in cases))
    r = subprocess.run([binary, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == f"ok {len(cases)}" and not r.stderr.strip(), r.stdout + r.stderr


def test_geometry_under_the_sanitizers(tmp_path):
    """tests/c/gcm_msg_geom_test.cpp: slots, rounds, front padding, live lanes and combine steps
    of every length 0 .. 5000 and the boundaries up to 1 << 24; the pass split at pass_messages
    and one either side; every message of a pass with exactly one (workgroup, wave)."""
    binary = _build(tmp_path, "gcm_msg_geom_test")
    r = subprocess.run([binary], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "ok" and not r.stderr.strip(), r.stdout + r.stderr
