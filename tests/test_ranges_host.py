"""Host side of ranged downloads (ec_gcm_open_ranges_sized; uplink_amd/downloads.py
range_geometry, object_ranges): the exports and their binding, the pure geometry
header (uplink_amd/csrc/range_geom.hpp) under the sanitizers, and the Python
mirror against a definitional model in numpy and against
streams.calc_encompassing_blocks.  No device needed."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from uplink_amd import _native, downloads, encryption, streams

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


class Scheme:
    def __init__(self, k, ess):
        self.k, self.ess = k, ess

    def required_count(self):
        return self.k

    def erasure_share_size(self):
        return self.ess

    def stripe_size(self):
        return self.k * self.ess


def test_exports_exist_and_reject_null_arguments(native):
    for name in ("ec_gcm_open_ranges_sized", "ec_gcm_ranged_stats"):
        assert name in _native.SIGNATURES
        assert hasattr(native, name)
    ptr = (ctypes.c_void_p * 1)(16)
    one = (ctypes.c_size_t * 1)(1)
    zero = (ctypes.c_size_t * 1)(0)
    bad = _native.EC_ERR_INVALID_ARG
    # no context: before anything else, whatever the other arguments are
    assert native.ec_gcm_open_ranges_sized(None, 1, ptr, zero, one, zero, one, 16, 16, 16, ptr, 16, None) == bad
    assert native.ec_gcm_open_ranges_sized(None, 0, None, None, None, None, None, 16, None, None, None, None, None) == bad
    assert native.ec_gcm_open_ranges_sized(None, 1, None, None, None, None, None, 16, None, None, None, None, None) == bad
    assert native.ec_gcm_ranged_stats(None, None, None) == bad
    with open(_native.HEADER) as fh:
        text = fh.read()
    for want in ("ec_gcm_open_ranges_sized(", "ec_gcm_ranged_stats(", "const size_t *first_block",
                 "eestream/decode.go:199-227", "store.go:360-375"):
        assert want in text, want


def test_binding_rejects_mismatched_lists():
    class S:
        ctx = None

    s = S()
    ok = dict(ciphers=[16], first_block=[0], nblocks=[1], head=[0], length=[1], outs=[32])
    for name, v in (("ciphers", [16, 16]), ("outs", [32, 48]), ("nblocks", [1, 2]), ("nblocks", [-1]),
                    ("first_block", [0, 0]), ("first_block", [-1]), ("head", []), ("head", [-1]),
                    ("length", [1, 1]), ("length", [-1])):
        a = dict(ok, **{name: v})
        with pytest.raises(ValueError):
            encryption.open_ranges_sized(s, a["ciphers"], a["first_block"], a["nblocks"], a["head"], a["length"], 16,
                                         16, 16, a["outs"], 16)


def test_range_geom_under_the_sanitizers(tmp_path):
    """tests/c/range_geom_test.cpp: a stand-alone program over range_geom.hpp (every (offset,
    length) of plaintexts of 0 .. 160 bytes at in_block 16, 32 and 48 under (k, ess) (2,8), (3,8)
    and (4,16) against the definitional minimal cover; the worked example; the overflow and
    0x7FFFFFFF edges; the call's (head, length, nblocks) rule), compiled with the host compiler
    and -fsanitize=address,undefined, run directly."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    binary = str(tmp_path / "range_geom_test")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "uplink_amd", "csrc"), "-o", binary,
                         os.path.join(HERE, "c", "range_geom_test.cpp")], capture_output=True, text=True,
                        timeout=300)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    r = subprocess.run([binary], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "ok" and not r.stderr.strip(), r.stdout + r.stderr


def _model(P, off, length, ib, k, ess):
    """the minimal cover by definition: the blocks that hold a wanted plaintext byte, the
    encrypted bytes of those blocks, the stripes that hold any of them"""
    B, S = ib + 16, k * ess
    nblk = P // ib + 1
    want = np.zeros(nblk * ib, dtype=bool)
    want[off:off + length] = True
    blocks = np.flatnonzero(want.reshape(nblk, ib).any(axis=1))
    enc = np.zeros((nblk, B), dtype=bool)
    enc[blocks] = True
    enc = enc.reshape(-1)
    nstr = -(-len(enc) // S)
    stripes = np.flatnonzero(np.pad(enc, (0, nstr * S - len(enc))).reshape(nstr, S).any(axis=1))
    return blocks, stripes


@pytest.mark.parametrize("ib,k,ess", [(16, 2, 8), (32, 3, 8), (48, 4, 16), (16, 4, 16)])
def test_range_geometry_is_the_minimal_cover(ib, k, ess):
    es = Scheme(k, ess)
    B, S = ib + 16, k * ess
    for P in (0, 1, 47, 96, 131):
        for off in range(P + 1):
            for length in range(P - off + 1):
                g = downloads.range_geometry(P, off, length, es, B)
                blocks, stripes = _model(P, off, length, ib, k, ess)
                assert (g.plain_size, g.offset, g.length) == (P, off, length)
                assert g.nblocks == len(blocks) and g.nstripes == len(stripes)
                if length:
                    assert g.first_block == blocks[0] and blocks[-1] - blocks[0] + 1 == len(blocks)
                    assert g.first_stripe == stripes[0] and stripes[-1] - stripes[0] + 1 == len(stripes)
                assert g.head == off - g.first_block * ib and 0 <= g.head < ib
                assert g.enc_offset == g.first_block * B and g.enc_length == g.nblocks * B
                assert g.skip == g.enc_offset - g.first_stripe * S and 0 <= g.skip < S
                assert (g.piece_offset, g.piece_length) == (g.first_stripe * ess, g.nstripes * ess)
                assert (g.first_block, g.nblocks) == streams.calc_encompassing_blocks(off, length, ib)
                assert (g.first_stripe, g.nstripes) == streams.calc_encompassing_blocks(g.enc_offset, g.enc_length, S)


def test_range_geometry_worked_example_and_errors():
    es = Scheme(29, 256)
    g = downloads.range_geometry(67108864, 10_000_000, 1_048_576, es)
    assert (g.first_block, g.head, g.nblocks, g.enc_offset) == (1349, 6608, 143, 10_014_976)
    assert (g.first_stripe, g.nstripes, g.skip) == (1349, 143, 0)
    assert (g.piece_offset, g.piece_length) == (345_344, 36_608)
    assert 29 * g.piece_length == 1_061_632
    # RS(3,7), ess 8, block 32: skip cycles through 0, 8, 16
    assert [downloads.range_geometry(1000, 16 * b, 16, Scheme(3, 8), 32).skip for b in range(6)] == [0, 8, 16, 0, 8, 16]
    for P, off, length in ((100, 101, 0), (100, 50, 51), (100, -1, 1), (100, 0, -1), (-1, 0, 0), (1 << 64, 0, 1)):
        with pytest.raises(ValueError):
            downloads.range_geometry(P, off, length, es)
    assert downloads.range_geometry(100, 100, 0, es).nblocks == 0
    for bs in (16, 40, (1 << 24) + 32):
        with pytest.raises(ValueError):
            downloads.range_geometry(100, 0, 1, es, bs)
    top = 0x7FFFFFFF * 16
    small = Scheme(2, 8)
    assert downloads.range_geometry(top + 16, top - 16, 16, small, 32).first_block == 0x7FFFFFFE
    assert downloads.range_geometry(top + 16, 0, top, small, 32).nblocks == 0x7FFFFFFF
    for off, length in ((top - 16, 17), (top, 1), (0, top + 1)):
        with pytest.raises(ValueError):
            downloads.range_geometry(top + 16, off, length, small, 32)


def test_object_ranges_against_slicing_a_concatenation():
    rng = np.random.default_rng(3)
    for sizes in ([5, 0, 7, 1, 12], [10], [0, 0, 3], []):
        segs = [rng.integers(0, 256, s, dtype=np.uint8) for s in sizes]
        whole = np.concatenate(segs) if segs else np.zeros(0, np.uint8)
        total = len(whole)
        for off in range(total + 1):
            for length in range(total - off + 1):
                tr = downloads.object_ranges(sizes, off, length)
                assert all(n > 0 and 0 <= o and o + n <= sizes[i] for i, o, n in tr)
                assert [i for i, _, _ in tr] == sorted({i for i, _, _ in tr})  # in order, each segment once
                got = np.concatenate([segs[i][o:o + n] for i, o, n in tr]) if tr else np.zeros(0, np.uint8)
                assert np.array_equal(got, whole[off:off + length]), (sizes, off, length)
                if length == 0:
                    assert tr == []
        for off, length in ((total + 1, 0), (0, total + 1), (total, 1), (-1, 1), (0, -1)):
            with pytest.raises(ValueError):
                downloads.object_ranges(sizes, off, length)
    assert downloads.object_ranges([5, 0, 7, 1, 12], 4, 10) == [(0, 4, 1), (2, 0, 7), (3, 0, 1), (4, 0, 1)]
    with pytest.raises(ValueError):
        downloads.object_ranges([5, -1], 0, 1)
