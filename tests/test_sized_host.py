"""Host side of the sized share-set calls (ec_rebuild_segments_sized,
ec_decode_segments_sized, uplink_amd/downloads.py): the download geometry of
GetWithOptions, the exports' binding, and the pure geometry header
(uplink_amd/csrc/sized_geom.hpp) under the sanitizers.  No device needed."""
import ctypes
import os
import shutil
import subprocess

import pytest

from uplink_amd import _native, downloads, ecclient, eestream

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


class _Scheme:
    """Duck-typed ErasureScheme (sizes only)."""

    def __init__(self, k, n, ess):
        self.k, self.n, self.ess = k, n, ess

    def total_count(self):
        return self.n

    def required_count(self):
        return self.k

    def erasure_share_size(self):
        return self.ess

    def stripe_size(self):
        return self.k * self.ess


@pytest.mark.parametrize("k,n,ess", [(29, 80, 256), (20, 60, 4096), (4, 10, 64), (2, 4, 8)])
def test_segment_geometry_follows_get_with_options(k, n, ess):
    es = _Scheme(k, n, ess)
    stripe = k * ess
    sizes = [0, 1, stripe - 1, stripe, stripe + 1, 2 * stripe, 7 * stripe - 4, 7 * stripe - 3, 300000, 67254016]
    for size in sizes:
        padded, piece, nstripes = downloads.segment_geometry(size, es)
        assert padded == ecclient.calc_padded(size, stripe), size
        assert padded % stripe == 0 and 0 <= padded - size < stripe
        assert piece * k == padded and piece == nstripes * ess
        # the upload side's piece size (CalcPieceSize pads size + 4 bytes of trailer): the
        # same piece when the download's size is the padded plaintext's, as uplink passes it
        if size >= 4:
            assert eestream.calc_piece_size(size - 4, es) == piece, size
    with pytest.raises(ValueError):
        downloads.segment_geometry(-1, es)


def test_segment_geometry_table():
    es = _Scheme(29, 80, 256)  # stripe 7424
    table = {0: (0, 0, 0), 1: (7424, 256, 1), 7423: (7424, 256, 1), 7424: (7424, 256, 1), 7425: (14848, 512, 2),
             300000: (304384, 10496, 41), 67254016: (67254016, 2319104, 9059)}
    for size, want in table.items():
        assert downloads.segment_geometry(size, es) == want, size
    # the production segment: 67,254,016 bytes are 9059 stripes exactly; PadReader's 4-byte
    # trailer makes the upload 9060 stripes (CalcPieceSize), and that padded size is what
    # its download is sized from
    assert eestream.calc_piece_size(67254016, es) == 9060 * 256
    assert downloads.segment_geometry(67254016 + 4, es) == (9060 * 7424, 9060 * 256, 9060)
    assert downloads.segment_geometry(9060 * 7424, es) == (9060 * 7424, 9060 * 256, 9060)


def test_exports_exist_and_reject_a_null_context(native):
    for name in ("ec_rebuild_segments_sized", "ec_decode_segments_sized"):
        assert name in _native.SIGNATURES
        assert hasattr(native, name)
    one = (ctypes.c_int * 1)(1)
    ptr = (ctypes.c_void_p * 1)(16)
    st = (ctypes.c_size_t * 1)(1)
    rc = (ctypes.c_int * 1)(5)
    assert native.ec_rebuild_segments_sized(None, 1, one, one, ptr, st, ptr, None) == _native.EC_ERR_INVALID_ARG
    assert native.ec_decode_segments_sized(None, 1, one, one, ptr, st, ptr, rc, None) == _native.EC_ERR_INVALID_ARG
    assert native.ec_rebuild_segments_sized(None, 0, None, None, None, None, None, None) == _native.EC_ERR_INVALID_ARG
    assert rc[0] == 5
    with open(_native.HEADER) as fh:
        text = fh.read()
    assert "ec_rebuild_segments_sized(" in text and "ec_decode_segments_sized(" in text


def test_codec_rejects_mismatched_lists():
    class S:
        ctx = None
        _lib = None

    codec = eestream.SegmentCodec(S())
    with pytest.raises(ValueError):
        codec.rebuild_segments_sized([([1], [16])], [1, 2], [32])
    with pytest.raises(ValueError):
        codec.rebuild_segments_sized([([1], [16])], [-1], [32])
    with pytest.raises(ValueError):
        codec.decode_segments_sized([([1, 2], [16])], [1], [32])


def test_sized_geom_under_the_sanitizers(tmp_path):
    """tests/c/sized_geom_test.cpp: a stand-alone program over sized_geom.hpp
    (tile bases, the part split at a synthetic grid limit, the pass split, the
    32-bit chunk limit), compiled with the host compiler and
    -fsanitize=address,undefined, run directly."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    binary = str(tmp_path / "sized_geom_test")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "uplink_amd", "csrc"), "-o", binary,
                         os.path.join(HERE, "c", "sized_geom_test.cpp")], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    r = subprocess.run([binary], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "ok" and not r.stderr.strip(), r.stdout + r.stderr
