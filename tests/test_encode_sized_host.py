"""Host side of the sized encode (ec_encode_segments_sized, uplink_amd/uploads.py):
the upload geometry of PadReader, the export's binding, and the pure geometry
header (uplink_amd/csrc/enc_sized_geom.hpp) under the sanitizers.  No device needed."""
import ctypes
import os
import shutil
import subprocess

import pytest

from uplink_amd import _native, eestream, pipeline, uploads

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


@pytest.mark.parametrize("k,n,ess", [(29, 80, 256), (20, 60, 4096), (4, 10, 64), (2, 4, 16)])
def test_upload_geometry_follows_pad_reader(k, n, ess):
    es = _Scheme(k, n, ess)
    stripe = k * ess
    sizes = [1, stripe - 5, stripe - 4, stripe - 3, stripe, 3 * stripe + 17, 0, 7419, 7420, 100000]
    for size in sizes:
        padded, piece, nstripes = uploads.upload_geometry(size, es)
        assert padded == pipeline._pad_len(size, stripe), size
        assert padded % stripe == 0 and 4 <= padded - size <= stripe + 3
        assert piece * k == padded and piece == nstripes * ess
        assert eestream.calc_piece_size(size, es) == piece, size
    with pytest.raises(ValueError):
        uploads.upload_geometry(-1, es)


def test_upload_geometry_table():
    es = _Scheme(29, 80, 256)  # stripe 7424
    table = {0: (7424, 256, 1), 1: (7424, 256, 1), 7419: (7424, 256, 1), 7420: (7424, 256, 1), 7421: (14848, 512, 2),
             7424: (14848, 512, 2), 22289: (29696, 1024, 4), 100000: (103936, 3584, 14),
             67254016: (9060 * 7424, 9060 * 256, 9060)}
    for size, want in table.items():
        assert uploads.upload_geometry(size, es) == want, size


def test_export_exists_and_rejects_null_arguments(native):
    assert "ec_encode_segments_sized" in _native.SIGNATURES
    assert hasattr(native, "ec_encode_segments_sized")
    ptr = (ctypes.c_void_p * 1)(16)
    st = (ctypes.c_size_t * 1)(1)
    assert native.ec_encode_segments_sized(None, 1, ptr, st, None, ptr, 0, None) == _native.EC_ERR_INVALID_ARG
    assert native.ec_encode_segments_sized(None, 0, None, None, None, None, 0, None) == _native.EC_ERR_INVALID_ARG
    with open(_native.HEADER) as fh:
        text = fh.read()
    assert "ec_encode_segments_sized(" in text and "single.go:233-238" in text and "encode.go:39-75" in text


def test_codec_rejects_mismatched_lists():
    class S:
        ctx = None
        _lib = None

    codec = eestream.SegmentCodec(S())
    with pytest.raises(ValueError):
        codec.encode_segments_sized([16], [1, 2], [32])
    with pytest.raises(ValueError):
        codec.encode_segments_sized([16], [1], [32, 48])
    with pytest.raises(ValueError):
        codec.encode_segments_sized([16], [-1], [32])
    with pytest.raises(ValueError):
        codec.encode_segments_sized([16], [1], [32], data_len=[1, 2])


def test_enc_sized_geom_under_the_sanitizers(tmp_path):
    """tests/c/encode_sized_geom_test.cpp: a stand-alone program over enc_sized_geom.hpp
    (blocks per segment and first blocks, the pair count for odd and even totals, the pad
    amount and its validation at the stripe boundaries, the pass split at 1024 segments),
    compiled with the host compiler and -fsanitize=address,undefined, run directly."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    binary = str(tmp_path / "encode_sized_geom_test")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "uplink_amd", "csrc"), "-o", binary,
                         os.path.join(HERE, "c", "encode_sized_geom_test.cpp")], capture_output=True, text=True,
                        timeout=300)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    r = subprocess.run([binary], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "ok" and not r.stderr.strip(), r.stdout + r.stderr
