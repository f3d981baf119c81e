"""Host side of segment repair with a size per segment
(ec_repair_segments_sized, uplink_amd/repair.py repair_segments_sized): the
export's binding, the argument errors raised before any engine call, and the
geometry its passes are laid out with under the sanitizers.  No device needed."""
import ctypes
import os
import shutil
import subprocess

import pytest

from uplink_amd import _native, eestream, repair

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_export_exists_and_rejects_a_null_context(native):
    assert "ec_repair_segments_sized" in _native.SIGNATURES
    assert hasattr(native, "ec_repair_segments_sized")
    restype, argtypes = _native.SIGNATURES["ec_repair_segments_sized"]
    sets = _native.SIGNATURES["ec_repair_segments_sets"][1]
    # ec_repair_segments_sets with a pointer to size_t where that call takes one size_t
    assert restype is ctypes.c_int and len(argtypes) == len(sets) == 12
    assert argtypes[8] is ctypes.POINTER(ctypes.c_size_t) and sets[8] is ctypes.c_size_t
    assert [a for i, a in enumerate(argtypes) if i != 8] == [a for i, a in enumerate(sets) if i != 8]
    one = (ctypes.c_int * 1)(1)
    ptr = (ctypes.c_void_p * 1)(16)
    st = (ctypes.c_size_t * 1)(1)
    assert native.ec_repair_segments_sized(None, 1, one, one, ptr, one, one, ptr, st, 0, None, None) == \
        _native.EC_ERR_INVALID_ARG
    assert native.ec_repair_segments_sized(None, 0, None, None, None, None, None, None, None, 0, None, None) == \
        _native.EC_ERR_INVALID_ARG
    with open(_native.HEADER) as fh:
        text = fh.read()
    assert "ec_repair_segments_sized(" in text


def test_raw_call_rejects_mismatched_lists():
    with pytest.raises(ValueError):
        repair.repair_call_sized(None, [([1, 2], [16], [3])], [32], [1])
    with pytest.raises(ValueError):
        repair.repair_call_sized(None, [([1], [16], [3, 4])], [32], [1])
    with pytest.raises(ValueError):
        repair.repair_call_sized(None, [([1], [16], [3])], [32], [1, 2])  # a stripe count too many
    with pytest.raises(ValueError):
        repair.repair_call_sized(None, [([1], [16], [3])], [32], [-1])


class _Scheme:
    """Duck-typed ErasureScheme without a context: any engine call would fail on it."""
    ctx = None

    def __init__(self, k, ess):
        self.k, self.ess = k, ess

    def erasure_share_size(self):
        return self.ess

    def required_count(self):
        return self.k


def test_piece_lengths_are_checked_before_any_engine_call():
    torch = pytest.importorskip("torch")
    es = _Scheme(2, 64)

    def piece(nbytes):
        return torch.zeros(nbytes, dtype=torch.uint8)

    ok = ([0, 1], [piece(128), piece(128)], [2])
    # lengths that differ within one segment
    with pytest.raises(eestream.InfectiousError) as ei:
        repair.repair_segments_sized(es, [ok, ([0, 1], [piece(64), piece(128)], [3])])
    assert ei.value.code == _native.EC_ERR_SHARE_SIZE
    # a length that is no multiple of the share size
    with pytest.raises(eestream.InfectiousError) as ei:
        repair.repair_segments_sized(es, [ok, ([0, 1], [piece(96), piece(96)], [3])])
    assert ei.value.code == _native.EC_ERR_INVALID_ARG
    with pytest.raises(eestream.InfectiousError) as ei:
        repair.repair_segments_sized(_Scheme(2, 0), [ok])
    assert ei.value.code == _native.EC_ERR_INVALID_ARG
    with pytest.raises(ValueError):
        repair.repair_segments_sized(es, [([0, 1, 2], [piece(64), piece(64)], [3])])
    # nothing to repair
    assert repair.repair_segments_sized(es, []) == []
    assert repair.repair_segments_sized(es, [], hash_pieces=True) == ([], [])


def test_repairer_has_the_sized_form():
    assert callable(repair.SegmentRepairer.repair_sized)


def test_repair_sized_geom_under_the_sanitizers(tmp_path):
    """tests/c/repair_sized_geom_test.cpp: a stand-alone program over
    sized_geom.hpp and rs_rows.hpp's share_max_tiles with the 8-wave class
    present (every tile of every segment in exactly one launch under its own map
    entry, a class cut at a small fake launch limit, classes in mixed order, the
    pass split), compiled with the host compiler and
    -fsanitize=address,undefined, run directly."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    binary = str(tmp_path / "repair_sized_geom_test")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "uplink_amd", "csrc"), "-o", binary,
                         os.path.join(HERE, "c", "repair_sized_geom_test.cpp")],
                        capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    r = subprocess.run([binary], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "ok" and not r.stderr.strip(), r.stdout + r.stderr
