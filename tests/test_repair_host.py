"""Host logic of segment repair (uplink_amd/repair.py, ec_repair_segments_sets):
SegmentRepairer's target selection against RedundancyStrategy's thresholds, and
the argument validation that needs no device."""
import ctypes

import pytest

from uplink_amd import _native, eestream, repair


class _Scheme:
    """Duck-typed ErasureScheme (sizes only)."""

    def __init__(self, k, n, ess=256):
        self.k, self.n, self.ess = k, n, ess

    def total_count(self):
        return self.n

    def required_count(self):
        return self.k


def _repairer(k=29, rep=35, opt=65, n=80):
    return repair.SegmentRepairer(eestream.RedundancyStrategy(_Scheme(k, n), rep, opt))


@pytest.mark.parametrize("healthy,needs", [(29, True), (34, True), (35, True), (36, False), (64, False), (80, False)])
def test_targets_follow_the_repair_threshold(healthy, needs):
    """ecclient.put's rule (client.go:113-116): at most the repair threshold (and
    below the optimal threshold) is too few"""
    r = _repairer()
    have = list(range(3, 3 + healthy)) if healthy < 78 else list(range(healthy))
    assert r.needs_repair(have) == needs
    t = r.targets(have[::-1])
    if needs:
        assert t == [x for x in range(80) if x not in have]
        assert len(t) + healthy == 80
    else:
        assert t == []


def test_thresholds_at_the_total_count():
    """repair == optimal == total (RedundancyStrategy's defaults): only a complete
    segment is left alone, as put accepts only a full set of limits then"""
    r = repair.SegmentRepairer(eestream.RedundancyStrategy(_Scheme(2, 4)))
    assert r.targets([0, 1, 2, 3]) == []
    assert r.targets([3, 0, 2]) == [1]
    assert r.targets([1, 2]) == [0, 3]


def test_too_few_or_bad_healthy_pieces():
    r = _repairer()
    with pytest.raises(eestream.NotEnoughShares):
        r.targets(range(28))
    with pytest.raises(ValueError):
        r.targets(list(range(29)) + [3])
    with pytest.raises(ValueError):
        r.targets(list(range(29)) + [80])
    with pytest.raises(ValueError):
        r.targets([-1] + list(range(29)))


def test_binding_and_validation_without_a_device(native):
    assert _native.EC_FLAG_CHECK_SHARES == 0x4
    assert "ec_repair_segments_sets" in _native.SIGNATURES
    one = (ctypes.c_int * 1)(1)
    ptr = (ctypes.c_void_p * 1)(16)
    # no context
    assert native.ec_repair_segments_sets(None, 1, one, one, ptr, one, one, ptr, 1, 0, None, None) == \
        _native.EC_ERR_INVALID_ARG
    assert native.ec_repair_segments_sets(None, 0, None, None, None, None, None, None, 0, 0, None, None) == \
        _native.EC_ERR_INVALID_ARG
    with open(_native.HEADER) as fh:
        text = fh.read()
    assert "#define EC_FLAG_CHECK_SHARES 0x4" in text and "ec_repair_segments_sets(" in text


def test_flatten_rejects_mismatched_lists():
    with pytest.raises(ValueError):
        repair.repair_call(None, [([1, 2], [16], [3])], [32], 1)
    with pytest.raises(ValueError):
        repair.repair_call(None, [([1], [16], [3, 4])], [32], 1)
