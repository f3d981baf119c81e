"""Which share lists the six share-set exports refuse, and with which code
(include/uplink_ec.h ec_rebuild_segments_sets / _sized, ec_decode_segments_sets
/ _sized, ec_repair_segments_sets / _sized): the cases the other suites leave
out.  RS(4,10), ess 16, two stripes, two segments per call, the first valid.
Rebuild and Decode: code and bytes are the oracle's (rebuild / decode; but a
Decode list with an out-of-range number, which the header's code stands for).  Repair:
the code the header documents -- the basis is Rebuild's choice, every share of
the list is validated -- and the oracle's encoded pieces.  A refused call writes
nothing: every output window and guard still holds the marker.

Asserted elsewhere already, and so not here: too few shares, an out-of-range
number among the picked and a number picked twice in test_sized.py (Rebuild; for
Decode the out-of-range number is an unpicked one), test_repair.py and
test_repair_sized.py."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from uplink_amd import _native as N  # noqa: E402

pytestmark = pytest.mark.gpu

K, NN, ESS, STRIPES = 4, 10, 16, 2
PLEN, SEG = STRIPES * ESS, STRIPES * K * ESS
GUARD, MARK = 64, 0xCD
CODE = {-10: N.EC_ERR_NOT_ENOUGH_SHARES, -11: N.EC_ERR_INVALID_SHARE, -12: N.EC_ERR_SINGULAR,
        -13: N.EC_ERR_TOO_MANY_ERRORS}
FIRST = ([9, 0, 5, 2, 7], [1, 3])  # the valid first segment: its shares, its repair targets
# The second segment's lists per case: (numbers, position of an unpicked share that holds other
# bytes than its number's piece, repair targets).  With k = 4 the pick takes 0, 1, 2, 3 from the
# front of the sorted list while they are there and the rest from its back.
CASES = {
    "invalid_picked": [([0, 1, 2, 10], None, [5, 6]), ([-1, 1, 2, 3], None, [5, 6])],
    "invalid_unpicked": [([0, 1, 2, 3, 10], None, [5, 6]), ([3, -1, 0, 2, 1], None, [5, 6])],
    "picked_twice": [([5, 6, 7, 7], None, [0, 1]), ([6, 6, 5, 5, 0], None, [1, 2])],
    "repeat_unpicked": [([0, 1, 2, 3, 3], 4, [5, 6]), ([9, 9, 1, 0, 2], 0, [5, 6])],
    "too_few": [([5, 6, 7], None, [0, 1])],
}
REPAIR_WANT = {"invalid_picked": N.EC_ERR_INVALID_SHARE, "invalid_unpicked": N.EC_ERR_INVALID_SHARE,
               "picked_twice": N.EC_ERR_SINGULAR, "repeat_unpicked": N.EC_OK, "too_few": N.EC_ERR_NOT_ENOUGH_SHARES}
EXPORTS = ["rebuild_sets", "rebuild_sized", "decode_sets", "decode_sized", "repair_sets", "repair_sized"]
ELSEWHERE = {(e, c) for e in ("rebuild_sized", "repair_sets", "repair_sized")
             for c in ("too_few", "invalid_picked", "picked_twice")} | \
            {("decode_sized", c) for c in ("too_few", "invalid_unpicked", "picked_twice")}


@pytest.fixture(scope="module")
def world(oracle):
    """two random segments, their pieces by the oracle (host and device), a piece of other bytes,
    one context; shared by the tests and left unchanged"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    rng = np.random.default_rng(410)
    f = oracle.FEC(K, NN)
    segs = [rng.integers(0, 256, SEG, dtype=np.uint8) for _ in range(2)]
    refs = [f.encode_segment(s, ESS) for s in segs]
    junk = rng.integers(0, 256, PLEN, dtype=np.uint8)
    L = N.load()
    ctx = ctypes.c_void_p()
    assert L.ec_create(K, NN, ESS, ctypes.byref(ctx)) == 0
    yield dict(f=f, segs=segs, refs=refs, junk=junk, d=[torch.tensor(r).cuda() for r in refs],
               d_junk=torch.tensor(junk).cuda(), L=L, ctx=ctx, oracle=oracle)
    torch.cuda.synchronize()
    L.ec_destroy(ctx)


class Windows:
    """one marker-filled device buffer with `count` windows of `size` bytes, guards around each"""

    def __init__(self, count, size):
        self.size = size
        self.buf = torch.full((GUARD + count * (size + GUARD),), MARK, dtype=torch.uint8, device="cuda")
        self.ptrs = [self.buf.data_ptr() + GUARD + i * (size + GUARD) for i in range(count)]

    def check(self, contents):
        want = np.full(self.buf.numel(), MARK, dtype=np.uint8)
        for i, b in enumerate(contents):
            if b is not None:
                want[GUARD + i * (self.size + GUARD):][:self.size] = b
        got = self.buf.cpu().numpy()
        assert np.array_equal(got, want), f"first difference at byte {int(np.flatnonzero(got != want)[0])}"


def call(w, export, lists, targets, junk_at, flags=0):
    """the export over the two segments; segment 1's share at list position junk_at points at the
    other bytes.  Returns (rc, windows, status or None)."""
    L, ctx = w["L"], w["ctx"]
    flat = [x for nums in lists for x in nums]
    ptrs = [(w["d_junk"] if (g, i) == (1, junk_at) else w["d"][g][min(max(x, 0), NN - 1)]).data_ptr()
            for g, nums in enumerate(lists) for i, x in enumerate(nums)]
    a_ns = (ctypes.c_int * 2)(*[len(nums) for nums in lists])
    a_nums = (ctypes.c_int * len(flat))(*flat)
    a_ptrs = (ctypes.c_void_p * len(flat))(*ptrs)
    a_st = (ctypes.c_size_t * 2)(STRIPES, STRIPES)
    stream = torch.cuda.current_stream().cuda_stream
    kind, shape = export.split("_")
    status = None
    if kind == "repair":
        tflat = [t for ts in targets for t in ts]
        win = Windows(len(tflat), PLEN)
        status = torch.full((2,), 77, dtype=torch.int32, device="cuda") if flags else None
        rc = getattr(L, f"ec_repair_segments_{shape}")(
            ctx, 2, a_ns, a_nums, a_ptrs, (ctypes.c_int * 2)(*[len(ts) for ts in targets]),
            (ctypes.c_int * len(tflat))(*tflat), (ctypes.c_void_p * len(tflat))(*win.ptrs),
            a_st if shape == "sized" else STRIPES, flags, status.data_ptr() if flags else None, stream)
    else:
        win = Windows(2, SEG)
        args = [ctx, 2, a_ns, a_nums, a_ptrs, a_st if shape == "sized" else STRIPES,
                (ctypes.c_void_p * 2)(*win.ptrs)]
        if export == "decode_sized":
            args.append(None)
        rc = getattr(L, f"ec_{kind}_segments_{shape}")(*args, stream)
    torch.cuda.synchronize()
    return rc, win, status


def oracle_outcome(w, decode, nums, junk_at):
    """(EC code, the segment stripe-major or None) of the oracle's Rebuild / Decode of segment 1's list.
    A Decode list with a number out of range is not put to the oracle, whose Correct indexes its
    matrix by every number it is given: the header's code for it is the expected one (Decode
    checks all shares, as infectious' Correct does)."""
    if decode and any(x < 0 or x >= NN for x in nums):
        return N.EC_ERR_INVALID_SHARE, None
    datas =[w["junk"] if i == junk_at else w["refs"][1][min(max(x, 0), NN - 1)] for i, x in enumerate(nums)]
    try:
        out = w["f"].decode(nums, datas) if decode else w["f"].rebuild(nums, datas)
    except w["oracle"].OracleError as e:
        return CODE[e.code], None
    return N.EC_OK, np.ascontiguousarray(out.reshape(K, STRIPES, ESS).transpose(1, 0, 2)).reshape(-1)


@pytest.mark.parametrize("export,case", [(e, c) for e in EXPORTS for c in CASES if (e, c) not in ELSEWHERE])
def test_second_segment_refused_or_not(world, export, case):
    w = world
    kind = export.split("_")[0]
    for nums, junk_at, targets in CASES[case]:
        if kind == "decode":
            junk_at = None  # (Decode compares every share: a clean list, both copies the piece)
        lists, tg = [FIRST[0], nums], [FIRST[1], targets]
        if kind == "repair":
            want = REPAIR_WANT[case]
            contents = [w["refs"][g][t] for g in range(2) for t in tg[g]]
        else:
            want, seg1 = oracle_outcome(w, kind == "decode", nums, junk_at)
            contents = [w["segs"][0], seg1]
        if case == "invalid_unpicked":
            assert want == (N.EC_OK if kind == "rebuild" else N.EC_ERR_INVALID_SHARE)
        elif case == "repeat_unpicked":
            assert want == N.EC_OK
        else:
            assert want != N.EC_OK
        rc, win, _ = call(w, export, lists, tg, junk_at)
        print(export, case, nums, "rc", rc, "want", want)
        assert rc == want, (nums, N.strerror(rc), N.strerror(want))
        win.check(contents if want == N.EC_OK else [None] * len(contents))
        if kind == "repair" and want == N.EC_OK:
            # with the share check the unpicked copy is compared with the picked one
            for j, flagged in ((junk_at, 1), (None, 0)):
                rc, win, status = call(w, export, lists, tg, j, flags=N.EC_FLAG_CHECK_SHARES)
                assert rc == N.EC_OK and status.tolist() == [0, flagged], (nums, rc, status.tolist())
                if not flagged:
                    win.check(contents)
    for g in range(2):
        assert np.array_equal(w["d"][g].cpu().numpy(), w["refs"][g]), "a piece was written"
    assert np.array_equal(w["d_junk"].cpu().numpy(), w["junk"])
