"""GPU parity of segment repair (include/uplink_ec.h ec_repair_segments_sets,
uplink_amd/repair.py): the lost pieces of a batch of segments regenerated from
any k of the pieces each still has, a share set and a target set per segment.
Every expected piece is the oracle's encode_segment output, compared bit-exact;
outputs are carved out of 0xCD-filled buffers with guards, which must come back
untouched."""
import ctypes
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from uplink_amd import _native  # noqa: E402

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GUARD = 64
CHECK = _native.EC_FLAG_CHECK_SHARES


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)


class Ctx:
    def __init__(self, k, n, ess):
        self.L = _native.load()
        self.k, self.n, self.ess = k, n, ess
        self.ctx = ctypes.c_void_p()
        assert self.L.ec_create(k, n, ess, ctypes.byref(self.ctx)) == 0

    def close(self):
        torch.cuda.synchronize()
        self.L.ec_destroy(self.ctx)


def encode_all(oracle, k, n, ess, nseg, stripes, seed):
    """(segments, their pieces [nseg, n, plen] by the oracle)"""
    rng = np.random.default_rng(seed)
    f = oracle.FEC(k, n)
    segs = [rng.integers(0, 256, stripes * k * ess, dtype=np.uint8) for _ in range(nseg)]
    return segs, np.stack([f.encode_segment(s, ess, threads=8) for s in segs])


@pytest.fixture(scope="module")
def rs29(oracle):
    """RS(29,80), ess 256, 41 stripes (5.1 tiles: a ragged last tile), 12 segments: (ref pieces, the same on the device)"""
    _, ref = encode_all(oracle, 29, 80, 256, 12, 41, 2980)
    ref.setflags(write=False)
    return ref, torch.tensor(ref).cuda()  # (a copy: ref stays read-only)


def basis_of(nums, k):
    """indices into nums of the k shares infectious Rebuild chooses"""
    order = sorted(range(len(nums)), key=lambda i: nums[i])
    b, e, out = 0, len(nums) - 1, []
    for i in range(k):
        if nums[order[b]] == i:
            out.append(order[b])
            b += 1
        else:
            out.append(order[e])
            e -= 1
    return out


class Outs:
    """One 0xCD-filled device buffer with a piece-sized window per target, GUARD bytes before, between and after"""

    def __init__(self, targets, plen):
        self.plen = plen
        self.count = sum(len(t) for t in targets)
        self.buf = torch.full((GUARD + self.count * (plen + GUARD),), 0xCD, dtype=torch.uint8, device="cuda")
        self.ptrs = [self.buf.data_ptr() + GUARD + i * (plen + GUARD) for i in range(self.count)]

    def expect(self, pieces):
        """the whole buffer with window i holding pieces[i] (None: untouched)"""
        want = np.full(self.buf.numel(), 0xCD, dtype=np.uint8)
        for i, p in enumerate(pieces):
            if p is not None:
                o = GUARD + i * (self.plen + GUARD)
                want[o:o + self.plen] = p
        return want

    def check(self, pieces):
        got = self.buf.cpu().numpy()
        want = self.expect(pieces)
        if not np.array_equal(got, want):
            w = int(np.flatnonzero(got != want)[0])
            raise AssertionError(f"first difference at byte {w} (window {(w - GUARD) // (self.plen + GUARD)}, "
                                 f"offset {(w - GUARD) % (self.plen + GUARD)}): {got[w]:#x} != {want[w]:#x}")


def call_repair(c, d_pieces, sets, targets, stripes, outs=None, flags=0, status=None, stream=None, seg_of=None):
    """sets[g] / targets[g]: share and target numbers of segment g (its pieces: d_pieces[seg_of[g]])"""
    plen = stripes * c.ess
    nseg = len(sets)
    seg_of = seg_of or list(range(nseg))
    outs = outs or Outs(targets, plen)
    flat = [x for s in sets for x in s]
    tflat = [x for t in targets for x in t]
    rc = c.L.ec_repair_segments_sets(
        c.ctx, nseg, (ctypes.c_int * nseg)(*[len(s) for s in sets]), (ctypes.c_int * max(len(flat), 1))(*flat),
        (ctypes.c_void_p * max(len(flat), 1))(*[d_pieces[seg_of[g]][x].data_ptr() for g, s in enumerate(sets) for x in s]),
        (ctypes.c_int * nseg)(*[len(t) for t in targets]), (ctypes.c_int * max(len(tflat), 1))(*tflat),
        (ctypes.c_void_p * max(len(tflat), 1))(*outs.ptrs), stripes, flags,
        status.data_ptr() if status is not None else None, (stream or torch.cuda.current_stream()).cuda_stream)
    return rc, outs


def expected(ref, targets, seg_of=None):
    return [ref[(seg_of[g] if seg_of else g)][t] for g, ts in enumerate(targets) for t in ts]


def random_case(rng, k, n, count, extra=0):
    """a shuffled (k + extra)-subset and `count` shuffled targets among the other pieces"""
    perm = [int(x) for x in rng.permutation(n)]
    nums, rest = perm[:k + extra], perm[k + extra:]
    return nums, rest[:count]


def test_checked_library(native):
    """First, so that an access of the new kernel outside its segment's shares or
    outputs is skipped and reported by the bounds-checked build instead of
    reaching the card: a fresh process loads lib/checked/libuplink_ec_checked.so
    and runs the 41-stripe RS(29,80) case with 51 and with 3 targets and the
    share check.  The two libraries must be one build."""
    child = [sys.executable, os.path.join(HERE, "repair_checked_child.py")]
    r = subprocess.run(child + ["--build-id"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    ident = r.stdout.split("build", 1)[1].split()[0]
    assert ident == native.ec_build_id().decode(), f"checked library build {ident} is not the product's: rebuild both"
    r = subprocess.run(child, capture_output=True, text=True, timeout=240)
    assert "uplink_ec checked" not in r.stdout + r.stderr, r.stdout + r.stderr
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "ok"


def test_wave_class_boundaries(rs29):
    """12 segments in one call with 1 .. 51 targets: every wave-count class (2, 3,
    4 waves up to 14, 24, 32 rows; 8 waves above) and each side of every
    boundary.  All data present -> all parity; the all-parity basis 51..79 ->
    data and parity; seeded random 29-subsets; shares and targets unsorted; two
    segments with k + 5 shares (the surplus ignored)."""
    ref, d_pieces = rs29
    k, n, ess, stripes = 29, 80, 256, 41
    counts = [1, 8, 9, 14, 15, 24, 25, 32, 33, 45, 51, 51]
    rng = np.random.default_rng(51)
    sets, targets = [], []
    for g, cnt in enumerate(counts):
        if g == 10:
            nums, tg = list(range(k)), list(range(k, n))
        elif g == 11:
            nums, tg = list(range(51, 80))[::-1], [int(x) for x in rng.permutation(51)]
        else:
            nums, tg = random_case(rng, k, n, cnt, extra=5 if g in (1, 9) else 0)
        assert len(tg) == cnt
        sets.append(nums)
        targets.append(tg)
    c = Ctx(k, n, ess)
    try:
        rc, outs = call_repair(c, d_pieces, sets, targets, stripes)
        assert rc == 0, _native.strerror(rc)
        torch.cuda.synchronize()
        outs.check(expected(ref, targets))
        assert c.L.ec_last_body(c.ctx) == _native.EC_BODY_JUMP_TABLE
    finally:
        c.close()


@pytest.mark.parametrize("k,n,ess,stripes", [(29, 80, 256, 1), (29, 80, 256, 8), (29, 80, 256, 9), (1, 3, 256, 20),
                                             (2, 4, 256, 33), (4, 10, 16, 257), (50, 80, 256, 9)])
def test_tile_edges_and_small_codes(oracle, k, n, ess, stripes):
    """Less than a tile, exactly one (8 stripes of 256), one and a bit; codes with
    fewer inputs than a chunk holds (RS(1,3) is replication, RS(2,4)); ess 16; a
    wide code.  Per code: every other piece from the first k, from the last k,
    and random sets with 1 target and with all."""
    _, ref = encode_all(oracle, k, n, ess, 4, stripes, k * 1000 + stripes)
    d_pieces = torch.from_numpy(ref).cuda()
    rng = np.random.default_rng(stripes)
    sets = [list(range(k)), list(range(n - k, n))]
    targets = [list(range(k, n)), list(range(n - k))[::-1]]
    for cnt in (1, n - k):
        nums, tg = random_case(rng, k, n, cnt)
        sets.append(nums)
        targets.append(tg)
    c = Ctx(k, n, ess)
    try:
        rc, outs = call_repair(c, d_pieces, sets, targets, stripes)
        assert rc == 0, _native.strerror(rc)
        torch.cuda.synchronize()
        outs.check(expected(ref, targets))
    finally:
        c.close()


def test_engine_limit(oracle):
    """RS(128,256): 128 inputs and 128 targets, two passes of 64 rows on 8 waves"""
    k, n, ess, stripes = 128, 256, 256, 3
    _, ref = encode_all(oracle, k, n, ess, 2, stripes, 128256)
    d_pieces = torch.from_numpy(ref).cuda()
    rng = np.random.default_rng(128)
    sets = [list(range(128, 256)), None]
    targets = [list(range(128)), None]
    sets[1], targets[1] = random_case(rng, k, n, 128)
    c = Ctx(k, n, ess)
    try:
        rc, outs = call_repair(c, d_pieces, sets, targets, stripes)
        assert rc == 0, _native.strerror(rc)
        torch.cuda.synchronize()
        outs.check(expected(ref, targets))
    finally:
        c.close()


def test_byte_path(oracle, rs29):
    """What the bit-sliced kernel cannot take goes through the byte kernel with the
    same results: a share size that is no multiple of 16, and an aligned shape
    with one share pointer 8 bytes off."""
    k, n, ess, stripes = 29, 80, 24, 41
    _, ref = encode_all(oracle, k, n, ess, 2, stripes, 24)
    d_pieces = torch.from_numpy(ref).cuda()
    rng = np.random.default_rng(24)
    cases = [random_case(rng, k, n, 51), random_case(rng, k, n, 3)]
    sets, targets = [s for s, _ in cases], [t for _, t in cases]
    c = Ctx(k, n, ess)
    try:
        rc, outs = call_repair(c, d_pieces, sets, targets, stripes)
        assert rc == 0, _native.strerror(rc)
        torch.cuda.synchronize()
        outs.check(expected(ref, targets))
    finally:
        c.close()
    ref, d_ref = rs29
    ess, plen = 256, 41 * 256
    nums, tg = random_case(rng, k, n, 40)
    # segment 0 as it is; segment 1 the same with its third share copied to an address 8 bytes past alignment
    off = torch.full((plen + 32,), 0xEE, dtype=torch.uint8, device="cuda")
    shifted = off[8:8 + plen]
    assert shifted.data_ptr() % 16 == 8
    shifted.copy_(d_ref[1][nums[2]])
    pieces = [{x: d_ref[1][x] for x in nums}, {x: (shifted if x == nums[2] else d_ref[1][x]) for x in nums}]
    c = Ctx(k, n, ess)
    try:
        rc, outs = call_repair(c, pieces, [nums, nums], [tg, tg], 41)
        assert rc == 0, _native.strerror(rc)
        torch.cuda.synchronize()
        outs.check(expected(ref, [tg, tg], seg_of=[1, 1]))
    finally:
        c.close()


def _check_setup(rs29, rng):
    """four segments with k + 3 shares each, the shares copied into one buffer
    whose gaps hold 0xFF: (nums, targets, buffer, piece tensors per segment)"""
    ref, d_ref = rs29
    k, n, plen = 29, 80, 41 * 256
    cases = [random_case(rng, k, n, cnt, extra=3) for cnt in (5, 20, 48, 30)]
    sets, targets = [s for s, _ in cases], [t for _, t in cases]
    total = sum(len(s) for s in sets)
    buf = torch.full((GUARD + total * (plen + GUARD),), 0xFF, dtype=torch.uint8, device="cuda")
    pieces, i = [], 0
    for g, s in enumerate(sets):
        row = {}
        for x in s:
            o = GUARD + i * (plen + GUARD)
            row[x] = buf[o:o + plen]
            row[x].copy_(d_ref[g][x])
            i += 1
        pieces.append(row)
    return sets, targets, buf, pieces


def test_share_check(rs29):
    ref, _ = rs29
    k, stripes, plen = 29, 41, 41 * 256
    sets, targets, buf, pieces = _check_setup(rs29, np.random.default_rng(3))
    clean = buf.clone()
    c = Ctx(29, 80, 256)
    try:
        status = torch.full((4,), 0x55, dtype=torch.int32, device="cuda")
        rc, outs = call_repair(c, pieces, sets, targets, stripes, flags=CHECK, status=status)
        assert rc == 0, _native.strerror(rc)
        torch.cuda.synchronize()
        assert status.cpu().tolist() == [0, 0, 0, 0]
        outs.check(expected(ref, targets))
        # one byte in the last valid column of a surplus share of segment 1, one byte of a basis share of segment 3
        b1, b3 = basis_of(sets[1], k), basis_of(sets[3], k)
        surplus = [x for i, x in enumerate(sets[1]) if i not in b1]
        pieces[1][surplus[1]][plen - 1] ^= 0x01
        pieces[3][sets[3][b3[7]]][1234] ^= 0x80
        status.fill_(0x55)
        rc, outs = call_repair(c, pieces, sets, targets, stripes, flags=CHECK, status=status)
        assert rc == 0, _native.strerror(rc)
        torch.cuda.synchronize()
        assert status.cpu().tolist() == [0, 1, 0, 1]
        got = outs.buf.cpu().numpy()
        want = outs.expect(expected(ref, targets))
        lo = GUARD + len(targets[0]) * (plen + GUARD)  # segment 1's first window
        assert np.array_equal(got[:lo], want[:lo])
        w0 = GUARD + (len(targets[0]) + len(targets[1])) * (plen + GUARD)  # segment 2's first window
        w1 = w0 + len(targets[2]) * (plen + GUARD)
        assert np.array_equal(got[w0 - GUARD:w1], want[w0 - GUARD:w1])
        assert np.all(got[-GUARD:] == 0xCD)
        # the shares themselves are only read
        dirty = buf.cpu().numpy() != clean.cpu().numpy()
        assert int(dirty.sum()) == 2
    finally:
        c.close()


def test_share_check_corrects_through_repair_segments(rs29):
    """repair_segments(check=True): flagged segments are corrected as Decode
    corrects them and repaired again; two bad shares in one column of a k + 3
    set are past correction: infectious.TooManyErrors."""
    from uplink_amd import eestream, repair
    ref, d_ref = rs29
    k, plen = 29, 41 * 256
    sets, targets, buf, pieces = _check_setup(rs29, np.random.default_rng(4))
    scheme = eestream.RSScheme(eestream.new_fec(29, 80), 256)
    try:
        b1, b3 = basis_of(sets[1], k), basis_of(sets[3], k)
        surplus = [x for i, x in enumerate(sets[1]) if i not in b1]
        pieces[1][surplus[0]][plen - 1] ^= 0x01
        pieces[3][sets[3][b3[0]]][77] ^= 0x80
        batch = [(s, [pieces[g][x] for x in s], t) for g, (s, t) in enumerate(zip(sets, targets))]
        outs = repair.repair_segments(scheme, batch, check=True)
        torch.cuda.synchronize()
        for g in range(4):
            assert np.array_equal(outs[g].cpu().numpy(), ref[g][targets[g]]), g
            for x in sets[g]:  # corrected in place, as infectious corrects share.Data
                assert torch.equal(pieces[g][x], d_ref[g][x]), (g, x)
        pieces[2][sets[2][0]][500] ^= 0x10
        pieces[2][sets[2][1]][500] ^= 0x22
        with pytest.raises(eestream.TooManyErrors):
            repair.repair_segments(scheme, batch, check=True)
        # fewer shares than k
        with pytest.raises(eestream.NotEnoughShares):
            repair.repair_segments(scheme, [(sets[0][:k - 1], [pieces[0][x] for x in sets[0][:k - 1]], targets[0])])
    finally:
        torch.cuda.synchronize()
        scheme.close()


def test_errors(rs29):
    """Every validation case; nothing is queued before all segments are
    validated, so a call whose last segment is invalid leaves the outputs of the
    earlier ones untouched."""
    ref, d_pieces = rs29
    k, n, stripes = 29, 80, 41
    N = _native
    rng = np.random.default_rng(9)
    good, gt = random_case(rng, k, n, 6)
    c = Ctx(k, n, 256)
    try:
        def run(sets, targets, **kw):
            rc, outs = call_repair(c, d_pieces, sets, targets, stripes, **kw)
            torch.cuda.synchronize()
            outs.check([None] * outs.count)  # nothing written
            return rc

        assert run([good, good[:k - 1]], [gt, gt]) == N.EC_ERR_NOT_ENOUGH_SHARES
        d80 = [dict(enumerate(d_pieces[g])) for g in range(2)]
        for d in d80:
            d[80] = d[-1] = d[0]  # (a pointer for the invalid numbers)
        for bad in (80, -1):
            rc, outs = call_repair(c, d80, [good, good[:k - 1] + [bad]], [gt, gt], stripes)
            torch.cuda.synchronize()
            outs.check([None] * outs.count)
            assert rc == N.EC_ERR_INVALID_SHARE
        assert run([good, good], [gt, gt[:2] + [80]]) == N.EC_ERR_INVALID_SHARE
        assert run([good, good], [gt, gt[:2] + [-1]]) == N.EC_ERR_INVALID_SHARE
        # a basis share chosen twice
        assert run([good, good[:k - 1] + [good[0]]], [gt, gt]) == N.EC_ERR_SINGULAR
        assert run([good, good], [gt, [good[3]]]) == N.EC_ERR_INVALID_ARG  # a target that is a given share
        assert run([good, good], [gt, [gt[0], gt[1], gt[0]]]) == N.EC_ERR_INVALID_ARG  # repeated
        assert run([good, good], [gt, gt], flags=CHECK) == N.EC_ERR_INVALID_ARG  # the flag without dev_status
        assert run([good, good], [gt, gt], flags=0x8) == N.EC_ERR_INVALID_ARG
        outs = Outs([gt, gt], stripes * 256)
        outs.ptrs[-1] = None
        assert run([good, good], [gt, gt], outs=outs) == N.EC_ERR_INVALID_ARG  # a NULL output
        nullp = [dict(enumerate(d_pieces[0])), dict(enumerate(d_pieces[1]))]

        class Null:
            def data_ptr(self):
                return None
        nullp[1][good[4]] = Null()
        rc, outs = call_repair(c, nullp, [good, good], [gt, gt], stripes)
        torch.cuda.synchronize()
        outs.check([None] * outs.count)
        assert rc == N.EC_ERR_INVALID_ARG  # a NULL share
        # nothing to do
        assert run([good], [[]]) == N.EC_OK
        rc, outs = call_repair(c, d_pieces, [good], [gt], 0)
        assert rc == N.EC_OK
        assert c.L.ec_repair_segments_sets(c.ctx, 0, None, None, None, None, None, None, stripes, 0, None, None) == 0
        # a segment without targets is skipped, its neighbours repaired
        rc, outs = call_repair(c, d_pieces, [good, good[:3], good], [gt, [], gt[:2]], stripes)
        assert rc == N.EC_OK
        torch.cuda.synchronize()
        outs.check(expected(ref, [gt, [], gt[:2]]))
    finally:
        c.close()
    # the engine's limits
    c = Ctx(129, 200, 256)
    try:
        z = torch.zeros(256, dtype=torch.uint8, device="cuda")
        rc, _ = call_repair(c, [{x: z for x in range(200)}], [list(range(129))], [[150]], 1)
        assert rc == N.EC_ERR_UNSUPPORTED
    finally:
        c.close()
    c = Ctx(4, 200, 256)
    try:
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        rc, outs = call_repair(c, [{x: z for x in range(200)}], [list(range(129))], [[150]], 1, flags=CHECK,
                               status=status)
        assert rc == N.EC_ERR_UNSUPPORTED
        torch.cuda.synchronize()
        outs.check([None])
    finally:
        c.close()


def _many_calls(c, ref, d_pieces, seed, stream, ncalls=40):
    """ncalls calls of 2 segments each, distinct sets and targets, queued back to
    back on `stream` with nothing waited for; returns what to verify afterwards"""
    rng = np.random.default_rng(seed)
    done = []
    with torch.cuda.stream(stream):
        for i in range(ncalls):
            seg_of = [int(rng.integers(0, 12)), int(rng.integers(0, 12))]
            cases = [random_case(rng, 29, 80, int(rng.integers(1, 52))) for _ in range(2)]
            sets, targets = [s for s, _ in cases], [t for _, t in cases]
            rc, outs = call_repair(c, d_pieces, sets, targets, 41, stream=stream, seg_of=seg_of)
            assert rc == 0, (i, _native.strerror(rc))
            done.append((outs, expected(ref, targets, seg_of)))
    return done


def test_staging_reuse_back_to_back(rs29):
    """40 calls on one stream with no synchronisation between them: each call's
    staging is its own until the event behind its launches has completed"""
    ref, d_pieces = rs29
    c = Ctx(29, 80, 256)
    try:
        done = _many_calls(c, ref, d_pieces, 40, torch.cuda.current_stream())
        torch.cuda.synchronize()
        assert len(done) == 40
        for outs, want in done:
            outs.check(want)
        # and again, now that every block is free: they are reused
        done = _many_calls(c, ref, d_pieces, 41, torch.cuda.current_stream())
        torch.cuda.synchronize()
        for outs, want in done:
            outs.check(want)
    finally:
        c.close()


def test_staging_reuse_two_threads_two_streams(rs29):
    ref, d_pieces = rs29
    c = Ctx(29, 80, 256)
    try:
        res, errs = {}, []

        def work(i):
            try:
                torch.cuda.set_device(0)
                res[i] = _many_calls(c, ref, d_pieces, 100 + i, torch.cuda.Stream())
            except BaseException as e:  # noqa: BLE001
                errs.append(e)

        ths = [threading.Thread(target=work, args=(i,)) for i in range(2)]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        torch.cuda.synchronize()
        assert not errs, errs
        for i in range(2):
            assert len(res[i]) == 40
            for outs, want in res[i]:
                outs.check(want)
    finally:
        c.close()


def test_round_trip_through_rebuild(oracle):
    """Repaired pieces, mixed with originals, rebuild the original segment"""
    k, n, ess, stripes = 29, 80, 256, 41
    segs, ref = encode_all(oracle, k, n, ess, 2, stripes, 77)
    d_pieces = torch.from_numpy(ref).cuda()
    rng = np.random.default_rng(77)
    cases = [random_case(rng, k, n, 20), random_case(rng, k, n, 40)]
    sets, targets = [s for s, _ in cases], [t for _, t in cases]
    c = Ctx(k, n, ess)
    try:
        rc, outs = call_repair(c, d_pieces, sets, targets, stripes)
        assert rc == 0
        plen = stripes * ess
        dec = torch.full((2, stripes * k * ess), 0xCD, dtype=torch.uint8, device="cuda")
        nums, ptrs, w = [], [], 0
        for g in range(2):
            mix = targets[g][:15] + sets[g][:k - 15]  # 15 repaired pieces, 14 originals
            for x in mix:
                nums.append(x)
                ptrs.append(outs.ptrs[w + targets[g].index(x)] if x in targets[g] else d_pieces[g][x].data_ptr())
            w += len(targets[g])
        rc = c.L.ec_rebuild_segments_sets(c.ctx, 2, (ctypes.c_int * 2)(k, k), (ctypes.c_int * len(nums))(*nums),
                                          (ctypes.c_void_p * len(ptrs))(*ptrs), stripes,
                                          (ctypes.c_void_p * 2)(dec[0].data_ptr(), dec[1].data_ptr()),
                                          torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        torch.cuda.synchronize()
        assert plen * k == dec.shape[1]
        for g in range(2):
            assert np.array_equal(dec[g].cpu().numpy(), segs[g]), g
    finally:
        c.close()


def test_piece_hashes_and_repairer(oracle, rs29):
    """hash_pieces: the BLAKE3 PutPiece sends with each regenerated piece;
    SegmentRepairer: the targets by the thresholds, regenerated"""
    from oracle import blake3 as B
    from uplink_amd import eestream, repair
    ref, d_ref = rs29
    k, n = 29, 80
    rng = np.random.default_rng(5)
    cases = [random_case(rng, k, n, 51), random_case(rng, k, n, 2)]
    scheme = eestream.RSScheme(eestream.new_fec(k, n), 256)
    try:
        batch = [(s, [d_ref[g][x] for x in s], t) for g, (s, t) in enumerate(cases)]
        outs, hashes = repair.repair_segments(scheme, batch, hash_pieces=True)
        torch.cuda.synchronize()
        for g, (s, t) in enumerate(cases):
            assert np.array_equal(outs[g].cpu().numpy(), ref[g][t])
            want = np.stack([np.frombuffer(B.blake3(ref[g][x]), dtype=np.uint8) for x in t])
            assert np.array_equal(hashes[g].cpu().numpy(), want), g
        rep = repair.SegmentRepairer(eestream.RedundancyStrategy(scheme, 35, 65))
        healthy = [int(x) for x in rng.permutation(n)[:33]]
        fine = [int(x) for x in rng.permutation(n)[:36]]
        got = rep.repair([{x: d_ref[3][x] for x in healthy}, {x: d_ref[4][x] for x in fine}])
        torch.cuda.synchronize()
        assert sorted(got[0]) == sorted(set(range(n)) - set(healthy)) and got[1] == {}
        for t, p in got[0].items():
            assert np.array_equal(p.cpu().numpy(), ref[3][t]), t
    finally:
        torch.cuda.synchronize()
        scheme.close()
