"""GPU parity of the sized share-set calls (include/uplink_ec.h
ec_rebuild_segments_sized, ec_decode_segments_sized, uplink_amd/downloads.py):
a batch of segments, each from its own share set and of its own size, in one
call.  Every expected segment is the test's own random input, its pieces the
oracle's encode_segment output; outputs are carved out of 0xCD-filled buffers
with guards, which must come back untouched, and the piece buffers are compared
whole as well (a Rebuild writes no input)."""
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
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import sized_checked_child as H  # noqa: E402

N = _native
EDGE = H.EDGE_STRIPES


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)


@pytest.fixture(scope="module")
def rs29(oracle):
    """RS(29,80), ess 256, one segment per EDGE stripe count: (segments, reference
    pieces, the same on the device); shared by the tests and left unchanged"""
    segs, refs = H.encode_segments(oracle, 29, 80, 256, EDGE, 2980)
    return segs, refs, H.to_device(refs)


def by_stripes(rs29, stripes):
    """(segments, refs, device pieces) of the EDGE segments with these stripe counts"""
    segs, refs, d = rs29
    idx = [EDGE.index(s) for s in stripes]
    return [segs[i] for i in idx], [refs[i] for i in idx], [d[i] for i in idx]


def pieces_unchanged(d, refs):
    for g, (t, r) in enumerate(zip(d, refs)):
        assert np.array_equal(t.cpu().numpy(), r), f"the pieces of segment {g} were written"


def test_checked_library(native):
    """First, so that an access of the new kernel outside its segment's own share
    or output is skipped and reported by the bounds-checked build instead of
    reaching the card: a fresh process loads lib/checked/libuplink_ec_checked.so
    and runs the tile-edge RS(29,80) batch, both orders, and a Decode batch.  The
    two libraries must be one build."""
    child = [sys.executable, os.path.join(HERE, "sized_checked_child.py")]
    r = subprocess.run(child + ["--build-id"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    ident = r.stdout.split("build", 1)[1].split()[0]
    assert ident == native.ec_build_id().decode(), f"checked library build {ident} is not the product's: rebuild both"
    r = subprocess.run(child, capture_output=True, text=True, timeout=240)
    assert "uplink_ec checked" not in r.stdout + r.stderr, r.stdout + r.stderr
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "ok"


@pytest.mark.parametrize("reverse", [False, True])
def test_tile_edges_in_one_call(rs29, reverse):
    """Stripe counts 1, 4, 5, 7, 8, 9, 16, 17, 41, 0, 130 of RS(29,80) ess 256 (8
    stripes per tile) in one call: less than half a tile, the vB boundary at 64
    chunks, one tile minus / exactly / plus one stripe, two tiles exactly and plus
    one, ragged last tiles, a skipped segment (too few shares, NULL output: none
    of it is looked at).  A shuffled 29-subset each; one segment with every data
    share present, one all parity, one with k + 6 shares."""
    segs, refs, d = rs29
    sets = H.edge_sets(np.random.default_rng(11))
    o = list(range(len(EDGE)))[::-1] if reverse else list(range(len(EDGE)))
    c = H.Ctx(29, 80, 256)
    try:
        rc, outs, _ = H.call_sized(c, [d[g] for g in o], [sets[g] for g in o], [EDGE[g] for g in o])
        assert rc == 0, N.strerror(rc)
        assert outs.ptrs[o.index(9)] is None
        torch.cuda.synchronize()
        outs.check([segs[g] for g in o])
        pieces_unchanged(d, refs)
        assert c.L.ec_last_body(c.ctx) == N.EC_BODY_JUMP_TABLE
    finally:
        c.close()


def test_wave_classes_by_sizes(rs29):
    """1 .. 29 missing data shares: the 2-, 3- and 4-wave classes (up to 14, 24, 29
    rows) on each side of their boundaries, a different stripe count per segment;
    the 2-wave class holds 9, 41 and 1 stripes next to each other in its tile map,
    the 3-wave class 17, 5 and 8, the 4-wave class 16 and 130."""
    plan = [(1, 9), (15, 17), (14, 41), (25, 16), (24, 5), (5, 1), (29, 130), (20, 8)]
    stripes = [s for _, s in plan]
    segs, refs, d = by_stripes(rs29, stripes)
    rng = np.random.default_rng(3)
    sets = [H.missing_set(rng, 29, 80, m) for m, _ in plan]
    for (m, _), s in zip(plan, sets):
        assert len(set(s)) == 29 and sum(x >= 29 for x in s) == m
    c = H.Ctx(29, 80, 256)
    try:
        rc, outs, _ = H.call_sized(c, d, sets, stripes)
        assert rc == 0, N.strerror(rc)
        torch.cuda.synchronize()
        outs.check(segs)
        pieces_unchanged(d, refs)
    finally:
        c.close()


@pytest.mark.parametrize("k,n,ess,stripes", [(20, 60, 4096, [1, 2, 3]), (4, 10, 64, [1, 31, 32, 33, 257]),
                                             (50, 80, 256, [9, 1]), (128, 256, 16, [3, 1])])
def test_other_geometries(oracle, k, n, ess, stripes):
    """ess 4096: a tile is half a stripe; ess 64: 32 stripes (out_off / copy_off are
    offsets within a stripe of the segment's own output); a wide code; RS(128,256)
    from parity only: 128 rows, more than one pass of rows on 4 waves."""
    segs, refs = H.encode_segments(oracle, k, n, ess, stripes, k * 1000 + ess)
    d = H.to_device(refs)
    rng = np.random.default_rng(k + ess)
    sets = [H.shuffled_subset(rng, n, k) for _ in stripes]
    sets[0] = [n - 1 - x for x in H.shuffled_subset(rng, k, k)]  # the last k shares
    c = H.Ctx(k, n, ess)
    try:
        for decode in (False, True):
            rc, outs, codes = H.call_sized(c, d, sets, stripes, decode=decode)
            assert rc == 0, N.strerror(rc)
            torch.cuda.synchronize()
            outs.check(segs)
            pieces_unchanged(d, refs)
            assert codes is None or codes == [0] * len(stripes)
    finally:
        c.close()


def test_equal_sizes_agree_with_the_sets_call(oracle):
    """6 segments x 41 stripes: byte for byte what ec_rebuild_segments_sets writes, and the oracle's"""
    k, n, ess, stripes = 29, 80, 256, [41] * 6
    segs, refs = H.encode_segments(oracle, k, n, ess, stripes, 641)
    d = H.to_device(refs)
    rng = np.random.default_rng(6)
    sets = [H.missing_set(rng, k, n, m) for m in (3, 29, 16, 0, 22, 9)]
    c = H.Ctx(k, n, ess)
    try:
        rc, outs, _ = H.call_sized(c, d, sets, stripes)
        assert rc == 0, N.strerror(rc)
        other = H.Outs([41 * k * ess] * 6)
        flat = [x for s in sets for x in s]
        rc = c.L.ec_rebuild_segments_sets(
            c.ctx, 6, (ctypes.c_int * 6)(*[k] * 6), (ctypes.c_int * len(flat))(*flat),
            (ctypes.c_void_p * len(flat))(*[d[g][x].data_ptr() for g, s in enumerate(sets) for x in s]), 41,
            (ctypes.c_void_p * 6)(*other.ptrs), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, N.strerror(rc)
        torch.cuda.synchronize()
        assert torch.equal(outs.buf, other.buf)
        outs.check(segs)
        pieces_unchanged(d, refs)
    finally:
        c.close()


def _decode_batch(rs29, stripes, extra, seed):
    segs, refs, d = by_stripes(rs29, stripes)
    rng = np.random.default_rng(seed)
    sets = [H.shuffled_subset(rng, 80, 29 + extra) for _ in stripes]
    return segs, refs, [t.clone() for t in d], sets


def test_decode_corrects_one_piece(rs29):
    """k + 2 shares each; segment 1 (9 stripes: one tile and a stripe) has one piece
    damaged in a few bytes, its last 16-byte chunk among them: flagged by the
    pass, corrected in place and rebuilt; the other segments' pieces untouched"""
    stripes = [1, 9, 41, 17]
    segs, refs, dp, sets = _decode_batch(rs29, stripes, 2, 62)
    victim = dp[1][sets[1][11]]
    for at, v in ((0, 0x01), (700, 0xFF), (victim.numel() - 16, 0x80), (victim.numel() - 1, 0x33)):
        victim[at] ^= v
    c = H.Ctx(29, 80, 256)
    try:
        rc, outs, codes = H.call_sized(c, dp, sets, stripes, decode=True)
        assert rc == 0, N.strerror(rc)
        assert codes == [0, 0, 0, 0]
        outs.check(segs)
        pieces_unchanged(dp, refs)  # (segment 1's corrected, as infectious corrects share.Data)
    finally:
        c.close()


def test_decode_uncorrectable_segment_does_not_stop_the_others(rs29):
    """k + 1 shares each and one piece of segment 2 damaged: a single surplus share
    detects any single-share error and corrects none, so segment 2's outcome is
    EC_ERR_TOO_MANY_ERRORS, which the call returns, while the other segments'
    outputs are complete and right.  seg_rc == NULL: the same code.
    (ec_decode_segments words this case NotEnoughShares, as infectious does,
    tests/test_decode_edges.py case X3; in the sized call too few shares is only
    ever the call's argument error, and a segment's outcome is TooManyErrors.)"""
    stripes = [5, 8, 17, 4, 16]
    segs, refs, dp, sets = _decode_batch(rs29, stripes, 1, 71)
    dp[2][sets[2][5]][1000] ^= 0x44
    c = H.Ctx(29, 80, 256)
    try:
        for want_rc in (True, False):
            rc, outs, codes = H.call_sized(c, dp, sets, stripes, decode=True, want_rc=want_rc)
            print(f"seg_rc {'given' if want_rc else 'NULL'}: rc {rc}, codes {codes}")
            outs.check(segs, skip=[2])
            for g in (0, 1, 3, 4):
                assert np.array_equal(dp[g].cpu().numpy(), refs[g]), g
            assert rc == N.EC_ERR_TOO_MANY_ERRORS, N.strerror(rc)
            if want_rc:
                assert codes == [0, 0, N.EC_ERR_TOO_MANY_ERRORS, 0, 0]
    finally:
        c.close()


def test_decode_each_failed_segment_has_its_own_outcome(rs29):
    """A batch in which segment 0 has k + 1 shares and one error (detected, nothing
    to correct with), segment 2 has k + 2 shares and two bad pieces in one column
    (both TooManyErrors), segment 3 has k + 2 shares and one bad piece
    (corrected) and the others are clean:
    every flagged segment is attempted, seg_rc holds each outcome, the call
    returns the first in segment order, and the segments that succeeded are
    complete and right.  seg_rc == NULL: the same code."""
    stripes = [5, 8, 17, 4, 16]
    segs, refs, dp, sets = _decode_batch(rs29, stripes, 2, 72)
    sets[0] = sets[0][:30]
    dp[0][sets[0][3]][77] ^= 0x01
    dp[2][sets[2][0]][500] ^= 0x10
    dp[2][sets[2][1]][500] ^= 0x22
    dp[3][sets[3][9]][4 * 256 - 1] ^= 0x80
    c = H.Ctx(29, 80, 256)
    try:
        for want_rc in (True, False):
            if not want_rc:  # (corrected by the first call: damaged again)
                dp[3][sets[3][9]][4 * 256 - 1] ^= 0x80
            rc, outs, codes = H.call_sized(c, dp, sets, stripes, decode=True, want_rc=want_rc)
            assert rc == N.EC_ERR_TOO_MANY_ERRORS, N.strerror(rc)
            if want_rc:
                assert codes == [N.EC_ERR_TOO_MANY_ERRORS, 0, N.EC_ERR_TOO_MANY_ERRORS, 0, 0]
            outs.check(segs, skip=[0, 2])
            for g in (1, 3, 4):
                assert np.array_equal(dp[g].cpu().numpy(), refs[g]), g
    finally:
        c.close()


def test_off_the_bit_sliced_path(oracle, rs29):
    """A share size that is no multiple of 16 (every segment through the byte
    kernel, its own stripe count); and an ess-256 batch in which one segment has a
    piece pointer 8 bytes off and another its output: those two go on their own,
    the rest stay in the pass; the results are the same."""
    k, n, ess, stripes = 29, 80, 100, [3, 0, 7]
    segs, refs = H.encode_segments(oracle, k, n, ess, stripes, 100)
    d = H.to_device(refs)
    rng = np.random.default_rng(100)
    sets = [H.shuffled_subset(rng, n, k) for _ in stripes]
    c = H.Ctx(k, n, ess)
    try:
        rc, outs, _ = H.call_sized(c, d, sets, stripes)
        assert rc == 0, N.strerror(rc)
        torch.cuda.synchronize()
        outs.check(segs)
        pieces_unchanged(d, refs)
    finally:
        c.close()
    stripes = [9, 17, 5, 41]
    segs, refs, d = by_stripes(rs29, stripes)
    sets = [H.shuffled_subset(rng, 80, 29) for _ in stripes]
    # segment 1's third share copied to an address 8 bytes past alignment
    plen = 17 * 256
    off = torch.full((plen + 32,), 0xEE, dtype=torch.uint8, device="cuda")
    shifted = off[8:8 + plen]
    assert shifted.data_ptr() % 16 == 8
    shifted.copy_(d[1][sets[1][2]])
    pieces = [{x: t[x] for x in range(80)} for t in d]
    pieces[1][sets[1][2]] = shifted
    c = H.Ctx(29, 80, 256)
    try:
        for decode in (False, True):
            outs = H.Outs([s * 29 * 256 for s in stripes], shift=[0, 0, 8, 0])
            assert outs.ptrs[2] % 16 == 8 and outs.ptrs[3] % 16 == 0
            rc, outs, codes = H.call_sized(c, pieces, sets, stripes, outs=outs, decode=decode)
            assert rc == 0, N.strerror(rc)
            torch.cuda.synchronize()
            outs.check(segs)
            pieces_unchanged(d, refs)
            assert off[:8].eq(0xEE).all() and off[8 + plen:].eq(0xEE).all()
            assert codes is None or codes == [0, 0, 0, 0]
    finally:
        c.close()


def test_errors(rs29):
    """Every validation case, in Rebuild and in Decode: all segments are checked
    before anything is queued, so a call whose last segment is invalid leaves the
    outputs of the earlier ones untouched."""
    stripes = [9, 41, 5]
    segs, refs, d = by_stripes(rs29, stripes)
    k, n = 29, 80
    rng = np.random.default_rng(9)
    good = [H.shuffled_subset(rng, n, k) for _ in stripes]
    c = H.Ctx(k, n, 256)
    try:
        def run(sets, decode, pieces=None, st=None, outs=None, **kw):
            outs = outs or H.Outs([s * k * 256 for s in stripes])
            rc, outs, _ = H.call_sized(c, pieces or d, sets, st or stripes, outs=outs, decode=decode, **kw)
            torch.cuda.synchronize()
            outs.check([None] * len(sets))  # nothing written: windows and guards still 0xCD
            return rc

        for decode in (False, True):
            assert run(good[:2] + [good[2][:k - 1]], decode) == N.EC_ERR_NOT_ENOUGH_SHARES
            # a basis share chosen twice
            assert run(good[:2] + [good[2][:k - 1] + [good[2][0]]], decode) == N.EC_ERR_SINGULAR
            assert run(good, decode, null_stripes=True) == N.EC_ERR_INVALID_ARG
            outs = H.Outs([s * k * 256 for s in stripes])
            outs.ptrs[2] = None
            assert run(good, decode, outs=outs) == N.EC_ERR_INVALID_ARG  # a NULL output of a non-empty segment
            nullp = [{x: t[x] for x in range(n)} for t in d]
            nullp[2][good[2][4]] = None
            assert run(good, decode, pieces=nullp) == N.EC_ERR_INVALID_ARG  # a NULL share
            # a stripe count whose chunks do not fit 32 bits
            assert run(good, decode, st=[9, 41, 1 << 28]) == N.EC_ERR_UNSUPPORTED
        # a share number out of range: among the surplus shares Decode checks them all
        d80 = [{x: t[min(max(x, 0), n - 1)] for x in range(-1, n + 1)} for t in d]
        for bad in (80, -1):
            assert run(good[:2] + [good[2] + [bad]], True, pieces=d80) == N.EC_ERR_INVALID_SHARE
        assert run(good[:2] + [good[2][:k - 1] + [80]], False, pieces=d80) == N.EC_ERR_INVALID_SHARE
        # a capturing stream: refused before anything is staged
        for decode in (False, True):
            s = torch.cuda.Stream()
            graph = torch.cuda.CUDAGraph()
            outs = H.Outs([x * k * 256 for x in stripes])
            with torch.cuda.graph(graph, stream=s, capture_error_mode="relaxed"):
                torch.zeros(1, device="cuda")  # (something for the graph to hold)
                rc, _, _ = H.call_sized(c, d, good, stripes, outs=outs, decode=decode, stream=s)
            assert rc == N.EC_ERR_UNSUPPORTED
            torch.cuda.synchronize()
            outs.check([None] * 3)
        # nothing to do
        assert c.L.ec_rebuild_segments_sized(c.ctx, 0, None, None, None, None, None, None) == 0
        assert c.L.ec_decode_segments_sized(c.ctx, 0, None, None, None, None, None, None, None) == 0
        assert run(good, False, st=[0, 0, 0]) == N.EC_OK
        # the context still works afterwards
        rc, outs, codes = H.call_sized(c, d, good, stripes, decode=True)
        assert rc == 0 and codes == [0, 0, 0]
        outs.check(segs)
        pieces_unchanged(d, refs)
    finally:
        c.close()
    # the engine's limit
    c = H.Ctx(129, 200, 256)
    try:
        z = torch.zeros(256, dtype=torch.uint8, device="cuda")
        rc, outs, _ = H.call_sized(c, [{x: z for x in range(200)}], [list(range(129))], [1])
        assert rc == N.EC_ERR_UNSUPPORTED
        torch.cuda.synchronize()
        outs.check([None])
    finally:
        c.close()


def _many_calls(c, rs29, seed, stream, ncalls=40):
    """ncalls calls of 3 segments each, distinct sets and sizes, queued back to back
    on `stream` with nothing waited for; returns what to verify afterwards"""
    segs, refs, d = rs29
    rng = np.random.default_rng(seed)
    pool = [g for g, s in enumerate(EDGE) if 0 < s <= 41]
    done = []
    with torch.cuda.stream(stream):
        for i in range(ncalls):
            pick = [pool[int(x)] for x in rng.integers(0, len(pool), 3)]
            sets = [H.missing_set(rng, 29, 80, int(rng.integers(0, 30))) for _ in pick]
            rc, outs, _ = H.call_sized(c, [d[g] for g in pick], sets, [EDGE[g] for g in pick], stream=stream)
            assert rc == 0, (i, N.strerror(rc))
            done.append((outs, [segs[g] for g in pick]))
    return done


def test_staging_reuse_back_to_back(rs29):
    """40 calls on one stream with no synchronisation between them: each call's
    staging is its own until the event behind its launches has completed"""
    c = H.Ctx(29, 80, 256)
    try:
        done = _many_calls(c, rs29, 40, torch.cuda.current_stream())
        torch.cuda.synchronize()
        assert len(done) == 40
        for outs, want in done:
            outs.check(want)
        # and again, now that every block is free: they are reused
        done = _many_calls(c, rs29, 41, torch.cuda.current_stream())
        torch.cuda.synchronize()
        for outs, want in done:
            outs.check(want)
        pieces_unchanged(rs29[2], rs29[1])
    finally:
        c.close()


def test_staging_reuse_two_threads_two_streams(rs29):
    c = H.Ctx(29, 80, 256)
    try:
        res, errs = {}, []

        def work(i):
            try:
                torch.cuda.set_device(0)
                res[i] = _many_calls(c, rs29, 100 + i, torch.cuda.Stream())
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


def test_decode_downloads(oracle):
    """Downloads of 0, 1, 7423, 7424, 7425 and 300000 bytes of RS(29,80) (stripe
    7424): the pieces are the oracle's encode of the plaintext padded to whole
    stripes; each result is the plaintext, `size` bytes long."""
    from uplink_amd import downloads, eestream
    k, n, ess = 29, 80, 256
    sizes = [0, 1, 7423, 7424, 7425, 300000]
    rng = np.random.default_rng(2026)
    f = oracle.FEC(k, n)
    scheme = eestream.RSScheme(eestream.new_fec(k, n), ess)
    try:
        plain, batch = [], []
        for size in sizes:
            padded, piece_size, nstripes = downloads.segment_geometry(size, scheme)
            p = rng.integers(0, 256, size, dtype=np.uint8)
            plain.append(p)
            seg = np.concatenate([p, rng.integers(0, 256, padded - size, dtype=np.uint8)])
            ref = f.encode_segment(seg, ess) if nstripes else np.zeros((n, 0), dtype=np.uint8)
            assert ref.shape == (n, piece_size)
            dref = torch.from_numpy(ref).cuda()
            batch.append((size, {x: dref[x] for x in H.shuffled_subset(rng, n, k + 2)}))
        for detect in (False, True):
            outs = downloads.decode_downloads(scheme, batch, error_detection=detect)
            torch.cuda.synchronize()
            for size, p, o in zip(sizes, plain, outs):
                assert o.numel() == size and o.is_cuda
                assert np.array_equal(o.cpu().numpy(), p), size
        # one piece of the last download damaged: corrected under error detection; with one
        # surplus share only, detected and reported per download (TooManyErrors)
        size, pieces = batch[-1]
        nums = list(pieces)
        pieces[nums[3]][77] ^= 0x21
        outs, errs = downloads.decode_downloads(scheme, batch, error_detection=True, collect_errors=True)
        assert errs == [None] * len(sizes)
        assert np.array_equal(outs[-1].cpu().numpy(), plain[-1])
        pieces[nums[3]][77] ^= 0x21
        short = dict(list(pieces.items())[:k + 1])
        batch[-1] = (size, short)
        outs, errs = downloads.decode_downloads(scheme, batch, error_detection=True, collect_errors=True)
        assert isinstance(errs[-1], eestream.TooManyErrors) and errs[:-1] == [None] * (len(sizes) - 1)
        for p, o in zip(plain[:-1], outs[:-1]):
            assert np.array_equal(o.cpu().numpy(), p)
        with pytest.raises(eestream.TooManyErrors):
            downloads.decode_downloads(scheme, batch, error_detection=True)
        # a piece of the wrong length
        pieces[nums[3]][77] ^= 0x21
        wrong = dict(short)
        wrong[nums[0]] = short[nums[0]][:-256]
        with pytest.raises(eestream.InfectiousError) as ei:
            downloads.decode_downloads(scheme, batch[:-1] + [(size, wrong)])
        assert ei.value.code == N.EC_ERR_SHARE_SIZE
    finally:
        torch.cuda.synchronize()
        scheme.close()


def test_fresh_context_lone_small_segment(rs29):
    """A new context's first call: one segment of one stripe"""
    segs, refs, d = by_stripes(rs29, [1])
    sets = [H.shuffled_subset(np.random.default_rng(1), 80, 29)]
    c = H.Ctx(29, 80, 256)
    try:
        rc, outs, _ = H.call_sized(c, d, sets, [1])
        assert rc == 0, N.strerror(rc)
        torch.cuda.synchronize()
        outs.check(segs)
        pieces_unchanged(d, refs)
    finally:
        c.close()
