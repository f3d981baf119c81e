"""GPU parity of segment repair with a size per segment (include/uplink_ec.h
ec_repair_segments_sized, uplink_amd/repair.py repair_segments_sized): the lost
pieces of a batch of segments of different sizes regenerated in one call, a
share set and a target set per segment.  Every expected piece is the oracle's
encode_segment row of the test's own random segment, compared bit-exact;
outputs are carved out of 0xCD-filled buffers with guards, which must come back
untouched, and the input pieces are compared whole afterwards."""
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

import repair_sized_checked_child as H  # noqa: E402

N = _native
EDGE = H.EDGE_STRIPES
CHECK = H.CHECK


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
    """(refs, device pieces) of the EDGE segments with these stripe counts"""
    _, refs, d = rs29
    idx = [EDGE.index(s) for s in stripes]
    return [refs[i] for i in idx], [d[i] for i in idx]


def run_batch(c, refs, d, sets, targets, stripes, **kw):
    """one call over device pieces d, checked against the oracle's pieces refs"""
    rc, outs = H.call_repair_sized(c, H.edge_pieces(d), sets, targets, stripes, **kw)
    assert rc == 0, N.strerror(rc)
    torch.cuda.synchronize()
    outs.check(H.expected(refs, targets))
    H.pieces_unchanged(d, refs)
    return outs


def test_checked_library(native):
    """First, so that an access of the new kernel outside its segment's own shares
    or outputs is skipped and reported by the bounds-checked build instead of
    reaching the card: a fresh process loads lib/checked/libuplink_ec_checked.so
    and runs the tile-edge RS(29,80) batch in both orders, and once with the
    share check.  The two libraries must be one build."""
    child = [sys.executable, os.path.join(HERE, "repair_sized_checked_child.py")]
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
    """Stripe counts 1, 4, 5, 7, 8, 9, 16, 17, 41, 0, 130, 8 of RS(29,80) ess 256 (8
    stripes per tile) in one call: less than half a tile, the vB boundary at 64
    chunks, one tile minus / exactly / plus one stripe, two tiles exactly and plus
    one, ragged last tiles; the segment of no stripes has NULL pointers and too
    few shares, the last one no targets.  A shuffled share set each, 1 .. 51
    targets."""
    _, refs, d = rs29
    sets, targets = H.edge_cases(np.random.default_rng(11))
    assert sorted(len(t) for t in targets)[-1] == 51 and [] in targets
    o = list(range(len(EDGE)))[::-1] if reverse else list(range(len(EDGE)))
    c = H.Ctx(29, 80, 256)
    try:
        outs = run_batch(c, [refs[g] for g in o], [d[g] for g in o], [sets[g] for g in o], [targets[g] for g in o],
                         [EDGE[g] for g in o])
        assert None in outs.ptrs  # the skipped segment's outputs
        assert c.L.ec_last_body(c.ctx) == N.EC_BODY_JUMP_TABLE
    finally:
        c.close()


def test_wave_classes_by_sizes(oracle):
    """RS(50,200): 14/15, 24/25, 32/33, 51, 64 and 65 rows (the 2-, 3-, 4- and 8-wave
    classes on each side of their boundaries; 65 rows are two passes on 8 waves),
    a different stripe count per segment, so every class's tile map holds
    different sizes side by side.  With the share check, three segments have
    surplus shares whose syndrome rows take the row count across a boundary
    (12 + 3, 30 + 3, 60 + 5)."""
    k, n, ess = 50, 200, 256
    plan = [(14, 0, 3), (12, 3, 9), (24, 0, 1), (25, 0, 17), (32, 0, 5), (30, 3, 8), (51, 0, 2), (64, 0, 4),
            (60, 5, 10), (65, 0, 7), (15, 0, 16), (33, 0, 6)]
    stripes = [s for _, _, s in plan]
    assert len(set(stripes)) == len(stripes)
    _, refs = H.encode_segments(oracle, k, n, ess, stripes, 50200)
    d = H.to_device(refs)
    rng = np.random.default_rng(50)
    cases = [H.random_case(rng, k, n, nt, extra) for nt, extra, _ in plan]
    sets, targets = [s for s, _ in cases], [t for _, t in cases]
    c = H.Ctx(k, n, ess)
    try:
        run_batch(c, refs, d, sets, targets, stripes)
        status = torch.full((len(plan),), 7, dtype=torch.int32, device="cuda")
        run_batch(c, refs, d, sets, targets, stripes, flags=CHECK, status=status)
        assert status.cpu().tolist() == [0] * len(plan)
    finally:
        c.close()


@pytest.mark.parametrize("k,n,ess,stripes,nt", [(20, 60, 4096, [1, 2, 3], None), (4, 10, 64, [1, 31, 32, 33, 257], None),
                                                (1, 3, 256, [20, 3, 9], None), (128, 256, 16, [3, 1], 128)])
def test_other_geometries(oracle, k, n, ess, stripes, nt):
    """ess 4096: a tile is half a stripe; ess 64: 32 stripes per tile; RS(1,3) is
    replication; RS(128,256) with 128 targets: two passes of 64 rows on 8 waves.
    The first segment from the last k shares, all others regenerated."""
    _, refs = H.encode_segments(oracle, k, n, ess, stripes, k * 1000 + ess)
    d = H.to_device(refs)
    rng = np.random.default_rng(k + ess)
    cases = [H.random_case(rng, k, n, nt or int(rng.integers(1, n - k + 1))) for _ in stripes]
    cases[0] = (list(range(n - k, n))[::-1], list(range(n - k)))
    sets, targets = [s for s, _ in cases], [t for _, t in cases]
    c = H.Ctx(k, n, ess)
    try:
        run_batch(c, refs, d, sets, targets, stripes)
    finally:
        c.close()


def test_off_the_bit_sliced_path(oracle, rs29):
    """A share size that is no multiple of 16 (every segment through the byte
    kernel, its own stripe count, the share check included); and an ess-256 batch
    in which one segment has a share pointer 8 bytes off and another an output
    pointer 8 bytes off, between aligned segments of other sizes: those two go on
    their own, the rest stay in the pass; the results are the same."""
    k, n, ess, stripes = 29, 80, 24, [41, 0, 3, 7]
    _, refs = H.encode_segments(oracle, k, n, ess, stripes, 24)
    d = H.to_device(refs)
    rng = np.random.default_rng(24)
    cases = [H.random_case(rng, k, n, cnt, extra) for cnt, extra in ((51, 0), (2, 0), (3, 2), (20, 0))]
    sets, targets = [s for s, _ in cases], [t for _, t in cases]
    c = H.Ctx(k, n, ess)
    try:
        run_batch(c, refs, d, sets, targets, stripes)
        status = torch.full((4,), 7, dtype=torch.int32, device="cuda")
        run_batch(c, refs, d, sets, targets, stripes, flags=CHECK, status=status)
        assert status.cpu().tolist() == [0, 0, 0, 0]
    finally:
        c.close()
    stripes = [9, 17, 5, 41, 1]
    refs, d = by_stripes(rs29, stripes)
    cases = [H.random_case(rng, 29, 80, cnt) for cnt in (10, 40, 3, 51, 7)]
    sets, targets = [s for s, _ in cases], [t for _, t in cases]
    # segment 1's third share copied to an address 8 bytes past alignment
    plen = 17 * 256
    off = torch.full((plen + 32,), 0xEE, dtype=torch.uint8, device="cuda")
    shifted = off[8:8 + plen]
    assert shifted.data_ptr() % 16 == 8
    shifted.copy_(d[1][sets[1][2]])
    pieces = H.edge_pieces(d)
    pieces[1][sets[1][2]] = shifted
    # segment 3's second output 8 bytes past alignment
    sizes = [stripes[g] * 256 for g, t in enumerate(targets) for _ in t]
    shift = [0] * len(sizes)
    w = len(targets[0]) + len(targets[1]) + len(targets[2]) + 1
    shift[w] = 8
    c = H.Ctx(29, 80, 256)
    try:
        outs = H.Outs(sizes, shift=shift)
        assert outs.ptrs[w] % 16 == 8 and outs.ptrs[w + 1] % 16 == 0 and outs.ptrs[w - 1] % 16 == 0
        rc, outs = H.call_repair_sized(c, pieces, sets, targets, stripes, outs=outs)
        assert rc == 0, N.strerror(rc)
        torch.cuda.synchronize()
        outs.check(H.expected(refs, targets))
        H.pieces_unchanged(d, refs)
        assert off[:8].eq(0xEE).all() and off[8 + plen:].eq(0xEE).all()
    finally:
        c.close()


def _check_setup(rs29, rng, stripes, extras, counts):
    """segments of these stripe counts with k + extras[g] shares each, the shares
    copied into one buffer whose gaps hold 0xFF: (refs, nums, targets, buffer,
    piece tensors per segment)"""
    refs, d = by_stripes(rs29, stripes)
    cases = [H.random_case(rng, 29, 80, cnt, extra) for cnt, extra in zip(counts, extras)]
    sets, targets = [s for s, _ in cases], [t for _, t in cases]
    total = sum(len(s) * (st * 256 + H.S.GUARD) for s, st in zip(sets, stripes))
    buf = torch.full((H.S.GUARD + total,), 0xFF, dtype=torch.uint8, device="cuda")
    pieces, at = [], H.S.GUARD
    for g, s in enumerate(sets):
        row, plen = {}, stripes[g] * 256
        for x in s:
            row[x] = buf[at:at + plen]
            row[x].copy_(d[g][x])
            at += plen + H.S.GUARD
        pieces.append(row)
    return refs, sets, targets, buf, pieces


def test_share_check(rs29):
    """k + 3 and k + 20 shares over segments of 5, 41, 9 and 17 stripes and one of
    none (skipped): clean, every status word is 0, the skipped segment's too, from
    a buffer prefilled with 7.  Then one byte in the last valid column of the
    shortest segment and one in the ragged last tile of the 41-stripe segment
    (bytes 10240 .. 10495 of its pieces): only those two words become 1."""
    stripes = [5, 41, 9, 17]
    refs, sets, targets, buf, pieces = _check_setup(rs29, np.random.default_rng(3), stripes, [3, 20, 20, 3],
                                                    [5, 20, 31, 30])
    # the skipped segment last: no stripes, NULL pointers
    sets.append([7, 3, 60])
    targets.append([1, 2])
    pieces.append({7: None, 3: None, 60: None})
    refs = refs + [np.zeros((80, 0), dtype=np.uint8)]
    stripes = stripes + [0]
    clean = buf.clone()
    c = H.Ctx(29, 80, 256)
    try:
        status = torch.full((5,), 7, dtype=torch.int32, device="cuda")
        rc, outs = H.call_repair_sized(c, pieces, sets, targets, stripes, flags=CHECK, status=status)
        assert rc == 0, N.strerror(rc)
        torch.cuda.synchronize()
        assert status.cpu().tolist() == [0, 0, 0, 0, 0]
        outs.check(H.expected(refs, targets))
        assert torch.equal(buf, clean)
        pieces[0][sets[0][1]][5 * 256 - 1] ^= 0x01
        pieces[1][sets[1][30]][10300] ^= 0x80
        status.fill_(7)
        rc, outs = H.call_repair_sized(c, pieces, sets, targets, stripes, flags=CHECK, status=status)
        assert rc == 0, N.strerror(rc)
        torch.cuda.synchronize()
        assert status.cpu().tolist() == [1, 1, 0, 0, 0]
        # the unflagged segments' pieces are right, every guard is intact
        want = H.expected(refs, targets)
        flagged = len(targets[0]) + len(targets[1])
        got = outs.buf.cpu().numpy()
        full = outs.expect(want)
        lo = outs.offs[flagged] - H.S.GUARD
        assert np.array_equal(got[lo:], full[lo:])
        for i in range(flagged):
            a, b = outs.offs[i], outs.offs[i] + outs.sizes[i]
            assert np.all(got[a - H.S.GUARD:a] == 0xCD) and np.all(got[b:b + 16] == 0xCD)
        # the shares themselves are only read
        assert int((buf != clean).sum()) == 2
    finally:
        c.close()


def test_share_check_corrects_through_repair_segments_sized(rs29):
    """repair_segments_sized(check=True): flagged segments are corrected in place
    as Decode corrects them, each with its own stripe count, and repaired again;
    two bad shares in one column of a k + 3 set are past correction:
    infectious.TooManyErrors, as repair_segments raises it."""
    from uplink_amd import eestream, repair
    stripes = [5, 41, 9, 17]
    refs, sets, targets, buf, pieces = _check_setup(rs29, np.random.default_rng(4), stripes, [3, 3, 3, 3],
                                                    [5, 20, 48, 30])
    scheme = eestream.RSScheme(eestream.new_fec(29, 80), 256)
    try:
        pieces[1][sets[1][0]][10300] ^= 0x01
        pieces[3][sets[3][9]][77] ^= 0x80
        batch = [(s, [pieces[g][x] for x in s], t) for g, (s, t) in enumerate(zip(sets, targets))]
        outs = repair.repair_segments_sized(scheme, batch, check=True)
        torch.cuda.synchronize()
        for g in range(4):
            assert outs[g].shape == (len(targets[g]), stripes[g] * 256) and outs[g].data_ptr() % 16 == 0
            assert np.array_equal(outs[g].cpu().numpy(), refs[g][targets[g]]), g
            for x in sets[g]:  # corrected in place, as infectious corrects share.Data
                assert np.array_equal(pieces[g][x].cpu().numpy(), refs[g][x]), (g, x)
        pieces[2][sets[2][0]][500] ^= 0x10
        pieces[2][sets[2][1]][500] ^= 0x22
        with pytest.raises(eestream.TooManyErrors):
            repair.repair_segments_sized(scheme, batch, check=True)
        # fewer shares than k
        with pytest.raises(eestream.NotEnoughShares):
            repair.repair_segments_sized(scheme, [batch[0], (sets[1][:28], [pieces[1][x] for x in sets[1][:28]],
                                                             targets[1])])
    finally:
        torch.cuda.synchronize()
        scheme.close()


def test_pass_split(oracle):
    """1030 segments of one and two stripes of RS(4,10) ess 64 in one call: more
    than a pass holds, so the call goes in two passes"""
    k, n, ess = 4, 10, 64
    base = [1, 2] * 8
    _, refs16 = H.encode_segments(oracle, k, n, ess, base, 410)
    d16 = H.to_device(refs16)
    rng = np.random.default_rng(1030)
    nseg = 1030
    pick = [int(x) for x in rng.integers(0, 16, nseg)]
    cases = [H.random_case(rng, k, n, int(rng.integers(1, 4))) for _ in range(nseg)]
    sets, targets = [s for s, _ in cases], [t for _, t in cases]
    c = H.Ctx(k, n, ess)
    try:
        rc, outs = H.call_repair_sized(c, H.edge_pieces([d16[i] for i in pick]), sets, targets, [base[i] for i in pick])
        assert rc == 0, N.strerror(rc)
        torch.cuda.synchronize()
        outs.check(H.expected([refs16[i] for i in pick], targets))
        H.pieces_unchanged(d16, refs16)
    finally:
        c.close()


def test_errors(rs29):
    """Every validation case in the last segment of a batch: all segments are
    checked before anything is queued, so every output byte and every status word
    of the batch stays as it was."""
    stripes = [9, 41, 5]
    refs, d = by_stripes(rs29, stripes)
    k, n = 29, 80
    rng = np.random.default_rng(9)
    cases = [H.random_case(rng, k, n, 6) for _ in stripes]
    good, gt = [s for s, _ in cases], [t for _, t in cases]
    sizes = [stripes[g] * 256 for g in range(3) for _ in range(6)]
    c = H.Ctx(k, n, 256)
    try:
        def run(sets, targets, pieces=None, st=None, outs=None, flags=CHECK, **kw):
            outs = outs or H.Outs(sizes[:sum(len(t) for t in targets)])
            status = torch.full((3,), 0x55, dtype=torch.int32, device="cuda")
            rc, outs = H.call_repair_sized(c, pieces or H.edge_pieces(d), sets, targets, st or stripes, outs=outs,
                                           flags=flags, status=status if flags == CHECK else None, **kw)
            torch.cuda.synchronize()
            outs.check([None] * len(outs.sizes))  # nothing written: windows and guards still 0xCD
            assert status.cpu().tolist() == [0x55] * 3
            return rc

        assert run(good[:2] + [good[2][:k - 1]], gt) == N.EC_ERR_NOT_ENOUGH_SHARES
        d80 = [{x: t[min(max(x, 0), n - 1)] for x in range(-1, n + 1)} for t in d]
        for bad in (80, -1):
            assert run(good[:2] + [good[2][:k - 1] + [bad]], gt, pieces=d80) == N.EC_ERR_INVALID_SHARE
            assert run(good, gt[:2] + [gt[2][:5] + [bad]]) == N.EC_ERR_INVALID_SHARE
        # a basis share chosen twice
        assert run(good[:2] + [good[2][:k - 1] + [good[2][0]]], gt) == N.EC_ERR_SINGULAR
        assert run(good, gt[:2] + [gt[2][:5] + [good[2][3]]]) == N.EC_ERR_INVALID_ARG  # a target that is a given share
        assert run(good, gt[:2] + [gt[2][:5] + [gt[2][0]]]) == N.EC_ERR_INVALID_ARG  # repeated
        assert run(good, gt, flags=0x8) == N.EC_ERR_INVALID_ARG
        assert run(good, gt, null_stripes=True) == N.EC_ERR_INVALID_ARG
        outs = H.Outs(sizes)
        outs.ptrs[-1] = None
        assert run(good, gt, outs=outs) == N.EC_ERR_INVALID_ARG  # a NULL output
        nullp = H.edge_pieces(d)
        nullp[2][good[2][4]] = None
        assert run(good, gt, pieces=nullp) == N.EC_ERR_INVALID_ARG  # a NULL share
        # a stripe count whose chunks do not fit 32 bits
        assert run(good, gt, st=[9, 41, 1 << 28]) == N.EC_ERR_UNSUPPORTED
        # the flag without dev_status
        outs = H.Outs(sizes)
        rc, _ = H.call_repair_sized(c, H.edge_pieces(d), good, gt, stripes, outs=outs, flags=CHECK)
        assert rc == N.EC_ERR_INVALID_ARG
        # a capturing stream: refused before anything is staged
        s = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        outs = H.Outs(sizes)
        status = torch.full((3,), 0x55, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=s, capture_error_mode="relaxed"):
            torch.zeros(1, device="cuda")  # (something for the graph to hold)
            rc, _ = H.call_repair_sized(c, H.edge_pieces(d), good, gt, stripes, outs=outs, flags=CHECK, status=status,
                                        stream=s)
        assert rc == N.EC_ERR_UNSUPPORTED
        torch.cuda.synchronize()
        outs.check([None] * len(sizes))
        assert status.cpu().tolist() == [0x55] * 3
        # nothing to do
        assert c.L.ec_repair_segments_sized(c.ctx, 0, None, None, None, None, None, None, None, 0, None, None) == 0
        rc, outs = H.call_repair_sized(c, H.edge_pieces(d), good, gt, [0, 0, 0], outs=H.Outs(sizes))
        assert rc == N.EC_OK
        torch.cuda.synchronize()
        outs.check([None] * len(sizes))
        # the context still works afterwards
        run_batch(c, refs, d, good, gt, stripes)
    finally:
        c.close()
    # the engine's limits
    z = torch.zeros(256, dtype=torch.uint8, device="cuda")
    c = H.Ctx(129, 200, 256)
    try:
        rc, outs = H.call_repair_sized(c, [{x: z for x in range(200)}], [list(range(129))], [[150]], [1])
        assert rc == N.EC_ERR_UNSUPPORTED
        torch.cuda.synchronize()
        outs.check([None])
    finally:
        c.close()
    c = H.Ctx(4, 200, 256)
    try:
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        rc, outs = H.call_repair_sized(c, [{x: z for x in range(200)}], [list(range(129))], [[150]], [1], flags=CHECK,
                                       status=status)
        assert rc == N.EC_ERR_UNSUPPORTED
        torch.cuda.synchronize()
        outs.check([None])
    finally:
        c.close()


def _many_calls(c, rs29, seed, stream, ncalls=40):
    """ncalls calls of 3 segments each, distinct sets, targets and sizes, queued
    back to back on `stream` with nothing waited for; returns what to verify afterwards"""
    _, refs, d = rs29
    rng = np.random.default_rng(seed)
    pool = [g for g, s in enumerate(EDGE) if 0 < s <= 41]
    done = []
    with torch.cuda.stream(stream):
        for i in range(ncalls):
            pick = [pool[int(x)] for x in rng.integers(0, len(pool), 3)]
            cases = [H.random_case(rng, 29, 80, int(rng.integers(1, 52))) for _ in pick]
            sets, targets = [s for s, _ in cases], [t for _, t in cases]
            rc, outs = H.call_repair_sized(c, H.edge_pieces([d[g] for g in pick]), sets, targets,
                                           [EDGE[g] for g in pick], stream=stream)
            assert rc == 0, (i, N.strerror(rc))
            done.append((outs, H.expected([refs[g] for g in pick], targets)))
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
        H.pieces_unchanged(rs29[2], rs29[1])
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


def test_equal_sizes_agree_with_the_sets_call(rs29):
    """6 segments x 41 stripes: byte for byte what ec_repair_segments_sets writes, and the oracle's"""
    refs, d = by_stripes(rs29, [41] * 6)
    rng = np.random.default_rng(6)
    cases = [H.random_case(rng, 29, 80, cnt) for cnt in (3, 51, 16, 25, 33, 9)]
    sets, targets = [s for s, _ in cases], [t for _, t in cases]
    c = H.Ctx(29, 80, 256)
    try:
        outs = run_batch(c, refs, d, sets, targets, [41] * 6)
        other = H.Outs(outs.sizes)
        flat = [x for s in sets for x in s]
        tflat = [x for t in targets for x in t]
        rc = c.L.ec_repair_segments_sets(
            c.ctx, 6, (ctypes.c_int * 6)(*[len(s) for s in sets]), (ctypes.c_int * len(flat))(*flat),
            (ctypes.c_void_p * len(flat))(*[d[g][x].data_ptr() for g, s in enumerate(sets) for x in s]),
            (ctypes.c_int * 6)(*[len(t) for t in targets]), (ctypes.c_int * len(tflat))(*tflat),
            (ctypes.c_void_p * len(tflat))(*other.ptrs), 41, 0, None, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, N.strerror(rc)
        torch.cuda.synchronize()
        assert torch.equal(outs.buf, other.buf)
    finally:
        c.close()


def test_round_trip_hashes_and_repairer(oracle, rs29):
    """Repaired pieces of segments of different sizes, mixed with originals,
    decode to the original segments (decode_downloads); hash_pieces: the BLAKE3
    PutPiece sends with each regenerated piece, a length per piece;
    SegmentRepairer.repair_sized on dicts of different sizes."""
    from oracle import blake3 as B
    from uplink_amd import downloads, eestream, repair
    stripes = [9, 41, 1, 17]
    segs, _, _ = rs29
    segs = [segs[EDGE.index(s)] for s in stripes]
    refs, d = by_stripes(rs29, stripes)
    k, n = 29, 80
    rng = np.random.default_rng(5)
    cases = [H.random_case(rng, k, n, cnt) for cnt in (20, 51, 40, 16)]
    scheme = eestream.RSScheme(eestream.new_fec(k, n), 256)
    try:
        batch = [(s, [d[g][x] for x in s], t) for g, (s, t) in enumerate(cases)]
        outs, hashes = repair.repair_segments_sized(scheme, batch, hash_pieces=True)
        torch.cuda.synchronize()
        dl = []
        for g, (s, t) in enumerate(cases):
            assert np.array_equal(outs[g].cpu().numpy(), refs[g][t]), g
            want = np.stack([np.frombuffer(B.blake3(refs[g][x]), dtype=np.uint8) for x in t])
            assert np.array_equal(hashes[g].cpu().numpy(), want), g
            # 15 regenerated pieces, 14 originals and 2 more for the error detection
            mix = {x: outs[g][i] for i, x in enumerate(t[:15])}
            mix.update({x: d[g][x] for x in s[:k - 15 + 2]})
            dl.append((segs[g].size, mix))
        for detect in (False, True):
            back = downloads.decode_downloads(scheme, dl, error_detection=detect)
            torch.cuda.synchronize()
            for g in range(4):
                assert np.array_equal(back[g].cpu().numpy(), segs[g]), (detect, g)
        H.pieces_unchanged(d, refs)
        rep = repair.SegmentRepairer(eestream.RedundancyStrategy(scheme, 35, 65))
        healthy = [[int(x) for x in rng.permutation(n)[:cnt]] for cnt in (33, 36, 29, 35)]
        got, gh = rep.repair_sized([{x: d[g][x] for x in h} for g, h in enumerate(healthy)], hash_pieces=True)
        torch.cuda.synchronize()
        assert got[1] == {} and gh[1] == {}
        for g in (0, 2, 3):
            assert sorted(got[g]) == sorted(set(range(n)) - set(healthy[g]))
            for t, p in got[g].items():
                assert np.array_equal(p.cpu().numpy(), refs[g][t]), (g, t)
                assert gh[g][t].cpu().numpy().tobytes() == B.blake3(refs[g][t]), (g, t)
    finally:
        torch.cuda.synchronize()
        scheme.close()
