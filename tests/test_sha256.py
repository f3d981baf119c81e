"""GPU parity of the SHA-256 piece hash (include/uplink_ec.h ec_sha256_*;
uplink_amd/piecehash.py, uploads.py, repair.py): pieces of different lengths
hashed in one call, one lane per piece.  Expected digests are hashlib.sha256's over
the test's own bytes, or over the oracle's FEC.encode_segment pieces; never the
engine's.  Pieces are windows of one 0xCD-filled buffer with 64-byte guards, the
hash buffer is guarded likewise, and both are compared whole.  No piece is longer
than 263 KiB except the two of the uniform entry point's second launch."""
import ctypes
import hashlib
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

import sha256_checked_child as H  # noqa: E402

N = _native
EDGE = H.EDGE_LENS
UP = H.UPLOAD_STRIPES


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)


@pytest.fixture(scope="module")
def edge():
    """the padding-edge pieces and their digests by hashlib; shared, read-only"""
    return H.edge_pieces()


@pytest.fixture(scope="module")
def rs29(oracle):
    """RS(29,80) ess 256, one upload per UP stripe count: (segments, the oracle's pieces, hashlib's
    digests of them); shared, read-only"""
    return H.upload_batch(oracle, 29, 80, 256, UP, 2983)


def test_checked_library(native):
    """First, so that an access of the lanes kernel outside a piece's own extent, a digest store
    outside the declared range or a state access outside the staging block is skipped and
    reported by the bounds-checked build instead of reaching the card: a fresh process loads
    lib/checked/libuplink_ec_checked.so and runs the padding-edge list, the parity-only upload
    batch and a short list at two blocks per launch.  The two libraries must be one build."""
    child = [sys.executable, os.path.join(HERE, "sha256_checked_child.py")]
    r = subprocess.run(child + ["--build-id"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    ident = r.stdout.split("build", 1)[1].split()[0]
    assert ident == native.ec_build_id().decode(), f"checked library build {ident} is not the product's: rebuild both"
    r = subprocess.run(child, capture_output=True, text=True, timeout=240)
    assert "uplink_ec checked" not in r.stdout + r.stderr, r.stdout + r.stderr
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "ok"


@pytest.mark.parametrize("order", ["given", "reversed", "shuffled"])
def test_every_padding_edge_in_one_list(edge, order):
    """lengths 0, 1, 55, 56, 57, 63, 64, 65, 119, 120, 121, 127, 128, 129, 4096 and 262,400 in one
    call: row i is hashlib's digest of piece i whatever the order, which pins the lane -> row map
    (the lanes are sorted by length)"""
    pieces, hashes = edge
    o = list(range(len(pieces)))
    if order == "reversed":
        o = o[::-1]
    elif order == "shuffled":
        o = [int(x) for x in np.random.default_rng(3).permutation(len(pieces))]
        assert o != sorted(o) and o != sorted(o, reverse=True)
    c = H.Ctx(29, 80, 256)
    try:
        ins, _ = H.run_list(c, [pieces[i] for i in o], [hashes[i] for i in o])
        assert ins.ptrs[o.index(0)] is None  # the empty piece: a NULL pointer
        assert H.stats(c) == [len(pieces), 0, 1]
    finally:
        c.close()


@pytest.mark.parametrize("count", [65, 129])
def test_more_than_one_wave_ragged(count):
    """65 and 129 pieces of (37 * i) % 700 bytes: one lane into a second and into a third wave"""
    pieces, hashes = H.edge_pieces([(37 * i) % 700 for i in range(count)], count)
    c = H.Ctx(29, 80, 256)
    try:
        H.run_list(c, pieces, hashes)
        assert H.stats(c) == [count, 0, 1]
    finally:
        c.close()


def test_alignment(edge):
    """every padding-edge length at base offsets 0, 1, 4, 8 and 15 past 16-byte alignment within
    one allocation, in one call: the pieces at offset 0 (and the empty ones, which have no
    address) take the 16-byte loads, the others the byte loads; same digests"""
    pieces, hashes = edge
    ps, hs, shift = [], [], []
    for i, sh in enumerate([0, 1, 4, 8, 15]):
        for j in range(len(pieces)):
            jj = (j + 3 * i) % len(pieces)  # (another order per offset)
            ps.append(pieces[jj]), hs.append(hashes[jj]), shift.append(sh)
    c = H.Ctx(29, 80, 256)
    try:
        ins, _ = H.run_list(c, ps, hs, shift=shift)
        fast = sum(1 for p in ins.ptrs if p is None or p % 16 == 0)
        assert fast == len(pieces) + 4 and {p % 16 for p in ins.ptrs if p is not None} == {0, 1, 4, 8, 15}
        assert H.stats(c) == [fast, len(ps) - fast, 1]  # both classes ran, in one launch
    finally:
        c.close()


def test_carried_state():
    """two blocks per launch (ec_sha256_set_launch_blocks): lengths 0, 11, .. 330 and one piece of
    4,096 bytes take 33 launches, the state of every unfinished piece carried between them and
    pieces finishing in different launches; the digests are unchanged, the launch counter is the
    geometry's prediction, and the default comes back"""
    lens = list(range(0, 331, 11)) + [4096]
    pieces, hashes = H.edge_pieces(lens, 77)
    c = H.Ctx(29, 80, 256)
    try:
        assert c.L.ec_sha256_set_launch_blocks(c.ctx, 2) == 0
        H.run_list(c, pieces, hashes)
        want = -(-((4096 + 8) // 64 + 1) // 2)
        assert want == 33 == H.launches_of(lens, 2)
        assert H.stats(c) == [len(lens), 0, want]
        # odd addresses: the byte cursor is set anew at every launch
        H.run_list(c, pieces[1:], hashes[1:], shift=[1] * (len(lens) - 1))
        assert H.stats(c) == [len(lens), len(lens) - 1, 2 * want]
        assert c.L.ec_sha256_set_launch_blocks(c.ctx, 0) == 0  # the default again
        H.run_list(c, pieces, hashes)
        assert H.stats(c) == [2 * len(lens), len(lens) - 1, 2 * want + 1]
    finally:
        c.close()


@pytest.mark.parametrize("parity_only", [False, True])
def test_upload_batch(oracle, rs29, parity_only):
    """RS(29,80) ess 256, stripe counts 1, 3, 41, 1025 and 0.  The four uploads that have bytes go
    through encode_uploads(hash_pieces=True, hash_algo=SHA256) (PadReader's padding leaves no
    upload without a stripe): all n digests per upload against hashlib over the oracle's pieces
    of the padded buffer, so with parity_only the data-piece digests read in place from the
    segment equal those of the full encode.  The whole batch, with the skipped segment, goes
    through the calls encode_uploads is made of (SegmentCodec.encode_segments_sized and
    hash_segments_sized(algo=SHA256)) with every hash row pre-filled with 0xA5: the skipped
    segment's rows stay as they were."""
    from uplink_amd import eestream, piecehash, uploads

    sha = piecehash.PieceHashAlgorithm.SHA256
    k, n, ess = 29, 80, 256
    segs, refs, hashes = rs29
    scheme = eestream.RSScheme(eestream.new_fec(k, n), ess)
    try:
        live = [g for g, s in enumerate(UP) if s]
        sizes = [UP[g] * k * ess - 4 - 3 * g for g in live]  # 4 + 3g bytes short of whole stripes
        bufs = [torch.from_numpy(np.array(segs[g])).cuda() for g in live]
        assert [uploads.upload_geometry(s, scheme)[2] for s in sizes] == [UP[g] for g in live]
        pieces, got = uploads.encode_uploads(scheme, list(zip(sizes, bufs)), parity_only=parity_only,
                                             hash_pieces=True, hash_algo=sha)
        torch.cuda.synchronize()
        f = oracle.FEC(k, n)
        for i, g in enumerate(live):
            ref = f.encode_segment(bufs[i].cpu().numpy(), ess, threads=8)  # (the padding is the engine's input too)
            assert np.array_equal(pieces[i].cpu().numpy(), ref[k:] if parity_only else ref), g
            want = np.stack([H.sha(row) for row in ref])
            assert tuple(got[i].shape) == (n, 32) and np.array_equal(got[i].cpu().numpy(), want), g
        # the batch with its skipped segment
        codec = eestream.SegmentCodec(scheme)
        rows = n - k if parity_only else n
        d_segs = [torch.from_numpy(np.array(s)).cuda() if len(s) else None for s in segs]
        d_out = [torch.empty((rows, s * ess), dtype=torch.uint8, device="cuda") if s else None for s in UP]
        d_hash = torch.full((len(UP), n, 32), 0xA5, dtype=torch.uint8, device="cuda")
        codec.encode_segments_sized(d_segs, UP, d_out, parity_only=parity_only)
        codec.hash_segments_sized(d_segs, UP, d_out, d_hash, parity_only=parity_only, algo=sha)
        torch.cuda.synchronize()
        h = d_hash.cpu().numpy()
        for g, s in enumerate(UP):
            if s == 0:
                assert (h[g] == 0xA5).all()
            else:
                assert np.array_equal(d_out[g].cpu().numpy(), refs[g][k:] if parity_only else refs[g]), g
                assert np.array_equal(h[g], hashes[g]), g
    finally:
        torch.cuda.synchronize()
        scheme.close()


@pytest.mark.parametrize("ess,want", [(64, [30, 0, 1]), (8, [11, 19, 1])])
def test_other_runs(oracle, ess, want):
    """RS(4,10), stripe counts 1, 15 and 17, parity only, so that the data pieces are read strided:
    ess 64 -- runs of 64 bytes, every piece on the 16-byte loads; ess 8 -- runs of 8 bytes, byte
    loads (and contiguous pieces of 8, 120 and 136 bytes of which every other one starts 8 bytes
    past 16-byte alignment: 11 pieces fast, 19 bytewise)"""
    k, n, stripes = 4, 10, [1, 15, 17]
    segs, refs, hashes = H.upload_batch(oracle, k, n, ess, stripes, 7 * k + ess)
    c = H.Ctx(k, n, ess)
    try:
        H.run_upload_batch(c, segs, refs, hashes, stripes, parity_only=True)
        assert H.stats(c) == want
    finally:
        c.close()


def test_uniform_entry_points(oracle):
    """hash_device over a strided view (the data pieces in place in a stripe-major segment, and
    contiguous rows at a stride), hash_host, blake3_host(algo=SHA256) and hash_segments(algo=SHA256)
    against hashlib; the default algorithm is still BLAKE3"""
    from oracle import blake3 as ob
    from uplink_amd import eestream, piecehash

    sha = piecehash.PieceHashAlgorithm.SHA256
    k, n, ess, nstripes, nseg = 4, 10, 64, 9, 2
    rng = np.random.default_rng(8)
    seg = rng.integers(0, 256, nseg * nstripes * k * ess, dtype=np.uint8)
    d_seg = torch.from_numpy(seg).cuda()
    plen = nstripes * ess
    # data piece j of segment 0, in place: runs of ess bytes, k*ess apart
    out = torch.empty((k, 32), dtype=torch.uint8, device="cuda")
    piecehash.hash_device(d_seg, k, plen, ess, out, run=ess, run_stride=k * ess, algo=sha)
    torch.cuda.synchronize()
    shares = seg[:nstripes * k * ess].reshape(nstripes, k, ess)
    for j in range(k):
        assert out[j].cpu().numpy().tobytes() == hashlib.sha256(shares[:, j].tobytes()).digest(), j
    # rows of 100 bytes, 113 apart, from an odd address: the byte loads
    out = torch.empty((5, 32), dtype=torch.uint8, device="cuda")
    piecehash.blake3_device(d_seg.data_ptr() + 3, 5, 100, 113, out, algo=sha)
    torch.cuda.synchronize()
    for j in range(5):
        assert out[j].cpu().numpy().tobytes() == hashlib.sha256(seg[3 + 113 * j:3 + 113 * j + 100].tobytes()).digest()
    # host rows
    rows = rng.integers(0, 256, (7, 1000), dtype=np.uint8)
    for call in (piecehash.hash_host, piecehash.blake3_host):
        got = call(rows, algo=sha)
        assert got.shape == (7, 32)
        for j in range(7):
            assert got[j].tobytes() == hashlib.sha256(rows[j].tobytes()).digest()
    assert piecehash.hash_host(rows[0])[0].tobytes() == ob.blake3(rows[0])  # the default: BLAKE3
    assert piecehash.hash_host(np.zeros((2, 0), np.uint8), algo=sha)[1].tobytes() == hashlib.sha256(b"").digest()
    # hash_segments: all n pieces of nseg segments of one size
    scheme = eestream.RSScheme(eestream.new_fec(k, n), ess)
    try:
        codec = eestream.SegmentCodec(scheme)
        par = torch.empty(nseg * (n - k) * plen, dtype=torch.uint8, device="cuda")
        codec.encode_segments(d_seg, nseg, nstripes, par, parity_only=True)
        d_hash = torch.empty((nseg, n, 32), dtype=torch.uint8, device="cuda")
        piecehash.hash_segments(scheme, d_seg, par, nseg, nstripes, d_hash, algo=sha)
        torch.cuda.synchronize()
        f = oracle.FEC(k, n)
        for g in range(nseg):
            ref = f.encode_segment(seg[g * nstripes * k * ess:(g + 1) * nstripes * k * ess], ess, threads=8)
            assert np.array_equal(d_hash[g].cpu().numpy(), np.stack([H.sha(r) for r in ref])), g
    finally:
        torch.cuda.synchronize()
        scheme.close()


def test_uniform_second_launch():
    """two pieces of 1 MiB + 100 bytes through ec_sha256_pieces: 16,386 blocks, so a second launch
    picks the state up from the stream's scratch (the only pieces here above 263 KiB: the uniform
    entry point has no launch_blocks to turn down)"""
    from uplink_amd import piecehash

    ln = (1 << 20) + 100
    assert H.launches_of([ln]) == 2
    data = np.random.default_rng(9).integers(0, 256, 2 * ln, dtype=np.uint8)
    d = torch.from_numpy(data).cuda()
    out = torch.empty((2, 32), dtype=torch.uint8, device="cuda")
    piecehash.hash_device(d, 2, ln, ln, out, algo=piecehash.PieceHashAlgorithm.SHA256)
    torch.cuda.synchronize()
    for j in range(2):
        assert out[j].cpu().numpy().tobytes() == hashlib.sha256(data[j * ln:(j + 1) * ln].tobytes()).digest(), j


def test_repair(oracle):
    """repair_segments_sized(hash_pieces=True, hash_algo=SHA256) for two segments of different
    sizes with targets of different counts: the regenerated pieces are the oracle's, their hashes
    hashlib's; SegmentRepairer.repair_sized passes the algorithm on"""
    from uplink_amd import eestream, piecehash, repair

    sha = piecehash.PieceHashAlgorithm.SHA256
    k, n, ess = 29, 80, 256
    segs, refs = H.encode_segments(oracle, k, n, ess, [3, 41], 31)
    d = [torch.from_numpy(np.array(r)).cuda() for r in refs]
    scheme = eestream.RSScheme(eestream.new_fec(k, n), ess)
    try:
        batch = [(list(range(k)), [d[0][i] for i in range(k)], [40, 79, 33]),
                 (list(range(n - k, n)), [d[1][i] for i in range(n - k, n)], [0])]
        outs, hs = repair.repair_segments_sized(scheme, batch, hash_pieces=True, hash_algo=sha)
        torch.cuda.synchronize()
        assert [tuple(h.shape) for h in hs] == [(3, 32), (1, 32)]
        for g, ((_, _, targets), o, h) in enumerate(zip(batch, outs, hs)):
            for i, t in enumerate(targets):
                assert np.array_equal(o[i].cpu().numpy(), refs[g][t]), (g, t)
                assert h[i].cpu().numpy().tobytes() == hashlib.sha256(refs[g][t].tobytes()).digest(), (g, t)
        outs2, hs2 = repair.repair_segments(scheme, batch[:1], hash_pieces=True, hash_algo=sha)
        torch.cuda.synchronize()
        assert torch.equal(hs2[0], hs[0]) and torch.equal(outs2[0], outs[0])
        rs = eestream.RedundancyStrategy(scheme, 35, 50)
        got, gh = repair.SegmentRepairer(rs).repair_sized([{i: d[0][i] for i in range(k + 2)}], hash_pieces=True,
                                                          hash_algo=sha)
        torch.cuda.synchronize()
        assert sorted(got[0]) == list(range(k + 2, n))
        for t, h in gh[0].items():
            assert h.cpu().numpy().tobytes() == hashlib.sha256(refs[0][t].tobytes()).digest(), t
    finally:
        torch.cuda.synchronize()
        scheme.close()


def test_argument_errors_write_nothing(edge, rs29):
    pieces, hashes = edge
    c = H.Ctx(29, 80, 256)
    try:
        sel = [7, 3, 12, 1]
        ps = [pieces[i] for i in sel]
        lens = [len(p) for p in ps]
        ins, out = H.Ins(ps), H.Outs([32 * len(ps)])

        def untouched():
            torch.cuda.synchronize()
            out.check([None])
            ins.check(ps)

        ptrs = list(ins.ptrs)
        ptrs[2] = None  # a NULL piece with a nonzero length in the middle of the list
        assert H.call_list(c, ptrs, lens, out.ptrs[0]) == N.EC_ERR_INVALID_ARG
        untouched()
        assert H.call_list(c, ins.ptrs, lens, None) == N.EC_ERR_INVALID_ARG
        st = torch.cuda.current_stream().cuda_stream
        a_len = (ctypes.c_size_t * 4)(*lens)
        a_ptr = (ctypes.c_void_p * 4)(*ins.ptrs)
        assert c.L.ec_sha256_pieces_list(c.ctx, 4, None, a_len, out.ptrs[0], st) == N.EC_ERR_INVALID_ARG
        assert c.L.ec_sha256_pieces_list(c.ctx, 4, a_ptr, None, out.ptrs[0], st) == N.EC_ERR_INVALID_ARG
        assert c.L.ec_sha256_pieces_list(c.ctx, 0, None, None, None, st) == N.EC_OK
        assert H.call_list(c, ins.ptrs, [lens[0], 1 << 61, lens[2], lens[3]], out.ptrs[0]) == N.EC_ERR_UNSUPPORTED
        untouched()
        assert H.stats(c) == [0, 0, 0]
        # the segment form: a NULL pieces[g] / segs[g] of a segment that is not skipped
        segs, refs, _ = rs29
        sg = [segs[1], segs[4], segs[2]]
        stripes = [UP[1], 0, UP[2]]
        sin = H.Ins(sg)
        pout = H.Outs(H.piece_sizes(c, stripes, True))
        hout = H.Outs([32 * c.n * 3])
        for which in ("pieces", "segs"):
            sp, pp = list(sin.ptrs), list(pout.ptrs)
            (pp if which == "pieces" else sp)[2] = None
            assert H.call_sha_sized(c, sp, stripes, pp, hout.ptrs[0], parity_only=True) == N.EC_ERR_INVALID_ARG
        assert H.call_sha_sized(c, None, stripes, pout.ptrs, hout.ptrs[0], parity_only=True) == N.EC_ERR_INVALID_ARG
        assert H.call_sha_sized(c, sin.ptrs, stripes, pout.ptrs, None, parity_only=True) == N.EC_ERR_INVALID_ARG
        assert H.call_sha_sized(c, sin.ptrs, [3, 0, 1 << 62], pout.ptrs, hout.ptrs[0]) == N.EC_ERR_UNSUPPORTED
        # a capturing stream: refused before anything is staged
        stream = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=stream, capture_error_mode="relaxed"):
            torch.zeros(1, device="cuda")  # (something for the graph to hold)
            rc = H.call_list(c, ins.ptrs, lens, out.ptrs[0], stream=stream)
        assert rc == N.EC_ERR_UNSUPPORTED
        torch.cuda.synchronize()
        hout.check([None])
        untouched()
        assert H.stats(c) == [0, 0, 0]
        # and the context still works
        assert H.call_list(c, ins.ptrs, lens, out.ptrs[0]) == 0
        torch.cuda.synchronize()
        out.check([np.concatenate([hashes[i] for i in sel])])
    finally:
        c.close()


def _list_calls(c, edge, count, seed, stream, errors):
    """`count` list calls back to back on one stream over varying small lists, checked at the end"""
    try:
        pieces, hashes = edge
        rng = np.random.default_rng(seed)
        runs = []
        with torch.cuda.stream(stream):
            for _ in range(count):
                o = [int(x) for x in rng.choice(len(pieces), size=int(rng.integers(1, 6)), replace=False)]
                ins = H.Ins([pieces[i] for i in o])
                out = H.Outs([32 * len(o)])
                rc = H.call_list(c, ins.ptrs, [len(pieces[i]) for i in o], out.ptrs[0], stream=stream)
                assert rc == 0, N.strerror(rc)
                runs.append((ins, out, o))
            stream.synchronize()
        for ins, out, o in runs:
            out.check([np.concatenate([hashes[i] for i in o])])
            ins.check([pieces[i] for i in o])
    except BaseException as e:  # noqa: BLE001 - handed to the test's thread
        errors.append(e)


def test_staging_reuse_two_threads_two_streams(edge):
    """two threads on two streams, 20 list calls each of different small lists on one context,
    none waited for before the last: the staging blocks, which also hold the carried state, are
    recycled behind their events"""
    c = H.Ctx(29, 80, 256)
    try:
        assert c.L.ec_sha256_set_launch_blocks(c.ctx, 64) == 0  # (the longest piece: 65 launches, state carried)
        errors = []
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        ts = [threading.Thread(target=_list_calls, args=(c, edge, 20, 600 + i, streams[i], errors)) for i in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errors, errors
    finally:
        c.close()
