"""GPU parity of the list form of the piece hash (include/uplink_ec.h
ec_blake3_pieces_list, ec_hash_segments_sized; uplink_amd/piecehash.py,
uploads.py, repair.py): pieces of different lengths hashed in one call.
Expected hashes are oracle.blake3's over the test's own bytes, or over the
oracle's FEC.encode_segment pieces; never the engine's.  Pieces are windows of one
0xCD-filled buffer with 64-byte guards, the hash buffer is guarded likewise, and
both are compared whole."""
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

import hash_sized_checked_child as H  # noqa: E402

N = _native
EDGE = H.EDGE_LENS
UP = H.UPLOAD_STRIPES


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)


@pytest.fixture(scope="module")
def ob(oracle):
    from oracle import blake3
    return blake3


@pytest.fixture(scope="module")
def edge(ob):
    """the tree-edge pieces and their hashes by the oracle; shared, read-only"""
    return H.edge_pieces(ob)


@pytest.fixture(scope="module")
def rs29(oracle, ob):
    """RS(29,80) ess 256, one upload per UP stripe count: (segments, the oracle's pieces, the
    oracle's hashes of them); shared, read-only"""
    return H.upload_batch(oracle, ob, 29, 80, 256, UP, 2982)


def test_checked_library(native):
    """First, so that an access of the list kernels outside a piece's own extent, or a hash or
    node store outside the declared range, is skipped and reported by the bounds-checked build
    instead of reaching the card: a fresh process loads lib/checked/libuplink_ec_checked.so and
    runs the tree-edge list (in order, reversed) and the upload batch (in order, reversed, with
    and without EC_FLAG_PARITY_ONLY).  The two libraries must be one build."""
    child = [sys.executable, os.path.join(HERE, "hash_sized_checked_child.py")]
    r = subprocess.run(child + ["--build-id"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    ident = r.stdout.split("build", 1)[1].split()[0]
    assert ident == native.ec_build_id().decode(), f"checked library build {ident} is not the product's: rebuild both"
    r = subprocess.run(child, capture_output=True, text=True, timeout=240)
    assert "uplink_ec checked" not in r.stdout + r.stderr, r.stdout + r.stderr
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "ok"


@pytest.mark.parametrize("reverse", [False, True])
def test_every_tree_edge_in_one_list(edge, reverse):
    """lengths 0 .. 2,319,360 across the block, chunk and group edges, with two-, three- and
    nine-group parents folds, in one call: one fast chunk launch and one parents launch"""
    pieces, hashes = edge
    if reverse:
        pieces, hashes = pieces[::-1], hashes[::-1]
    c = H.Ctx(29, 80, 256)
    try:
        ins, _ = H.run_list(c, pieces, hashes)
        assert ins.ptrs[[len(p) for p in pieces].index(0)] is None  # the empty piece: a NULL pointer
        assert H.stats(c) == [1, 0, 1, 0]
    finally:
        c.close()


def test_mixed_alignment(edge):
    """every third piece starts at an odd address: those take the byte path, the others keep
    the 16-byte loads (one launch of each kind), same hashes"""
    pieces, hashes = edge
    c = H.Ctx(29, 80, 256)
    try:
        H.run_list(c, pieces, hashes, shift=[1 if i % 3 == 2 else 0 for i in range(len(pieces))])
        assert H.stats(c) == [1, 1, 1, 0]
        # all of them odd (without the empty piece, which has no address): no fast launch
        H.run_list(c, pieces[1:], hashes[1:], shift=[1] * (len(pieces) - 1))
        assert H.stats(c) == [1, 2, 2, 0]
    finally:
        c.close()


@pytest.mark.parametrize("parity_only", [False, True])
@pytest.mark.parametrize("reverse", [False, True])
def test_upload_batch(rs29, reverse, parity_only):
    """stripe counts 1, 3, 4, 5, 0, 41, 130, 1023, 1024, 1025 in one ec_encode_segments_sized +
    ec_hash_segments_sized: all n hashes per segment against the oracle (so, with parity only,
    the data-piece hashes read in place from the segment equal those of the full encode); the
    skipped segment has NULL pointers and its hash rows stay 0xCD"""
    segs, refs, hashes = rs29
    o = list(range(len(UP)))[::-1] if reverse else list(range(len(UP)))
    c = H.Ctx(29, 80, 256)
    try:
        H.run_upload_batch(c, [segs[g] for g in o], [refs[g] for g in o], [hashes[g] for g in o], [UP[g] for g in o],
                           parity_only=parity_only)
        assert H.stats(c) == [1, 0, 1, 0]  # one pass, every piece on the 16-byte loads
    finally:
        c.close()


@pytest.mark.parametrize("k,n,ess,stripes,want", [(4, 10, 64, [1, 15, 16, 17, 4100], [1, 0, 1, 0]),
                                                  (2, 4, 8, [1, 127, 128, 129, 33000], [1, 1, 1, 0]),
                                                  (3, 7, 24, [1, 42, 43, 11000], [1, 1, 1, 0])])
def test_other_runs(oracle, ob, k, n, ess, stripes, want):
    """parity only, so that the data pieces are read strided: RS(4,10) ess 64 -- 64-byte runs, the
    block path of the fast kernel; RS(2,4) ess 8 and RS(3,7) ess 24 -- the byte path for the data
    pieces (one with a run that is no power of two) while the contiguous parity pieces keep the
    fast path; the last segment of each has pieces of more than one group"""
    segs, refs, hashes = H.upload_batch(oracle, ob, k, n, ess, stripes, 7 * k + ess)
    c = H.Ctx(k, n, ess)
    try:
        H.run_upload_batch(c, segs, refs, hashes, stripes, parity_only=True)
        assert H.stats(c) == want
    finally:
        c.close()


def test_oversize_fallback(ob):
    """a piece of 64 MiB + 1025 bytes (257 groups) between two small ones: it goes on its own
    through the uniform launch, the others through the list pass"""
    lens = [1025, 64 * 1024 * 1024 + 1025, 300 * 1024]
    pieces, hashes = H.edge_pieces(ob, lens, 64)
    c = H.Ctx(29, 80, 256)
    try:
        H.run_list(c, pieces, hashes)
        assert H.stats(c) == [1, 0, 1, 1]
    finally:
        c.close()


def test_python_surface(oracle, ob):
    """encode_uploads(hash_pieces=True) on sizes 0, 1, 7420, 7421, 100000: the hashes are the
    oracle's over the oracle's pieces of the padded buffer, also with parity_only; without
    hash_pieces the return is the list of piece tensors as before.  repair_segments
    (hash_pieces=True): the tensors ec_blake3_pieces gives for each output."""
    from uplink_amd import eestream, piecehash, repair, uploads

    k, n, ess = 29, 80, 256
    scheme = eestream.RSScheme(eestream.new_fec(k, n), ess)
    try:
        rng = np.random.default_rng(12)
        sizes = [0, 1, 7420, 7421, 100000]
        geo = [uploads.upload_geometry(s, scheme) for s in sizes]
        bufs = []
        for s, (padded, _, _) in zip(sizes, geo):
            b = np.full(padded, 0xEE, dtype=np.uint8)
            b[:s] = rng.integers(0, 256, s, dtype=np.uint8)
            bufs.append(torch.from_numpy(b).cuda())
        plain = uploads.encode_uploads(scheme, list(zip(sizes, bufs)))
        assert isinstance(plain, list) and all(isinstance(p, torch.Tensor) for p in plain)
        pieces, hashes = uploads.encode_uploads(scheme, list(zip(sizes, bufs)), hash_pieces=True)
        par, par_hashes = uploads.encode_uploads(scheme, list(zip(sizes, bufs)), parity_only=True, hash_pieces=True)
        torch.cuda.synchronize()
        f = oracle.FEC(k, n)
        base = hashes[0].untyped_storage().data_ptr()
        for g, (padded, piece_size, _) in enumerate(geo):
            ref = f.encode_segment(bufs[g].cpu().numpy(), ess, threads=8)
            want = ob.blake3_many(np.ascontiguousarray(ref), threads=8)
            assert tuple(pieces[g].shape) == (n, piece_size) and tuple(hashes[g].shape) == (n, 32)
            assert np.array_equal(pieces[g].cpu().numpy(), ref) and torch.equal(pieces[g], plain[g])
            assert np.array_equal(hashes[g].cpu().numpy(), want), g
            assert tuple(par[g].shape) == (n - k, piece_size) and torch.equal(par[g], pieces[g][k:])
            assert np.array_equal(par_hashes[g].cpu().numpy(), want), g
            assert hashes[g].untyped_storage().data_ptr() == base  # views of one buffer
        # blake3_pieces_list on tensors, one of them empty
        ts = [pieces[4][3], torch.empty(0, dtype=torch.uint8, device="cuda"), bufs[2][:1000]]
        got = piecehash.blake3_pieces_list(scheme, ts)
        torch.cuda.synchronize()
        assert tuple(got.shape) == (3, 32)
        for t, h in zip(ts, got):
            assert h.cpu().numpy().tobytes() == ob.blake3(t.cpu().numpy())
        # repair: two segments with targets of different counts
        p4 = pieces[4]
        batch = [(list(range(k)), [p4[i] for i in range(k)], [40, 79, 33]),
                 (list(range(n - k, n)), [p4[i] for i in range(n - k, n)], [0])]
        outs, hs = repair.repair_segments(scheme, batch, hash_pieces=True)
        torch.cuda.synchronize()
        assert [tuple(h.shape) for h in hs] == [(3, 32), (1, 32)]
        L = N.load()
        for (_, _, targets), o, h in zip(batch, outs, hs):
            for i, t in enumerate(targets):
                assert torch.equal(o[i], p4[t])
            if o.shape[0]:
                want = torch.empty((o.shape[0], 32), dtype=torch.uint8, device="cuda")
                rc = L.ec_blake3_pieces(o.data_ptr(), o.shape[0], o.shape[1], o.shape[1], 0, 0, want.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream)
                assert rc == 0
                torch.cuda.synchronize()
                assert torch.equal(h, want)
    finally:
        torch.cuda.synchronize()
        scheme.close()


def _list_calls(c, edge, count, seed, stream, errors):
    """`count` list calls back to back on one stream over varying small lists, checked at the end"""
    try:
        pieces, hashes = edge
        small = [i for i, p in enumerate(pieces) if len(p) <= 257 * 1024]
        rng = np.random.default_rng(seed)
        runs = []
        with torch.cuda.stream(stream):
            for _ in range(count):
                o = [int(x) for x in rng.choice(small, size=int(rng.integers(1, 6)), replace=False)]
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
    """two threads on two streams, 50 list calls each of different small lists on one context,
    none waited for before the last: the staging blocks are recycled behind their events"""
    c = H.Ctx(29, 80, 256)
    try:
        errors = []
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        ts = [threading.Thread(target=_list_calls, args=(c, edge, 50, 500 + i, streams[i], errors)) for i in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errors, errors
    finally:
        c.close()


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
        assert c.L.ec_blake3_pieces_list(c.ctx, 4, None, a_len, out.ptrs[0], st) == N.EC_ERR_INVALID_ARG
        assert c.L.ec_blake3_pieces_list(c.ctx, 4, a_ptr, None, out.ptrs[0], st) == N.EC_ERR_INVALID_ARG
        assert c.L.ec_blake3_pieces_list(c.ctx, 0, None, None, None, st) == N.EC_OK
        untouched()
        assert H.stats(c) == [0, 0, 0, 0]
        # the segment form: a NULL pieces[g] / segs[g] of a segment that is not skipped
        segs, refs, _ = rs29
        sg = [segs[1], segs[4], segs[5]]
        stripes = [UP[1], 0, UP[5]]
        sin = H.Ins(sg)
        pout = H.Outs(H.piece_sizes(c, stripes, True))
        hout = H.Outs([32 * c.n * 3])
        for which in ("pieces", "segs"):
            sp, pp = list(sin.ptrs), list(pout.ptrs)
            (pp if which == "pieces" else sp)[2] = None
            assert H.call_hash_sized(c, sp, stripes, pp, hout.ptrs[0], parity_only=True) == N.EC_ERR_INVALID_ARG
        assert H.call_hash_sized(c, None, stripes, pout.ptrs, hout.ptrs[0], parity_only=True) == N.EC_ERR_INVALID_ARG
        assert H.call_hash_sized(c, sin.ptrs, stripes, pout.ptrs, None, parity_only=True) == N.EC_ERR_INVALID_ARG
        assert H.call_hash_sized(c, sin.ptrs, [3, 0, 1 << 62], pout.ptrs, hout.ptrs[0]) == N.EC_ERR_UNSUPPORTED
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
        assert H.stats(c) == [0, 0, 0, 0]
        # and the context still works
        assert H.call_list(c, ins.ptrs, lens, out.ptrs[0]) == 0
        torch.cuda.synchronize()
        out.check([np.concatenate([hashes[i] for i in sel])])
    finally:
        c.close()
