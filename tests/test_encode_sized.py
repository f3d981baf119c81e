"""GPU parity of the sized encode (include/uplink_ec.h ec_encode_segments_sized,
uplink_amd/uploads.py): a batch of segments of different sizes encoded in one
call.  Expected pieces are the oracle's FEC.encode_segment of the test's own
random segments; piece buffers are windows of one 0xCD-filled buffer with
64-byte guards, compared whole, and so are the inputs (without data_len the call
writes no input byte)."""
import contextlib
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

import encode_sized_checked_child as H  # noqa: E402

N = _native
BLOCK = H.BLOCK_STRIPES


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)


@pytest.fixture(scope="module")
def rs29(oracle):
    """RS(29,80), ess 256, one segment per BLOCK stripe count: (segments, reference
    pieces); shared by the tests and left unchanged (read-only arrays)"""
    return H.encode_segments(oracle, 29, 80, 256, BLOCK, 2981)


def pick(rs29, idx):
    segs, refs = rs29
    return [segs[g] for g in idx], [refs[g] for g in idx], [BLOCK[g] for g in idx]


def test_checked_library(native):
    """First, so that an access of the new kernel outside its segment's own input or
    pieces is skipped and reported by the bounds-checked build instead of reaching
    the card: a fresh process loads lib/checked/libuplink_ec_checked.so and runs
    the block-edge RS(29,80) batches (in order, reversed, 53 blocks, one ragged
    block alone) and a parity-only batch.  The two libraries must be one build."""
    child = [sys.executable, os.path.join(HERE, "encode_sized_checked_child.py")]
    r = subprocess.run(child + ["--build-id"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    ident = r.stdout.split("build", 1)[1].split()[0]
    assert ident == native.ec_build_id().decode(), f"checked library build {ident} is not the product's: rebuild both"
    r = subprocess.run(child, capture_output=True, text=True, timeout=240)
    assert "uplink_ec checked" not in r.stdout + r.stderr, r.stdout + r.stderr
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "ok"


@pytest.mark.parametrize("name,order", H.block_batches(), ids=[b[0].replace(" ", "_") for b in H.block_batches()])
def test_block_edges_in_one_call(rs29, name, order):
    """Stripe counts 1, 3, 4, 5, 8, 9, 0, 41, 130 of RS(29,80) ess 256 (4 stripes per
    block) in one call: a quarter block, one stripe under a block, exactly a block
    and one over, two blocks and one over, a skipped segment with NULL pointers,
    ragged 10.25 and 32.5 blocks -- 54 blocks; reversed, so that a tile's two
    blocks land in other segments of other piece lengths; without the 1-stripe
    segment, 53 blocks, so that the last tile has no second block."""
    segs, refs, stripes = pick(rs29, order)
    c = H.Ctx(29, 80, 256)
    try:
        _, outs = H.run_batch(c, segs, refs, stripes)
        if 0 in stripes:
            assert outs.ptrs[stripes.index(0)] is None
        q, s = ctypes.c_ulonglong(), ctypes.c_ulonglong()
        assert c.L.ec_encoder_queue_stats(c.ctx, ctypes.byref(q), ctypes.byref(s)) == 0
        assert q.value + s.value == 1, "one encoder launch for the whole batch"
    finally:
        c.close()


def test_one_ragged_block_alone(rs29):
    """one 1-stripe segment on a fresh context: a single tile of only block A, a quarter full"""
    segs, refs, stripes = pick(rs29, [0])
    c = H.Ctx(29, 80, 256)
    try:
        H.run_batch(c, segs, refs, stripes)
    finally:
        c.close()


@pytest.mark.parametrize("reverse", [False, True])
def test_parity_only(rs29, reverse):
    """EC_FLAG_PARITY_ONLY on the block-edge batch: pieces[g] is [51][...], nothing else written"""
    o = list(range(len(BLOCK)))
    segs, refs, stripes = pick(rs29, o[::-1] if reverse else o)
    c = H.Ctx(29, 80, 256)
    try:
        H.run_batch(c, segs, refs, stripes, parity_only=True)
    finally:
        c.close()


@pytest.mark.parametrize("k,n,ess,stripes", [(50, 80, 256, [9, 1]), (20, 60, 4096, [1, 2, 3]),
                                             (4, 10, 64, [1, 15, 16, 17, 257]), (2, 4, 16, [1, 63, 64, 65]),
                                             (30, 60, 256, [5, 1]), (20, 50, 256, [5, 1])])
def test_other_library_built_codes(oracle, k, n, ess, stripes):
    """k = 50 > 36: a tile is two items; ess 4096: a block is a quarter stripe; ess 64 and
    16: 16 and 64 stripes per block, on each side of it; the 4-compute-wave codes"""
    segs, refs = H.encode_segments(oracle, k, n, ess, stripes, k * 1000 + ess + 1)
    c = H.Ctx(k, n, ess)
    try:
        assert c.L.ec_encode_kernel_name(c.ctx).decode() in ("special", "straight-line")
        for parity_only in (False, True):
            H.run_batch(c, segs, refs, stripes, parity_only=parity_only)
        q, s = ctypes.c_ulonglong(), ctypes.c_ulonglong()
        assert c.L.ec_encoder_queue_stats(c.ctx, ctypes.byref(q), ctypes.byref(s)) == 0
        assert q.value + s.value == 2, "the library-built encoder's sized form took both batches"
    finally:
        c.close()


ROUTING_CHILD = r"""
import os, sys
sys.path.insert(0, {here!r})
import numpy as np, torch
import encode_sized_checked_child as H
from oracle import oracle as O
O.build()
for k, n, ess, stripes in ((10, 20, 256, [1, 9, 0, 70]), (3, 7, 64, [5, 1, 300]), (10, 50, 64, [3, 8200])):
    segs, refs = H.encode_segments(O, k, n, ess, stripes, k)
    c = H.Ctx(k, n, ess)
    for parity_only in (False, True):
        H.run_batch(c, segs, refs, stripes, parity_only=parity_only)
    c.close()
assert os.listdir(os.environ["UPLINK_EC_JIT_CACHE"]) == [], os.listdir(os.environ["UPLINK_EC_JIT_CACHE"])
print("ok")
"""


def test_codes_without_a_library_encoder(tmp_path):
    """RS(10,20) and RS(3,7): every segment goes on its own through the existing path, same
    results; so does RS(10,50), whose 8200-stripe segment (256 tiles, 40 parity rows) would
    start its encoder's compile as an ec_encode_segments call; the call starts no run-time compile (the JIT cache directory stays empty, no
    compile line in the log).  In a child process: the log and the cache are per process."""
    jit = tmp_path / "jit"
    jit.mkdir()
    env = dict(os.environ, UPLINK_EC_JIT_CACHE=str(jit), UPLINK_EC_LOG="1")
    r = subprocess.run([sys.executable, "-c", ROUTING_CHILD.format(here=HERE)], capture_output=True, text=True,
                       timeout=240, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "ok"
    assert "encoder: start" not in r.stderr + r.stdout and "hiprtc" not in r.stderr + r.stdout, r.stderr
    assert os.listdir(jit) == []


def test_share_size_that_is_no_multiple_of_16(oracle):
    segs, refs = H.encode_segments(oracle, 29, 80, 100, [3, 1, 12], 100)
    c = H.Ctx(29, 80, 100)
    try:
        H.run_batch(c, segs, refs, [3, 1, 12])
    finally:
        c.close()


@pytest.mark.parametrize("what", ["input", "pieces"])
def test_misaligned_segment_inside_an_aligned_batch(rs29, what):
    """an input 1 byte off 16-byte alignment / a piece buffer 8 bytes off: that segment on
    its own, the rest of the batch in the pass"""
    segs, refs, stripes = pick(rs29, [3, 5, 1, 7])
    shift = [0, 1 if what == "input" else 8, 0, 0]
    c = H.Ctx(29, 80, 256)
    try:
        H.run_batch(c, segs, refs, stripes, **({"in_shift": shift} if what == "input" else {"out_shift": shift}))
        q, s = ctypes.c_ulonglong(), ctypes.c_ulonglong()
        assert c.L.ec_encoder_queue_stats(c.ctx, ctypes.byref(q), ctypes.byref(s)) == 0
        assert q.value + s.value == 1, "the three aligned segments in one launch of the compile-time encoder"
    finally:
        c.close()


@pytest.mark.parametrize("parity_only", [False, True])
def test_equal_sizes_agree_with_encode_segments(oracle, parity_only):
    """3 x 9 stripes: byte for byte what ec_encode_segments(nseg = 3) writes"""
    k, n, ess, stripes = 29, 80, 256, [9, 9, 9]
    segs, refs = H.encode_segments(oracle, k, n, ess, stripes, 999)
    c = H.Ctx(k, n, ess)
    try:
        _, outs = H.run_batch(c, segs, refs, stripes, parity_only=parity_only)
        d_in = torch.from_numpy(np.concatenate(segs)).cuda()
        rows = n - k if parity_only else n
        d_out = torch.full((3, rows * 9 * ess), 0xCD, dtype=torch.uint8, device="cuda")
        rc = c.L.ec_encode_segments(c.ctx, d_in.data_ptr(), 3, 9, d_out.data_ptr(),
                                    N.EC_FLAG_PARITY_ONLY if parity_only else 0, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, N.strerror(rc)
        torch.cuda.synchronize()
        for g in range(3):
            assert torch.equal(outs.buf[outs.offs[g]:outs.offs[g] + outs.sizes[g]], d_out[g])
    finally:
        c.close()


def _pad_case(oracle, c, sizes, seed):
    """per size: (the buffer as given: data then 0xEE, the padded segment as ec_pad_segments
    makes it on a copy, stripes, the oracle's pieces of the padded segment)"""
    stripe = c.k * c.ess
    rng = np.random.default_rng(seed)
    f = oracle.FEC(c.k, c.n)
    given, padded, stripes, refs = [], [], [], []
    for size in sizes:
        total = size + 4 + (stripe - (size + 4) % stripe) % stripe
        buf = np.full(total, 0xEE, dtype=np.uint8)
        buf[:size] = rng.integers(0, 256, size, dtype=np.uint8)
        d = torch.from_numpy(buf).cuda()
        assert c.L.ec_pad_segments(d.data_ptr(), 1, 0, size, stripe, torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        p = d.cpu().numpy()
        assert np.array_equal(p[:size], buf[:size]) and int.from_bytes(p[-4:].tobytes(), "big") == total - size
        given.append(buf)
        padded.append(p)
        stripes.append(total // stripe)
        refs.append(f.encode_segment(p, c.ess, threads=8))
    return given, padded, stripes, refs


def test_padding(oracle):
    """data_len given for sizes 1, stripe-5, stripe-4, stripe-3, stripe, 3 stripe+17: each
    segment's tail is what ec_pad_segments writes on a copy, the pieces the oracle's encode of
    the padded segment; a data_len that does not match nstripes: EC_ERR_INVALID_ARG and nothing
    written"""
    c = H.Ctx(29, 80, 256)
    try:
        stripe = 29 * 256
        sizes = [1, stripe - 5, stripe - 4, stripe - 3, stripe, 3 * stripe + 17]
        given, padded, stripes, refs = _pad_case(oracle, c, sizes, 77)
        assert stripes == [1, 1, 1, 2, 2, 4]
        ins, outs = H.Ins(given), H.Outs(H.piece_sizes(c, stripes))
        rc = H.call_encode(c, ins.ptrs, stripes, outs.ptrs, data_len=sizes)
        assert rc == 0, N.strerror(rc)
        torch.cuda.synchronize()
        ins.check(padded)
        outs.check(H.expected(c, refs))
        # one stripe too many / too few for one segment of the batch: nothing is written
        for g, wrong in ((5, 5), (3, 1), (0, 2)):
            ins, outs = H.Ins(given), H.Outs(H.piece_sizes(c, stripes))
            bad = list(stripes)
            bad[g] = wrong
            assert H.call_encode(c, ins.ptrs, bad, outs.ptrs, data_len=sizes) == N.EC_ERR_INVALID_ARG
            torch.cuda.synchronize()
            ins.check(given)
            outs.check([None] * len(sizes))
    finally:
        c.close()


def test_padding_on_the_existing_path(oracle):
    """the same through the routed path (ess 100: ec_pad_segments, then the byte kernel)"""
    c = H.Ctx(29, 80, 100)
    try:
        sizes = [1, 2900 - 4, 2900 * 2 + 17]
        given, padded, stripes, refs = _pad_case(oracle, c, sizes, 78)
        ins, outs = H.Ins(given), H.Outs(H.piece_sizes(c, stripes))
        assert H.call_encode(c, ins.ptrs, stripes, outs.ptrs, data_len=sizes) == 0
        torch.cuda.synchronize()
        ins.check(padded)
        outs.check(H.expected(c, refs))
    finally:
        c.close()


def test_errors_write_nothing(rs29):
    segs, refs, stripes = pick(rs29, [2, 0, 4])
    c = H.Ctx(29, 80, 256)
    try:
        ins, outs = H.Ins(segs), H.Outs(H.piece_sizes(c, stripes))

        def untouched():
            torch.cuda.synchronize()
            ins.check(segs)
            outs.check([None] * 3)

        for which in ("segs", "pieces"):  # a NULL segs[g] / pieces[g] with nstripes[g] > 0
            ip, op = list(ins.ptrs), list(outs.ptrs)
            (ip if which == "segs" else op)[2] = None
            assert H.call_encode(c, ip, stripes, op) == N.EC_ERR_INVALID_ARG
            untouched()
        for null in ("segs", "nstripes", "pieces"):  # a NULL array
            assert H.call_encode(c, ins.ptrs, stripes, outs.ptrs, null=(null,)) == N.EC_ERR_INVALID_ARG
            untouched()
        assert H.call_encode(c, ins.ptrs, [4, 1, 1 << 62], outs.ptrs) == N.EC_ERR_UNSUPPORTED
        untouched()
        # a capturing stream: refused before anything is staged (begin and end around the call only)
        st = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=st, capture_error_mode="relaxed"):
            torch.zeros(1, device="cuda")  # (something for the graph to hold)
            rc = H.call_encode(c, ins.ptrs, stripes, outs.ptrs, stream=st)
        assert rc == N.EC_ERR_UNSUPPORTED
        untouched()
        assert c.L.ec_encode_segments_sized(c.ctx, 0, None, None, None, None, 0, None) == N.EC_OK
        assert H.call_encode(c, [None] * 3, [0, 0, 0], [None] * 3) == N.EC_OK
        untouched()
        # and the context still works
        assert H.call_encode(c, ins.ptrs, stripes, outs.ptrs) == 0
        torch.cuda.synchronize()
        outs.check(H.expected(c, refs))
    finally:
        c.close()


def test_more_segments_than_a_pass(oracle):
    """1100 one-stripe segments (8 MB) in one call: kPassSegs = 1024 is crossed"""
    k, n, ess, nseg = 29, 80, 256, 1100
    rng = np.random.default_rng(1100)
    data = rng.integers(0, 256, nseg * k * ess, dtype=np.uint8)
    # one stripe per segment: the pieces of all of them are one encode_segment of the concatenation
    ref = oracle.FEC(k, n).encode_segment(data, ess, threads=8).reshape(n, nseg, ess).transpose(1, 0, 2)
    d_in = torch.from_numpy(data).cuda()
    d_out = torch.full((nseg + 2, n * ess), 0xCD, dtype=torch.uint8, device="cuda")
    c = H.Ctx(k, n, ess)
    try:
        rc = H.call_encode(c, [d_in.data_ptr() + g * k * ess for g in range(nseg)], [1] * nseg,
                           [d_out[g + 1].data_ptr() for g in range(nseg)])
        assert rc == 0, N.strerror(rc)
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        assert np.array_equal(got[1:-1].reshape(nseg, n, ess), ref)
        assert (got[0] == 0xCD).all() and (got[-1] == 0xCD).all()
        assert torch.equal(d_in.cpu(), torch.from_numpy(data))
    finally:
        c.close()


def _varying_calls(c, rs29, count, seed, stream=None, errors=None):
    """`count` calls back to back on one stream with varying batches, each checked at the end"""
    try:
        rng = np.random.default_rng(seed)
        live = [i for i, s in enumerate(BLOCK) if s and s <= 41]
        runs = []
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            for _ in range(count):
                o = [int(x) for x in rng.choice(live, size=int(rng.integers(1, 5)), replace=False)]
                segs, refs, stripes = pick(rs29, o)
                ins, outs = H.Ins(segs), H.Outs(H.piece_sizes(c, stripes))
                rc = H.call_encode(c, ins.ptrs, stripes, outs.ptrs, stream=stream)
                assert rc == 0, N.strerror(rc)
                runs.append((ins, outs, segs, refs))
            (stream or torch.cuda.current_stream()).synchronize()
        for ins, outs, segs, refs in runs:
            outs.check(H.expected(c, refs))
            ins.check(segs)
    except BaseException as e:  # noqa: BLE001 - handed to the test's thread
        if errors is None:
            raise
        errors.append(e)


def test_calls_back_to_back(rs29):
    """40 calls on one stream with varying sizes, none waited for before the last: the
    staging blocks and the tile-queue pair are recycled in stream order"""
    c = H.Ctx(29, 80, 256)
    try:
        _varying_calls(c, rs29, 40, 40)
    finally:
        c.close()


def test_two_threads_two_streams(rs29):
    c = H.Ctx(29, 80, 256)
    try:
        errors = []
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        ts = [threading.Thread(target=_varying_calls, args=(c, rs29, 20, 200 + i, streams[i], errors)) for i in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errors, errors
    finally:
        c.close()


def test_round_trip_with_the_download_side():
    """uploads.encode_uploads on sizes 0, 1, 7419, 7420, 100000, then
    SegmentCodec.rebuild_segments_sized from a seeded random 29-subset per segment: each
    output is the padded buffer; upload_geometry agrees with the shapes returned"""
    from uplink_amd import eestream, uploads

    k, n, ess = 29, 80, 256
    scheme = eestream.RSScheme(eestream.new_fec(k, n), ess)
    try:
        rng = np.random.default_rng(10)
        sizes = [0, 1, 7419, 7420, 100000]
        geo = [uploads.upload_geometry(s, scheme) for s in sizes]
        assert [g[2] for g in geo] == [1, 1, 1, 1, 14]
        bufs = []
        for s, (padded, _, _) in zip(sizes, geo):
            b = np.full(padded, 0xEE, dtype=np.uint8)
            b[:s] = rng.integers(0, 256, s, dtype=np.uint8)
            bufs.append(torch.from_numpy(b).cuda())
        with pytest.raises(ValueError):
            uploads.encode_uploads(scheme, [(sizes[4], bufs[4]), (sizes[3], bufs[3][:-1])])
        pieces = uploads.encode_uploads(scheme, list(zip(sizes, bufs)))
        for p, (padded, piece_size, _) in zip(pieces, geo):
            assert tuple(p.shape) == (n, piece_size) and piece_size * k == padded
        stripe = k * ess
        for s, b, (padded, _, _) in zip(sizes, bufs, geo):
            h = b.cpu().numpy()
            p = padded - s
            assert 4 <= p <= stripe + 3 and (h[s:-4] == p % 256).all() and int.from_bytes(h[-4:].tobytes(), "big") == p
        par = uploads.encode_uploads(scheme, list(zip(sizes, bufs)), parity_only=True)
        for p, q in zip(pieces, par):
            assert torch.equal(p[k:], q)
        sets = []
        for p in pieces:
            nums = [int(x) for x in rng.permutation(n)[:k]]
            sets.append((nums, [p[x] for x in nums]))
        outs = [torch.full((g[0],), 0xCD, dtype=torch.uint8, device="cuda") for g in geo]
        eestream.SegmentCodec(scheme).rebuild_segments_sized(sets, [g[2] for g in geo], outs)
        torch.cuda.synchronize()
        for o, b in zip(outs, bufs):
            assert torch.equal(o, b)
    finally:
        torch.cuda.synchronize()
        scheme.close()
