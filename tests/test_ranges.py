"""GPU parity of ranged downloads (include/uplink_ec.h ec_gcm_open_ranges_sized;
uplink_amd/downloads.py decode_ranges, open_ranges, download_ranges): byte ranges
of many segments opened in one call, each under its own key, nonce and first
block, every covered block authenticated whole and only the wanted bytes stored,
at any alignment.  Expected bytes are oracle.aesgcm's over the test's own bytes --
decrypt_blocks(key, increment(nonce, fb), covered blocks, ib)[head : head+len] --
never the engine's.  Device buffers are windows of one 0xCD-filled allocation
with 64-byte guards, compared whole."""
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

import gcm_sized_checked_child as G  # noqa: E402
import ranges_checked_child as H  # noqa: E402

N = _native
IB = H.IB


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)


@pytest.fixture(scope="module")
def ag(oracle):
    from oracle import aesgcm
    return aesgcm


@pytest.fixture(scope="module")
def cut(ag):
    """the cut-edge batch (H.cut_edge_specs) with the oracle's ciphertexts and expected outputs;
    shared, read-only"""
    return H.Ranges(ag, H.cut_edge_specs(), IB, 20261022)


def test_checked_library(native):
    """First, so that a load of gcm_open_ranged outside the nb*B bytes of a segment's covered
    blocks, a store outside the `length` bytes of its output or a status store outside the status
    words is skipped and reported by the bounds-checked build instead of reaching the card: a
    fresh process loads lib/checked/libuplink_ec_checked.so and runs the cut-edge batch (aligned,
    at window offsets 1, 8 and 15, and mixed) and the failing-block batch.  The two libraries must
    be one build."""
    child = [sys.executable, os.path.join(HERE, "ranges_checked_child.py")]
    r = subprocess.run(child + ["--build-id"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    ident = r.stdout.split("build", 1)[1].split()[0]
    assert ident == native.ec_build_id().decode(), f"checked library build {ident} is not the product's: rebuild both"
    r = subprocess.run(child, capture_output=True, text=True, timeout=240)
    assert "uplink_ec checked" not in r.stdout + r.stderr, r.stdout + r.stderr
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "ok"


def test_cut_edges_one_call(cut):
    """heads 0, 1, 15, 16, 17 and 7407 crossed with ends on, 1 past and 1 short of a block boundary;
    lengths 0, 1, 2 inside a 16-byte slot, across a slot boundary and across a block boundary;
    ranges inside one block, across two, across all six and a whole 6-block segment; first blocks
    0, 1 and 3 -- aligned and bytewise segments in one launch, one pass"""
    assert {0, 1, 15, 16, 17, IB - 1} <= set(cut.head) and {0, 1, 3} == set(cut.fb)
    assert {0, 1, 2, 3, 6} <= set(cut.nblocks) and 0 in cut.length
    c = H.Ctx(29, 80, 256)
    try:
        outs, _ = H.run_ranges(c, cut)
        g0 = cut.nblocks.index(0)
        assert outs.ptrs[g0] is None
        assert H.stats(c) == [1, 1]
        assert G.stats(c) == [0, 0, 0]  # the sized calls' counters do not move
    finally:
        c.close()


@pytest.mark.parametrize("in_block", [16, 1008, 1024])
def test_ghash_shape_edges(ag, in_block):
    """in_block 16: 2 GHASH slots, one Horner step, 62 padding lanes; 1008: 64 slots, no padding
    lane, so lane 0 computes AES(K, J0) afterwards; 1024: 65 slots, two steps, 63 padding lanes
    (test_gcm_sized.test_ghash_shape_edges).  1, 5 and 9 covered blocks, head and tail mid-slot
    (at in_block 16 the one block's head and tail share its only slot)."""
    specs = []
    for g, nb in enumerate([1, 5, 9]):
        head = 5 if in_block == 16 else 21
        tail = 3 if in_block == 16 else 27  # bytes of the last block left out
        specs.append(((0, 1, 3)[g], head, nb * in_block - head - tail))
    b = H.Ranges(ag, specs, in_block, 2000 + in_block)
    assert b.nblocks == [1, 5, 9]
    c = H.Ctx(29, 80, 256)
    try:
        H.run_ranges(c, b)
        H.run_ranges(c, b, 8, 1)
    finally:
        c.close()


@pytest.mark.parametrize("in_shift,out_shift", [(1, 0), (0, 1), (8, 8), (15, 15), (1, 15), (15, 8),
                                                (("mix", 1, 0), ("mix", 4, 0))])
def test_alignment(cut, in_shift, out_shift):
    """the cut-edge batch with its source and output windows 1, 8 and 15 bytes past a 16-byte
    boundary (and, mixed, every pair of 0, 1, 8, 15 in one call): the same bytes as with everything
    aligned, which is the expected output of both"""
    c = H.Ctx(29, 80, 256)
    try:
        dk = H.DevKeys(c.L, cut)
        aligned, _ = H.run_ranges(c, cut, dk=dk)
        shifted, _ = H.run_ranges(c, cut, in_shift, out_shift, dk=dk)
        a, s = aligned.buf.cpu().numpy(), shifted.buf.cpu().numpy()
        for g, n in enumerate(cut.length):
            assert np.array_equal(a[aligned.offs[g]:aligned.offs[g] + n], s[shifted.offs[g]:shifted.offs[g] + n]), g
        assert H.stats(c) == [2, 2]
    finally:
        c.close()


def test_nonce_carry_through_first_block(ag):
    """nonce + (first block + r) carries across the 32-bit words of the 12 bytes and wraps silently
    at the top (encryption.Increment): the expected bytes are sealed under the oracle's increment"""
    nonces = [b"\xff" * 4 + b"\x00" * 8, b"\xff" * 8 + b"\x00" * 4, b"\xff" * 12]
    specs = [(fb, 9, 3 * IB - 9 - 11) for fb in (0, 1) for _ in nonces]
    b = H.Ranges(ag, specs, IB, 78, nonces=nonces * 2)
    assert b.nblocks == [3] * 6
    c = H.Ctx(29, 80, 256)
    try:
        H.run_ranges(c, b)
    finally:
        c.close()


def test_failing_blocks(cut):
    """a tag bit in a covered block inside the wanted bytes; a ciphertext bit in a covered block
    OUTSIDE the wanted bytes (before the head, and behind the end): the status is still that
    block's absolute number; two bad blocks: the smaller absolute number; every other range of
    the call ends with -1 and the right plaintext"""
    c = H.Ctx(29, 80, 256)
    try:
        dk = H.DevKeys(c.L, cut)
        cs, want = H.corrupted(cut)
        assert sum(x >= 0 for x in want) == 4
        H.run_ranges(c, cut, ciphers=cs, want_status=want, dk=dk)
        H.run_ranges(c, cut, 8, 1, ciphers=cs, want_status=want, dk=dk)
    finally:
        c.close()


def test_whole_segments_equal_the_sized_open(ag):
    """first block 0, head 0 and length nb*ib: outputs and status byte-identical to
    ec_gcm_open_segments_sized on the same inputs, clean and with a failing block"""
    b = H.Ranges(ag, [(0, 0, nb * IB) for nb in (1, 3, 5, 9)], IB, 91)
    c = H.Ctx(29, 80, 256)
    try:
        dk = H.DevKeys(c.L, b)
        for damage in (False, True):
            cs = [x.copy() for x in b.ciphers]
            want = [-1] * 4
            if damage:
                cs[2][3 * (IB + 16) + 50] ^= 2
                want[2] = 3
            ranged, rstatus = H.run_ranges(c, b, ciphers=cs, want_status=want, dk=dk)
            ins = H.Ins(cs)
            outs = H.Outs(b.length)
            status = H.Outs([16])
            rc = G.call_open(c, ins.ptrs, b.nblocks, IB, dk, outs.ptrs, status.ptrs[0])
            assert rc == 0, N.strerror(rc)
            torch.cuda.synchronize()
            assert torch.equal(status.buf, rstatus.buf)
            assert torch.equal(outs.buf, ranged.buf)
    finally:
        c.close()


def test_more_than_one_pass(ag):
    """4097 one-block ranges of in_block 16 (4097 prepared keys): two passes, all status words
    defined; the one range of the second pass fails with its absolute block number"""
    rng = np.random.default_rng(4097)
    specs = []
    for g in range(4097):
        head = int(rng.integers(0, 16))
        specs.append(((0, 1, 3)[g % 3], head, int(rng.integers(1, 17 - head))))
    b = H.Ranges(ag, specs, 16, 4098)
    assert b.nblocks == [1] * 4097
    c = H.Ctx(29, 80, 256)
    try:
        dk = H.DevKeys(c.L, b)
        H.run_ranges(c, b, dk=dk)
        assert H.stats(c) == [2, 2]
        cs = [x.copy() for x in b.ciphers]
        cs[4096][20] ^= 1  # its tag
        H.run_ranges(c, b, ciphers=cs, want_status=[-1] * 4096 + [b.fb[4096]], dk=dk)
        assert H.stats(c) == [4, 4]
    finally:
        c.close()


def test_capped_regime(ag):
    """one 40,000-block range of in_block 16 beside ranges of 1, 5 and 700 blocks: more blocks than
    the target grid has waves (32,768), so the large range's waves run the stride loop more than
    once; its head and tail are cut mid-slot"""
    specs = [(0, 3, 9), (1, 3, 40000 * 16 - 3 - 5), (3, 0, 5 * 16), (0, 15, 700 * 16 - 15 - 15)]
    b = H.Ranges(ag, specs, 16, 33)
    assert b.nblocks == [1, 40000, 5, 700] and sum(b.nblocks) > 32768
    c = H.Ctx(29, 80, 256)
    try:
        H.run_ranges(c, b)
        assert H.stats(c) == [1, 1]
    finally:
        c.close()


def test_argument_errors_write_nothing(cut):
    sel = [0, 4, 10, 25]  # 2, 3, 3 and 1 covered blocks
    b = cut.pick(sel)
    assert b.nblocks == [2, 3, 3, 1]
    c = H.Ctx(29, 80, 256)
    try:
        dk = H.DevKeys(c.L, b)
        ins, outs, status = H.Ins(b.ciphers), H.Outs(b.length), H.Outs([16])
        sp = status.ptrs[0]

        def call(fb=b.fb, nb=b.nblocks, head=b.head, length=b.length, ib=IB, ip=ins.ptrs, op=outs.ptrs, **kw):
            return H.call_ranges(c, ip, fb, nb, head, length, ib, dk, op, sp, **kw)

        def untouched():
            torch.cuda.synchronize()
            outs.check([None] * 4)
            ins.check(b.ciphers)
            status.check([None])
            assert H.stats(c) == [0, 0]

        bad, unsup = N.EC_ERR_INVALID_ARG, N.EC_ERR_UNSUPPORTED

        def with_(lst, i, v):
            lst = list(lst)
            lst[i] = v
            return lst

        # EC_ERR_INVALID_ARG
        assert call(head=with_(b.head, 1, IB)) == bad                        # head >= in_block
        assert call(head=with_(b.head, 1, IB + 5)) == bad
        assert call(nb=with_(b.nblocks, 2, 2)) == bad                        # one block short of the cover
        assert call(nb=with_(b.nblocks, 2, 4)) == bad                        # one more than the cover
        assert call(nb=with_(b.nblocks, 3, 0)) == bad                        # 0 blocks with a length
        assert call(length=with_(b.length, 0, b.length[0] + 1)) == bad       # a length that needs one more block
        assert call(length=with_(b.length, 3, 0)) == bad                     # a block with no length
        assert call(length=with_(b.length, 3, (1 << 64) - 1)) == bad         # head + length wraps
        assert call(ip=with_(ins.ptrs, 2, None)) == bad                      # a NULL pointer of a segment not skipped
        assert call(op=with_(outs.ptrs, 2, None)) == bad
        for name in ("cipher", "first_block", "nblocks", "head", "length", "keys", "nonces", "out", "status"):
            assert call(null=(name,)) == bad, name
        # EC_ERR_UNSUPPORTED
        assert call(fb=with_(b.fb, 1, 0x7FFFFFFF - 2)) == unsup              # first block + 3 blocks = 0x80000000
        assert call(fb=with_(b.fb, 1, 1 << 40)) == unsup
        for ib in (24, 0, (1 << 24) + 16):
            assert call(ib=ib, head=[0] * 4) in (unsup,), ib
        st = torch.cuda.current_stream().cuda_stream
        assert c.L.ec_gcm_open_ranges_sized(c.ctx, 0, None, None, None, None, None, IB, None, None, None, None,
                                            st) == N.EC_OK
        untouched()
        # a capturing stream: refused before anything is staged
        stream = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=stream, capture_error_mode="relaxed"):
            torch.zeros(1, device="cuda")  # (something for the graph to hold)
            rc = call(stream=stream)
        assert rc == unsup
        untouched()
        # the largest first block that is supported, and the context still works
        assert call(fb=with_(b.fb, 3, 0x7FFFFFFF - 1)) == 0
        torch.cuda.synchronize()
        # (sealed under another nonce: its one block fails, with the largest block number there is)
        status.check([np.array([-1, -1, -1, 0x7FFFFFFE], dtype=np.int32).view(np.uint8)])
        assert call() == 0
        torch.cuda.synchronize()
        outs.check(b.want)
        ins.check(b.ciphers)
        status.check([np.full(4, -1, np.int32).view(np.uint8)])
        assert H.stats(c) == [2, 2]
    finally:
        c.close()


def _range_calls(c, cut, dk, count, seed, stream, errors):
    """`count` calls back to back on one stream over varying small lists, checked at the end"""
    try:
        small = [g for g, nb in enumerate(cut.nblocks) if 0 < nb <= 3]
        rng = np.random.default_rng(seed)
        runs = []
        with torch.cuda.stream(stream):
            for _ in range(count):
                o = sorted(int(x) for x in rng.choice(small, size=int(rng.integers(1, 6)), replace=False))
                # (segment g of the call uses key g: the others are skipped, 0 blocks and 0 bytes)
                on = lambda v, z=0: [v[g] if g in o else z for g in range(len(cut))]  # noqa: E731
                ins = H.Ins(on(cut.ciphers, np.zeros(0, np.uint8)), H.shifts(len(cut), ("mix", 1, 0)))
                outs = H.Outs(on(cut.length), H.shifts(len(cut), ("mix", 4, 0)))
                status = H.Outs([4 * len(cut)])
                rc = H.call_ranges(c, ins.ptrs, cut.fb, on(cut.nblocks), on(cut.head), on(cut.length), IB, dk,
                                   outs.ptrs, status.ptrs[0], stream=stream)
                assert rc == 0, N.strerror(rc)
                runs.append((ins, outs, status, o))
            stream.synchronize()
        for ins, outs, status, o in runs:
            outs.check([cut.want[g] if g in o else np.zeros(0, np.uint8) for g in range(len(cut))])
            status.check([np.full(len(cut), -1, np.int32).view(np.uint8)])
    except BaseException as e:  # noqa: BLE001 - handed to the test's thread
        errors.append(e)


def test_staging_reuse_two_threads_two_streams(cut):
    """two threads on two streams, 50 calls each of different small lists on one context, none
    waited for before the last: the staging blocks are recycled behind their events"""
    c = H.Ctx(29, 80, 256)
    try:
        dk = H.DevKeys(c.L, cut)
        torch.cuda.synchronize()
        errors = []
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        ts = [threading.Thread(target=_range_calls, args=(c, cut, dk, 50, 800 + i, streams[i], errors))
              for i in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errors, errors
        assert H.stats(c) == [100, 100]
    finally:
        c.close()


SCHEMES = [(29, 80, 256, 7424), (4, 10, 256, 1040), (3, 7, 8, 32)]


@pytest.mark.parametrize("k,n,ess,block", SCHEMES)
def test_python_end_to_end(oracle, ag, k, n, ess, block):
    """segments of 0, 1, 7404, 7405 and 100,000 plaintext bytes, encrypted by the oracle and
    encoded by oracle.FEC; the test hands over only the piece RANGES (copies of the slices) of a
    random share set of k per download, and download_ranges must return plaintext[off:off+len] for
    (0, 1), (0, P), (P-1, 1), (ib-1, 2), three blocks from the middle, the last block with the
    bytes next to the padding, and (x, 0).  RS(29,80) ess 256 B 7424: blocks equal stripes;
    RS(4,10) ess 256 B 1040: blocks straddle stripes, skip a non-zero multiple of 16; RS(3,7)
    ess 8 B 32: skip 8, the misaligned source.  A second run uses error_detection with k+2 shares
    and one corrupted byte inside a piece range."""
    from uplink_amd import downloads, eestream, encryption

    ib = block - 16
    scheme = eestream.RSScheme(eestream.new_fec(k, n), ess)
    try:
        rng = np.random.default_rng(1000 + k)
        f = oracle.FEC(k, n)
        stripe = k * ess
        sizes = [0, 1, 7404, 7405, 100000]
        items = []  # (segment, P, off, len)
        datas, pieces_of, keys, nonces = [], [], [], []
        for s, P in enumerate(sizes):
            data = rng.integers(0, 256, P, dtype=np.uint8)
            key = rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
            nonce = rng.integers(0, 256, 24, dtype=np.uint8).tobytes()
            enc = ag.encrypt_segment(data.tobytes(), key, nonce, block)
            enc = np.frombuffer(bytes(enc), dtype=np.uint8)
            assert len(enc) % block == 0
            nblocks = len(enc) // block
            last = max(P - 1, 0) // ib  # the last block that holds data: its tail is next to the padding
            padded = oracle.pad(enc, stripe)
            pieces_of.append(f.encode_segment(padded, ess, threads=8))
            datas.append(data)
            cand = [(0, 1), (0, P), (P - 1, 1), (ib - 1, 2), ((nblocks // 2 - 1) * ib + 7, 3 * ib - 9),
                    (last * ib, P - last * ib), (P // 2, 0), (P, 0)]
            for off, length in cand:
                if off >= 0 and length >= 0 and off + length <= P:
                    items.append((s, P, off, length))
                    keys.append(key)
                    nonces.append(nonce[:12])
        assert len(items) > 20
        dev_keys = encryption.prepare_keys(keys)
        dev_nonces = torch.from_numpy(np.frombuffer(b"".join(nonces), dtype=np.uint8).copy()).cuda()
        geos = [downloads.range_geometry(P, off, length, scheme, block) for _, P, off, length in items]
        if block == 1040:
            assert any(g.skip and g.skip % 16 == 0 for g in geos)
        if block == 32:
            assert any(g.skip == 8 for g in geos)
        if block == 7424:
            assert all(g.skip == 0 for g in geos)

        def fetch(extra, damage):
            ranges = []
            for i, ((s, _, _, _), g) in enumerate(zip(items, geos)):
                nums = [int(x) for x in rng.permutation(n)[:k + extra]]
                sl = {x: torch.from_numpy(np.array(pieces_of[s][x][g.piece_offset:g.piece_offset + g.piece_length]))
                      .cuda() for x in nums}
                if damage is not None and i == damage and g.piece_length:
                    sl[nums[1]][g.piece_length // 2] ^= 0x5A
                ranges.append((g, sl))
            return ranges

        with pytest.raises(Exception):  # a piece range of another length: as EC_ERR_SHARE_SIZE
            g = next(g for g in geos if g.piece_length)
            downloads.decode_ranges(scheme, [(g, {0: torch.zeros(g.piece_length + ess, dtype=torch.uint8,
                                                                 device="cuda")})])
        big = next(i for i, g in enumerate(geos) if g.nblocks >= 3)
        for extra, damage, detect in ((0, None, False), (2, big, True)):
            plains, status = downloads.download_ranges(scheme, fetch(extra, damage), dev_keys, dev_nonces,
                                                       block_size=block, error_detection=detect, check=True)
            assert status.cpu().tolist() == [-1] * len(items)
            for (s, _, off, length), got in zip(items, plains):
                assert got.numel() == length
                assert np.array_equal(got.cpu().numpy(), datas[s][off:off + length]), (s, off, length)
        # a flipped ciphertext bit outside the wanted bytes of a covered block still fails the download
        encs = downloads.decode_ranges(scheme, fetch(0, None))
        g = geos[big]
        assert g.head + g.length < g.nblocks * ib
        encs = [e.clone() for e in encs]
        encs[big][(g.nblocks - 1) * block + ib - 1] ^= 1  # the last plaintext byte of the last covered block
        with pytest.raises(encryption.DecryptionFailed) as e:
            downloads.open_ranges(scheme, list(zip(geos, encs)), dev_keys, dev_nonces, block_size=block, check=True)
        assert e.value.block == g.first_block + g.nblocks - 1
    finally:
        torch.cuda.synchronize()
        scheme.close()
