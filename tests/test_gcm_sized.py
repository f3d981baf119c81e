"""GPU parity of AES-256-GCM with a size per segment (include/uplink_ec.h
ec_gcm_seal_segments_sized, ec_gcm_open_segments_sized; uplink_amd/encryption.py,
uploads.py, downloads.py): segments of different block counts, each under its own
key and nonce, sealed or opened in one call.  Expected bytes are oracle.aesgcm's
(encrypt_blocks, decrypt_blocks, encrypt_segment) over the test's own bytes, never
the engine's.  Device buffers are windows of one 0xCD-filled allocation with
64-byte guards, compared whole."""
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

import gcm_sized_checked_child as H  # noqa: E402

N = _native
IB = H.IN_BLOCK


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
def edge(ag):
    """the block-count batch (1, 3, 4, 5, 0, 8, 9, 41, 130 blocks of 7408 bytes) with the oracle's
    ciphertexts; shared, read-only"""
    return H.Batch(ag, H.EDGE_BLOCKS, IB, 20261021)


def test_checked_library(native):
    """First, so that an access of gcm_blocks_sized or of the pad launch outside a segment's
    declared extent, or a status store outside the status words, is skipped and reported by the
    bounds-checked build instead of reaching the card: a fresh process loads
    lib/checked/libuplink_ec_checked.so and runs the block-count batch (in order, reversed), the
    capped batch, the open and the open of corrupted blocks; a second one runs the block-count
    batch with a 1100-block segment added under UPLINK_GCM_GRID_PER_CU=1.  The two libraries must
    be one build."""
    child = [sys.executable, os.path.join(HERE, "gcm_sized_checked_child.py")]
    r = subprocess.run(child + ["--build-id"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    ident = r.stdout.split("build", 1)[1].split()[0]
    assert ident == native.ec_build_id().decode(), f"checked library build {ident} is not the product's: rebuild both"
    for args, env in (([], os.environ), (["capped"], dict(os.environ, UPLINK_GCM_GRID_PER_CU="1"))):
        r = subprocess.run(child + args, capture_output=True, text=True, timeout=240, env=env)
        assert "uplink_ec checked" not in r.stdout + r.stderr, r.stdout + r.stderr
        assert r.returncode == 0, r.stdout + r.stderr
        assert r.stdout.strip().splitlines()[-1] == "ok"


@pytest.mark.parametrize("reverse", [False, True])
def test_block_count_edges(edge, reverse):
    """1, 3, 4, 5, 0, 8, 9, 41 and 130 blocks in one seal: a wave short of a workgroup, one
    workgroup, one block over, ragged tails; the skipped segment has NULL pointers; one launch,
    one pass"""
    o = list(range(len(H.EDGE_BLOCKS)))
    b = edge.pick(o[::-1] if reverse else o)
    c = H.Ctx(29, 80, 256)
    try:
        ins, outs = H.run_seal(c, b)
        g0 = b.nblocks.index(0)
        assert ins.ptrs[g0] is None and outs.ptrs[g0] is None
        assert H.stats(c) == [1, 0, 1]
    finally:
        c.close()


@pytest.mark.parametrize("in_block", [16, 1008, 1024])
def test_ghash_shape_edges(ag, in_block):
    """in_block 16: 2 GHASH slots, one Horner step, 62 padding lanes; 1008: 64 slots, no padding
    lane, so lane 0 computes AES(K, J0) afterwards; 1024: 65 slots, two steps, 63 padding lanes"""
    b = H.Batch(ag, [1, 5, 9], in_block, 1000 + in_block)
    c = H.Ctx(29, 80, 256)
    try:
        H.run_seal(c, b)
        H.run_open(c, b)
    finally:
        c.close()


def test_capped_regime(ag):
    """40,000 blocks of 16 bytes beside 1, 5 and 700: more blocks than the target grid has waves
    (32,768), so the large segment's workgroups are its share of the grid and its waves run the
    stride loop more than once"""
    b = H.Batch(ag, H.CAPPED_BLOCKS, 16, 32)
    assert sum(b.nblocks) > 32768
    c = H.Ctx(29, 80, 256)
    try:
        H.run_seal(c, b)
        assert H.stats(c) == [1, 0, 1]
    finally:
        c.close()


def test_nonce_carry(ag):
    """nonce + b carries across the 32-bit words of the 12 bytes, and wraps silently at the top
    (encryption.Increment)"""
    nonces = [b"\xff" * 4 + b"\x00" * 8, b"\xff" * 8 + b"\x00" * 4, b"\xff" * 12]
    b = H.Batch(ag, [3, 3, 3], IB, 77, nonces=nonces)
    c = H.Ctx(29, 80, 256)
    try:
        H.run_seal(c, b)
        H.run_open(c, b)
    finally:
        c.close()


def test_open_and_failing_blocks(edge):
    """the oracle's ciphertext opens to the plaintext with every status -1, the skipped segment's
    too; then a tag bit in blocks 7 and 2 of the 9-block segment (two workgroups: status 2), a
    ciphertext bit in block 0 of the 1-block segment (0) and a tag bit in block 129 of the
    130-block segment (129): every other status is -1 and those segments' plaintext is right"""
    c = H.Ctx(29, 80, 256)
    try:
        dk = H.DevKeys(c.L, edge)
        H.run_open(c, edge, dk=dk)
        assert H.stats(c) == [0, 1, 1]
        cs, want = H.corrupted(edge)
        assert sorted(want) == [-1] * 6 + [0, 2, 129]
        H.run_open(c, edge, cs, want, dk=dk)
    finally:
        c.close()


DATA_SIZES = [0, 1, 7403, 7404, 7405, 100000]


def test_data_len(oracle, ag):
    """sizes 0 .. 100000 across the padding's residue edges, in buffers pre-filled with 0xEE:
    after the call each buffer is the oracle's pad of its data and each output the oracle's
    encrypt_segment; a wrong nblocks[g] in the middle of the list: EC_ERR_INVALID_ARG, nothing
    written"""
    rng = np.random.default_rng(5)
    datas = [rng.integers(0, 256, s, dtype=np.uint8) for s in DATA_SIZES]
    padded = [oracle.pad(d, IB) for d in datas]
    nblocks = [len(p) // IB for p in padded]
    assert nblocks == [1, 1, 1, 1, 2, 14]
    keys = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in datas]
    nonces = [rng.integers(0, 256, 24, dtype=np.uint8).tobytes() for _ in datas]
    want = [ag.encrypt_segment(d.tobytes(), k, n) for d, k, n in zip(datas, keys, nonces)]
    b = H.Batch.__new__(H.Batch)
    b.keys, b.nonces = keys, [n[:12] for n in nonces]
    c = H.Ctx(29, 80, 256)
    try:
        dk = H.DevKeys(c.L, b)
        filled = [np.concatenate([d, np.full(len(p) - len(d), 0xEE, np.uint8)]) for d, p in zip(datas, padded)]
        ins = H.Ins(filled)
        outs = H.Outs([len(w) for w in want])
        bad = list(nblocks)
        bad[3] = 2
        assert H.call_seal(c, ins.ptrs, bad, IB, dk, outs.ptrs, data_len=DATA_SIZES) == N.EC_ERR_INVALID_ARG
        torch.cuda.synchronize()
        outs.check([None] * len(want))
        ins.check(filled)
        assert H.stats(c) == [0, 0, 0]
        rc = H.call_seal(c, ins.ptrs, nblocks, IB, dk, outs.ptrs, data_len=DATA_SIZES)
        assert rc == 0, N.strerror(rc)
        torch.cuda.synchronize()
        ins.check(padded)
        outs.check(want)
        assert H.stats(c) == [1, 0, 1]
    finally:
        c.close()


def test_same_bytes_as_the_uniform_call(ag):
    """four segments of 9 blocks through ec_gcm_seal_segments and through the sized call: both
    the oracle's bytes"""
    b = H.Batch(ag, [9, 9, 9, 9], IB, 99)
    c = H.Ctx(29, 80, 256)
    try:
        dk = H.DevKeys(c.L, b)
        H.run_seal(c, b, dk=dk)
        plain = torch.from_numpy(np.concatenate(b.plains)).cuda()
        out = H.Outs([4 * 9 * (IB + 16)])
        rc = c.L.ec_gcm_seal_segments(plain.data_ptr(), 4, 9, IB, dk.keys.data_ptr(), dk.nonces.data_ptr(), out.ptrs[0],
                                      torch.cuda.current_stream().cuda_stream)
        assert rc == 0, N.strerror(rc)
        torch.cuda.synchronize()
        out.check([np.concatenate(b.ciphers)])
    finally:
        c.close()


def test_more_than_one_pass(ag):
    """4097 one-block segments of 16 bytes (4097 prepared keys): two passes, the same bytes, and
    all status words defined after the open"""
    nseg = 4097
    b = H.Batch(ag, [1] * nseg, 16, 4097)
    c = H.Ctx(29, 80, 256)
    try:
        dk = H.DevKeys(c.L, b)
        H.run_seal(c, b, dk=dk)
        assert H.stats(c) == [2, 0, 2]
        cs = [x.copy() for x in b.ciphers]
        cs[4096][20] ^= 1  # the one segment of the second pass: its tag
        H.run_open(c, b, cs, [-1] * 4096 + [0], dk=dk)
        assert H.stats(c) == [2, 2, 4]
    finally:
        c.close()


def test_argument_errors_write_nothing(edge):
    sel = [2, 6, 3, 0]  # 4, 9, 5 and 1 blocks
    b = edge.pick(sel)
    c = H.Ctx(29, 80, 256)
    try:
        dk = H.DevKeys(c.L, b)
        ins, outs = H.Ins(b.plains), H.Outs([len(x) for x in b.ciphers])
        cins, pouts, status = H.Ins(b.ciphers), H.Outs([len(x) for x in b.plains]), H.Outs([16])

        def untouched():
            torch.cuda.synchronize()
            outs.check([None] * 4)
            ins.check(b.plains)
            pouts.check([None] * 4)
            cins.check(b.ciphers)
            status.check([None])
            assert H.stats(c) == [0, 0, 0]

        bad, unsup = N.EC_ERR_INVALID_ARG, N.EC_ERR_UNSUPPORTED
        sp = status.ptrs[0]
        for which in ("in", "out"):  # a NULL pointer of a segment that is not skipped
            ip, op = list(ins.ptrs), list(outs.ptrs)
            (ip if which == "in" else op)[2] = None
            assert H.call_seal(c, ip, b.nblocks, IB, dk, op) == bad
            ip, op = list(cins.ptrs), list(pouts.ptrs)
            (ip if which == "in" else op)[2] = None
            assert H.call_open(c, ip, b.nblocks, IB, dk, op, sp) == bad
        for which in ("in", "out"):  # an odd pointer
            ip, op = list(ins.ptrs), list(outs.ptrs)
            (ip if which == "in" else op)[1] += 1
            assert H.call_seal(c, ip, b.nblocks, IB, dk, op) == unsup
            ip, op = list(cins.ptrs), list(pouts.ptrs)
            (ip if which == "in" else op)[1] += 8
            assert H.call_open(c, ip, b.nblocks, IB, dk, op, sp) == unsup
        for ib in (24, 0, (1 << 24) + 16):
            assert H.call_seal(c, ins.ptrs, b.nblocks, ib, dk, outs.ptrs) == unsup
            assert H.call_open(c, cins.ptrs, b.nblocks, ib, dk, pouts.ptrs, sp) == unsup
        assert H.call_seal(c, ins.ptrs, [4, 1 << 31, 5, 1], IB, dk, outs.ptrs) == unsup
        for name in ("plain", "nblocks", "keys", "nonces", "out"):
            assert H.call_seal(c, ins.ptrs, b.nblocks, IB, dk, outs.ptrs, null=(name,)) == bad
        for name in ("cipher", "nblocks", "keys", "nonces", "out", "status"):
            assert H.call_open(c, cins.ptrs, b.nblocks, IB, dk, pouts.ptrs, sp, null=(name,)) == bad
        st = torch.cuda.current_stream().cuda_stream
        assert c.L.ec_gcm_seal_segments_sized(c.ctx, 0, None, None, None, IB, None, None, None, st) == N.EC_OK
        assert c.L.ec_gcm_open_segments_sized(c.ctx, 0, None, None, IB, None, None, None, None, st) == N.EC_OK
        untouched()
        # a capturing stream: refused before anything is staged
        stream = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=stream, capture_error_mode="relaxed"):
            torch.zeros(1, device="cuda")  # (something for the graph to hold)
            rc = H.call_seal(c, ins.ptrs, b.nblocks, IB, dk, outs.ptrs, stream=stream)
            rc2 = H.call_open(c, cins.ptrs, b.nblocks, IB, dk, pouts.ptrs, sp, stream=stream)
        assert rc == unsup and rc2 == unsup
        untouched()
        # and the context still works
        assert H.call_seal(c, ins.ptrs, b.nblocks, IB, dk, outs.ptrs) == 0
        assert H.call_open(c, cins.ptrs, b.nblocks, IB, dk, pouts.ptrs, sp) == 0
        torch.cuda.synchronize()
        outs.check(b.ciphers)
        pouts.check(b.plains)
        status.check([np.full(4, -1, np.int32).view(np.uint8)])
        assert H.stats(c) == [1, 1, 2]
    finally:
        c.close()


def _seal_calls(c, edge, dk, count, seed, stream, errors):
    """`count` seal calls back to back on one stream over varying small lists, checked at the end"""
    try:
        small = [g for g, nb in enumerate(edge.nblocks) if 0 < nb <= 9]
        rng = np.random.default_rng(seed)
        runs = []
        with torch.cuda.stream(stream):
            for _ in range(count):
                o = sorted(int(x) for x in rng.choice(small, size=int(rng.integers(1, 6)), replace=False))
                # (sorted: segment g of the call uses key g; pad the list with skipped segments so
                # that every segment keeps its own key and nonce)
                nb = [edge.nblocks[g] if g in o else 0 for g in range(len(edge.nblocks))]
                ins = H.Ins([edge.plains[g] if g in o else edge.plains[4] for g in range(len(nb))])
                outs = H.Outs([len(edge.ciphers[g]) if g in o else 0 for g in range(len(nb))])
                rc = H.call_seal(c, ins.ptrs, nb, IB, dk, outs.ptrs, stream=stream)
                assert rc == 0, N.strerror(rc)
                runs.append((ins, outs, o))
            stream.synchronize()
        for ins, outs, o in runs:
            outs.check([edge.ciphers[g] if g in o else np.zeros(0, np.uint8) for g in range(len(edge.nblocks))])
    except BaseException as e:  # noqa: BLE001 - handed to the test's thread
        errors.append(e)


def test_staging_reuse_two_threads_two_streams(edge):
    """two threads on two streams, 50 seal calls each of different small lists on one context,
    none waited for before the last: the staging blocks are recycled behind their events"""
    c = H.Ctx(29, 80, 256)
    try:
        dk = H.DevKeys(c.L, edge)
        torch.cuda.synchronize()
        errors = []
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        ts = [threading.Thread(target=_seal_calls, args=(c, edge, dk, 50, 700 + i, streams[i], errors))
              for i in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errors, errors
        assert H.stats(c) == [100, 0, 100]
    finally:
        c.close()


def test_python_surface(oracle, ag):
    """seal_uploads -> encode_uploads(hash_pieces=True) on sizes 0, 1, 7404, 7405, 100000 equals
    the chained oracles (encrypt_segment, pad to the stripe, FEC.encode_segment, blake3_many);
    decode_downloads from k parity pieces -> open_downloads returns the original bytes with
    status all -1; one corrupted tag raises DecryptionFailed with its block under check=True"""
    from oracle import blake3 as ob
    from uplink_amd import downloads, eestream, encryption, uploads

    k, n, ess = 29, 80, 256
    scheme = eestream.RSScheme(eestream.new_fec(k, n), ess)
    try:
        rng = np.random.default_rng(13)
        sizes = [0, 1, 7404, 7405, 100000]
        datas = [rng.integers(0, 256, s, dtype=np.uint8) for s in sizes]
        keys = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in sizes]
        nonces = [rng.integers(0, 256, 24, dtype=np.uint8).tobytes() for _ in sizes]
        dev_keys = encryption.prepare_keys(keys)
        dev_nonces = torch.from_numpy(np.frombuffer(b"".join(x[:12] for x in nonces), dtype=np.uint8).copy()).cuda()
        bufs = []
        for s, d in zip(sizes, datas):
            _, plain_cap, _ = uploads.cipher_geometry(s)
            h = np.full(plain_cap, 0xEE, dtype=np.uint8)
            h[:s] = d
            bufs.append(torch.from_numpy(h).cuda())
        with pytest.raises(ValueError):  # a short buffer: before anything is queued
            uploads.seal_uploads(scheme, [(sizes[3], bufs[2])], dev_keys, dev_nonces)
        sealed = uploads.seal_uploads(scheme, list(zip(sizes, bufs)), dev_keys, dev_nonces)
        pieces, hashes = uploads.encode_uploads(scheme, sealed, hash_pieces=True)
        torch.cuda.synchronize()
        f = oracle.FEC(k, n)
        encs = []
        for g, s in enumerate(sizes):
            enc = ag.encrypt_segment(datas[g].tobytes(), keys[g], nonces[g])
            assert sealed[g][0] == len(enc) == uploads.cipher_geometry(s)[2]
            assert sealed[g][1].numel() == uploads.upload_geometry(len(enc), scheme)[0]
            ref = f.encode_segment(oracle.pad(enc, k * ess), ess, threads=8)
            assert np.array_equal(sealed[g][1].cpu().numpy(), oracle.pad(enc, k * ess)), g
            assert np.array_equal(pieces[g].cpu().numpy(), ref), g
            assert np.array_equal(hashes[g].cpu().numpy(), ob.blake3_many(np.ascontiguousarray(ref), threads=8)), g
            encs.append(enc)
        # the download: k parity pieces each, decoded to enc_len bytes, then opened
        # (a download of enc_len bytes is whole stripes: its pieces are the upload's without the
        # stripe PadReader added)
        nums = list(range(n - k, n))
        ps = [downloads.segment_geometry(len(e), scheme)[1] for e in encs]
        got = downloads.decode_downloads(scheme, [(len(e), {i: pieces[g][i][:ps[g]] for i in nums})
                                                  for g, e in enumerate(encs)])
        plains, status = downloads.open_downloads(scheme, list(zip(sizes, got)), dev_keys, dev_nonces, check=True)
        assert status.cpu().tolist() == [-1] * len(sizes)
        for g, s in enumerate(sizes):
            assert plains[g].numel() == s and np.array_equal(plains[g].cpu().numpy(), datas[g]), g
        with pytest.raises(ValueError):  # an encrypted segment of another length
            downloads.open_downloads(scheme, [(sizes[2], got[3])], dev_keys, dev_nonces)
        bad = [t.clone() for t in got]
        bad[4][5 * 7424 + 7408 + 2] ^= 4  # the tag of block 5 of the 100000-byte download
        plains, status = downloads.open_downloads(scheme, list(zip(sizes, bad)), dev_keys, dev_nonces)
        assert status.cpu().tolist() == [-1, -1, -1, -1, 5]
        with pytest.raises(encryption.DecryptionFailed) as e:
            downloads.open_downloads(scheme, list(zip(sizes, bad)), dev_keys, dev_nonces, check=True)
        assert e.value.block == 5
    finally:
        torch.cuda.synchronize()
        scheme.close()
