"""GPU parity of the one-shot message cipher (include/uplink_ec.h
ec_gcm_seal_messages / ec_gcm_open_messages; uplink_amd/encryption.py encrypt,
decrypt, encrypt_key, decrypt_key; uploads.seal_inline_uploads;
downloads.open_content_keys, open_inline_downloads): lists of messages, each
under its own raw 32-byte key and nonce, sealed or opened in one call with nothing
prepared on the host.  Expected bytes are oracle.aesgcm's seal / open_ over the
test's own bytes and the GCM specification's vectors -- never the engine's.
Device buffers are windows of one 0xCD-filled allocation with 64-byte guards,
compared whole."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from uplink_amd import _native, downloads, encryption, uploads  # noqa: E402

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import messages_checked_child as M  # noqa: E402

N = _native


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
def boundary(ag):
    """every boundary length at every pair of window shifts, sealed by the oracle; shared, read-only"""
    return M.boundary_batch(ag)


@pytest.fixture()
def ctx(native):
    c = M.Ctx(29, 80, 256)
    yield c
    c.close()


def test_checked_library(native):
    """First, so that a load of gcm_messages outside a message's input, a store outside its output
    or a status store outside the status words is skipped and reported by the bounds-checked build
    instead of reaching the card: a fresh process loads lib/checked/libuplink_ec_checked.so and
    runs the boundary batch (seal and open) and the tamper batch.  The two libraries must be one
    build."""
    child = [sys.executable, os.path.join(HERE, "messages_checked_child.py")]
    r = subprocess.run(child + ["--build-id"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    ident = r.stdout.split("build", 1)[1].split()[0]
    assert ident == native.ec_build_id().decode(), f"checked library build {ident} is not the product's: rebuild both"
    r = subprocess.run(child, capture_output=True, text=True, timeout=240)
    assert "uplink_ec checked" not in r.stdout + r.stderr, r.stdout + r.stderr
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "ok"


def test_spec_vectors(ctx):
    """test cases 13, 14 and 15 of the GCM specification (AES-256, no AAD; plaintexts of 0, 16 and
    64 bytes) through the seal, ct || tag compared exactly, and back through the open, status 0"""
    b = M.Messages.of(M.spec_cases())
    M.run_seal(ctx, b)
    M.run_open(ctx, b)
    seal, open_, passes, per = M.stats(ctx)
    assert (seal, open_, passes) == (1, 1, 2) and per >= 1


def test_boundary_lengths_at_every_alignment(ctx, boundary):
    """One seal call and one open call over M.BOUNDARY_LENGTHS -- the issue's lengths and this lane
    layout's own: 2032 / 2033 (two rounds per lane to three) and 49, 112 / 113, 240 / 241, 496 /
    497 (a further step of the pairwise combination starts at 5, 9, 17 and 33 live lanes) -- each at
    every pair of source and output shifts 0, 1, 8, 15; the key and nonce arrays sit 5 bytes past
    a 16-byte boundary.  Outputs, inputs and guards compared whole."""
    M.run_boundary(ctx, boundary)


@pytest.mark.parametrize("count", [1, 3, 5])
def test_counts_that_do_not_fill_a_workgroup(ctx, boundary, count):
    b = boundary[0]
    pick = [g for g in range(len(b)) if b.lens[g] in (33, 1009, 4097)][::16][:3]
    order = (pick + [0, 200])[:count]
    sub = b.pick(order)
    M.run_seal(ctx, sub, ("mix", 1, 1), ("mix", 1, 3))
    M.run_open(ctx, sub, ("mix", 1, 2), ("mix", 1, 0))


def test_longest_message(ctx, ag):
    """1 << 24 bytes, the longest a message may be, beside a short one: 16385 rounds per lane
    through the same body (source aligned, output 1 byte past alignment), sealed and opened"""
    b = M.Messages(ag, [1 << 24, 5], 20261102)
    M.run_seal(ctx, b, 0, 1)
    M.run_open(ctx, b, 0, 1)


def test_tampered_messages_fail_alone(ctx, ag):
    """M.tampered: each tampered message ends with status 1 and len zero bytes, its neighbours with
    status 0 and their plaintext; guards intact"""
    b, sealed, keys, nonces, want = M.tampered(ag)
    assert sum(want) == 6
    for s_in, s_out in ((0, 0), (("mix", 1, 1), ("mix", 1, 3))):
        M.run_open(ctx, b, s_in, s_out, sealed=sealed, want_status=want, dk=M.DevKeys(b, 0, keys, nonces))
    M.run_open(ctx, b)  # untampered: all 0


def test_pass_boundary(ctx, ag):
    """2 * pass_messages + 1 messages of lengths cycling 0..47: three passes per call, all compared
    with the oracle"""
    per = M.stats(ctx)[3]
    n = 2 * per + 1
    b = M.Messages(ag, [g % 48 for g in range(n)], 20261028)
    before = M.stats(ctx)
    M.run_seal(ctx, b, ("mix", 3, 0), ("mix", 5, 1))
    mid = M.stats(ctx)
    assert mid[2] - before[2] == 3 and mid[0] - before[0] == 3 and mid[1] == before[1]
    M.run_open(ctx, b, ("mix", 5, 2), ("mix", 3, 3))
    after = M.stats(ctx)
    assert after[2] - mid[2] == 3 and after[1] - mid[1] == 3 and after[0] == mid[0]


def test_argument_errors_leave_everything_untouched(ctx, ag):
    b = M.Messages(ag, [48, 0, 17], 20261029)
    dk = M.DevKeys(b)
    ins, cins = M.Ins(b.plains), M.Ins(b.sealed)
    outs, plains = M.Outs([len(x) for x in b.sealed]), M.Outs(b.lens)
    status = M.Outs([4 * len(b)])
    bad, unsup = N.EC_ERR_INVALID_ARG, N.EC_ERR_UNSUPPORTED
    for null in ("in", "len", "keys", "nonces", "out"):
        assert M.call_seal(ctx, ins.ptrs, b.lens, dk, outs.ptrs, null=(null,)) == bad, null
        assert M.call_open(ctx, cins.ptrs, b.lens, dk, plains.ptrs, status.ptrs[0], null=(null,)) == bad, null
    assert M.call_open(ctx, cins.ptrs, b.lens, dk, plains.ptrs, status.ptrs[0], null=("status",)) == bad
    # a NULL pointer the rules do not allow: the plaintext of a non-empty message, any sealed side
    assert M.call_seal(ctx, [ins.ptrs[0], None, None], b.lens, dk, outs.ptrs) == bad
    assert M.call_seal(ctx, ins.ptrs, b.lens, dk, [outs.ptrs[0], None, outs.ptrs[2]]) == bad
    assert M.call_open(ctx, [cins.ptrs[0], None, cins.ptrs[2]], b.lens, dk, plains.ptrs, status.ptrs[0]) == bad
    assert M.call_open(ctx, cins.ptrs, b.lens, dk, [None, None, plains.ptrs[2]], status.ptrs[0]) == bad
    # a length above 1 << 24, after valid messages
    long = [b.lens[0], b.lens[1], (1 << 24) + 1]
    assert M.call_seal(ctx, ins.ptrs, long, dk, outs.ptrs) == unsup
    assert M.call_open(ctx, cins.ptrs, long, dk, plains.ptrs, status.ptrs[0]) == unsup
    # a capturing stream: refused before anything is staged
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side, capture_error_mode="relaxed"):
        torch.zeros(1, device="cuda")  # (something for the graph to hold)
        rc_s = M.call_seal(ctx, ins.ptrs, b.lens, dk, outs.ptrs, stream=side)
        rc_o = M.call_open(ctx, cins.ptrs, b.lens, dk, plains.ptrs, status.ptrs[0], stream=side)
    assert (rc_s, rc_o) == (unsup, unsup)
    # no messages: fine, nothing queued
    assert ctx.L.ec_gcm_seal_messages(ctx.ctx, 0, None, None, None, None, None, None) == 0
    assert ctx.L.ec_gcm_open_messages(ctx.ctx, 0, None, None, None, None, None, None, None) == 0
    torch.cuda.synchronize()
    assert M.stats(ctx)[:3] == [0, 0, 0]
    for w in (outs, plains, status):
        w.check([None] * len(w.sizes))
    ins.check(b.plains)
    cins.check(b.sealed)
    # and the same lists are fine once nothing is wrong with the call
    assert M.call_seal(ctx, ins.ptrs, b.lens, dk, outs.ptrs) == 0
    torch.cuda.synchronize()
    outs.check(b.sealed)


def test_side_stream(ctx, boundary):
    b = boundary[0].pick(range(0, len(boundary[0]), 7))
    dk = M.DevKeys(b)
    ins = M.Ins(b.plains)
    outs = M.Outs([len(x) for x in b.sealed])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    assert M.call_seal(ctx, ins.ptrs, b.lens, dk, outs.ptrs, stream=side) == 0
    side.synchronize()
    outs.check(b.sealed)


def test_two_threads_on_their_own_streams(ctx, boundary):
    b = boundary[0]
    halves = [b.pick(range(0, len(b), 2)), b.pick(range(1, len(b), 2))]
    errors = []

    def work(part, which):
        try:
            torch.cuda.set_device(0)
            side = torch.cuda.Stream()
            with torch.cuda.stream(side):
                for _ in range(3):
                    if which:
                        M.run_seal(ctx, part, ("mix", 1, 0), ("mix", 2, 1))
                    else:
                        M.run_open(ctx, part, ("mix", 2, 1), ("mix", 1, 0))
        except BaseException as e:  # noqa: BLE001 - reported by the main thread
            errors.append(e)

    threads = [threading.Thread(target=work, args=(halves[i], i)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


def test_python_mirrors(ag):
    rng = np.random.default_rng(20261030)
    key = rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
    nonce24 = rng.integers(0, 256, 24, dtype=np.uint8).tobytes()
    for n in (1, 16, 100, 4096):
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        want = bytes(ag.seal(key, nonce24[:12], data))
        got = encryption.encrypt(data, key, nonce24)
        assert got == want
        assert encryption.decrypt(want, key, nonce24) == data
        bad = bytearray(want)
        bad[n // 2] ^= 1
        with pytest.raises(encryption.DecryptionFailed) as e:
            encryption.decrypt(bytes(bad), key, nonce24)
        assert e.value.block == 0
    # the empty-data rule and a short cipher text
    assert encryption.encrypt(b"", key, nonce24) == b"" and encryption.decrypt(b"", key, nonce24) == b""
    with pytest.raises(encryption.DecryptionFailed):
        encryption.decrypt(bytes(15), key, nonce24)
    # a bare tag is a message: the empty plaintext's
    assert encryption.decrypt(bytes(ag.seal(key, nonce24[:12], b"")), key, nonce24) == b""
    content = rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
    ek = encryption.encrypt_key(content, key, nonce24)
    assert ek == bytes(ag.seal(key, nonce24[:12], content)) and len(ek) == 48
    assert encryption.decrypt_key(ek, key, nonce24) == content
    with pytest.raises(encryption.DecryptionFailed):
        encryption.decrypt_key(ek[:-1] + bytes([ek[-1] ^ 1]), key, nonce24)


class _Scheme:
    def __init__(self, c):
        self.ctx = c.ctx


def _inline_batch(ag, sizes, seed):
    rng = np.random.default_rng(seed)
    r = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()  # noqa: E731
    plains = [r(n) for n in sizes]
    ck, dk = [r(32) for _ in sizes], [r(32) for _ in sizes]
    nn, kn = [r(24) for _ in sizes], [r(24) for _ in sizes]
    enc = [bytes(ag.seal(k, n[:12], p)) if p else b"" for k, n, p in zip(ck, nn, plains)]
    ekeys = [bytes(ag.seal(d, n[:12], k)) for d, n, k in zip(dk, kn, ck)]
    return plains, ck, nn, dk, kn, enc, ekeys


def _dev(b):
    return torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda()


def test_seal_inline_uploads(ctx, ag):
    plains, ck, nn, dk, kn, enc, ekeys = _inline_batch(ag, [1, 100, 4096, 0, 33], 20261031)
    s = _Scheme(ctx)
    before = M.stats(ctx)
    got, got_keys = uploads.seal_inline_uploads(s, [_dev(p) for p in plains], ck, nn, dk, kn)
    torch.cuda.synchronize()
    after = M.stats(ctx)
    assert after[0] - before[0] == 1 and after[2] - before[2] == 1  # one call over the 2N messages
    assert [bytes(g.cpu().numpy()) for g in got] == enc
    assert got_keys.shape == (5, 48) and [bytes(r) for r in got_keys.cpu().numpy()] == ekeys
    # device tensors for the keys and nonces, and a side stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    rows = lambda xs, w: torch.stack([_dev(x[:w]) for x in xs])  # noqa: E731
    with torch.cuda.stream(side):
        got, got_keys = uploads.seal_inline_uploads(s, [_dev(p) for p in plains[:3]], rows(ck[:3], 32), rows(nn[:3], 12),
                                                    rows(dk[:3], 32), rows(kn[:3], 12), stream=side)
    side.synchronize()
    assert [bytes(g.cpu().numpy()) for g in got] == enc[:3]
    assert [bytes(r) for r in got_keys.cpu().numpy()] == ekeys[:3]
    with pytest.raises(ValueError):
        uploads.seal_inline_uploads(s, [_dev(plains[0])], ck[:2], nn[:1], dk[:1], kn[:1])


def test_open_inline_downloads(ctx, ag):
    plains, ck, nn, dk, kn, enc, ekeys = _inline_batch(ag, [1, 100, 4096, 0, 33, 700, 64], 20261101)
    s = _Scheme(ctx)
    keys, status = downloads.open_content_keys(s, ekeys, dk, kn)
    assert [bytes(r) for r in keys.cpu().numpy()] == ck and status.cpu().tolist() == [0] * 7
    got = downloads.open_inline_downloads(s, [_dev(e) if e else torch.empty(0, dtype=torch.uint8, device="cuda")
                                              for e in enc], ekeys, dk, kn, nn)
    assert [bytes(g.cpu().numpy()) for g in got] == plains
    # a corrupted encrypted key is that download's key failure, corrupted data that download's data failure
    ekeys2, enc2 = list(ekeys), list(enc)
    ekeys2[1] = ekeys2[1][:40] + bytes([ekeys2[1][40] ^ 2]) + ekeys2[1][41:]
    enc2[4] = bytes([enc2[4][0] ^ 1]) + enc2[4][1:]
    enc2[6] = enc2[6][:5]  # shorter than a tag
    got = downloads.open_inline_downloads(s, [_dev(e) if e else torch.empty(0, dtype=torch.uint8, device="cuda")
                                              for e in enc2], ekeys2, dk, kn, nn)
    assert isinstance(got[1], encryption.KeyDecryptionFailed)
    assert type(got[4]) is encryption.DecryptionFailed and type(got[6]) is encryption.DecryptionFailed
    for g in (0, 2, 3, 5):
        assert bytes(got[g].cpu().numpy()) == plains[g]
    keys, status = downloads.open_content_keys(s, ekeys2, dk, kn)
    assert status.cpu().tolist() == [0, 1, 0, 0, 0, 0, 0] and bytes(keys[1].cpu().numpy()) == bytes(32)
