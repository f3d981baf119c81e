"""Harness of tests/test_messages.py, and -- run as a program -- the child process
of its test_checked_library: ec_gcm_seal_messages and ec_gcm_open_messages against
the bounds-checked build of the library (every load of gcm_messages compared with
the message's len (+16 to open) input bytes, every store with its len (+16 sealed)
output bytes, every status store with the status words; one outside is skipped and
reported on stderr as "uplink_ec checked: ...").  Prints the library's build id
first, then "ok".  Sources and outputs sit in windows of 0xCD-filled buffers with
64-byte guards, at byte offsets 0, 1, 8 and 15 from a 16-byte boundary, and every
output, input and guard is compared whole.  Expected bytes are oracle.aesgcm's
seal over the test's own plaintexts, keys and nonces."""
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from uplink_amd import _native  # noqa: E402
from sized_checked_child import Ctx, Outs  # noqa: E402,F401
from encode_sized_checked_child import Ins  # noqa: E402,F401

TAG = 16
SHIFTS = [0, 1, 8, 15]
# The issue's list -- across a 16-byte slot (15, 16, 17; 31, 32, 33; 47, 48), across one slot per
# lane, i.e. 63, 64 and 65 GHASH inputs (1007, 1008, 1009: from one round per lane to two), and
# longer ones -- and the boundaries of this lane layout (gcm_msg_geom.hpp): 2032 / 2033, two rounds
# per lane to three; and where a further step of the pairwise combination starts, 3, 5, 9, 17 and 33
# live lanes at one round (lengths 17 and 33 above; 49, 113 with 112, 241 with 240, 497 with 496)
# and 33 live lanes at two rounds (1009 above).
BOUNDARY_LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 1007, 1008, 1009, 1023, 1024, 1025, 2048 + 5, 4095, 4096,
                    4097, 8191, 49, 112, 113, 240, 241, 496, 497, 2032, 2033]


def spec_cases():
    """the no-AAD AES-256 cases of tests/golden/aesgcm_vectors.json: (key, nonce, plaintext, ct || tag)"""
    with open(os.path.join(HERE, "golden", "aesgcm_vectors.json")) as fh:
        cases = json.load(fh)["cases"]
    out = [(bytes.fromhex(c["key"]), bytes.fromhex(c["iv"]), bytes.fromhex(c["pt"]),
            bytes.fromhex(c["ct"]) + bytes.fromhex(c["tag"])) for c in cases if not c["aad"] and len(c["key"]) == 64]
    assert sorted(len(c[2]) for c in out) == [0, 16, 64]
    return out


class Messages:
    """Messages of lens[i] bytes, each under a seeded random key and nonce of its own: the
    plaintexts and the oracle's sealed bytes; read-only"""

    def __init__(self, ag, lens, seed):
        rng = np.random.default_rng(seed)
        self.lens = [int(x) for x in lens]
        self.keys = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in self.lens]
        self.nonces = [rng.integers(0, 256, 12, dtype=np.uint8).tobytes() for _ in self.lens]
        self.plains = [rng.integers(0, 256, n, dtype=np.uint8) for n in self.lens]
        self.sealed = [np.frombuffer(bytes(ag.seal(k, n, p.tobytes())), dtype=np.uint8).copy() for k, n, p in
                       zip(self.keys, self.nonces, self.plains)]
        self.freeze()

    @classmethod
    def of(cls, cases):
        """from (key, nonce, plaintext, sealed) tuples"""
        b = object.__new__(cls)
        b.keys, b.nonces = [c[0] for c in cases], [c[1] for c in cases]
        b.plains = [np.frombuffer(c[2], dtype=np.uint8).copy() for c in cases]
        b.sealed = [np.frombuffer(c[3], dtype=np.uint8).copy() for c in cases]
        b.lens = [len(p) for p in b.plains]
        b.freeze()
        return b

    def freeze(self):
        assert all(len(s) == n + TAG for s, n in zip(self.sealed, self.lens))
        for a in self.plains + self.sealed:
            a.setflags(write=False)

    def __len__(self):
        return len(self.lens)

    def pick(self, order):
        b = object.__new__(Messages)
        for name in ("lens", "keys", "nonces", "plains", "sealed"):
            setattr(b, name, [getattr(self, name)[g] for g in order])
        return b


class DevKeys:
    """the messages' raw keys and nonces on the device, 32 and 12 bytes each, the arrays `shift`
    bytes past a 16-byte boundary (neither needs alignment)"""

    def __init__(self, b, shift=0, keys=None, nonces=None):
        kb = np.frombuffer(b"".join(keys or b.keys), dtype=np.uint8)
        nb = np.frombuffer(b"".join(nonces or b.nonces), dtype=np.uint8)
        self.kbuf = torch.zeros(len(kb) + 32, dtype=torch.uint8, device="cuda")
        self.nbuf = torch.zeros(len(nb) + 32, dtype=torch.uint8, device="cuda")
        self.keys = self.kbuf[shift:shift + len(kb)]
        self.nonces = self.nbuf[shift:shift + len(nb)]
        self.keys.copy_(torch.from_numpy(kb.copy()))
        self.nonces.copy_(torch.from_numpy(nb.copy()))


def stats(c):
    v = [ctypes.c_ulonglong() for _ in range(4)]
    assert c.L.ec_gcm_messages_stats(c.ctx, *[ctypes.byref(x) for x in v]) == 0
    return [x.value for x in v]  # seal launches, open launches, passes, messages per pass


def _call(fn, c, in_ptrs, lens, dk, out_ptrs, extra, stream, null):
    n = len(lens)
    a = lambda t, v: (t * max(n, 1))(*v)  # noqa: E731
    st = (stream or torch.cuda.current_stream()).cuda_stream
    return fn(c.ctx, n, None if "in" in null else a(ctypes.c_void_p, in_ptrs),
              None if "len" in null else a(ctypes.c_size_t, lens),
              None if "keys" in null else dk.keys.data_ptr(), None if "nonces" in null else dk.nonces.data_ptr(),
              None if "out" in null else a(ctypes.c_void_p, out_ptrs), *extra, st)


def call_seal(c, in_ptrs, lens, dk, out_ptrs, stream=None, null=()):
    """-> rc.  null: names of arguments passed as NULL"""
    return _call(c.L.ec_gcm_seal_messages, c, in_ptrs, lens, dk, out_ptrs, (), stream, null)


def call_open(c, in_ptrs, lens, dk, out_ptrs, status_ptr, stream=None, null=()):
    return _call(c.L.ec_gcm_open_messages, c, in_ptrs, lens, dk, out_ptrs,
                 (None if "status" in null else status_ptr,), stream, null)


def shifts(n, which):
    """n window offsets from a 16-byte boundary: one value for all, or ("mix", every, rot):
    0, 1, 8, 15 in turn, moving on every `every` messages, starting at turn `rot`"""
    if isinstance(which, tuple):
        return [SHIFTS[(g // which[1] + which[2]) % 4] for g in range(n)]
    return [which] * n


def run_seal(c, b, in_shift=0, out_shift=0, dk=None):
    """one seal call over the messages: every output, every input and all guards compared whole"""
    dk = dk or DevKeys(b)
    ins = Ins(b.plains, shifts(len(b), in_shift))
    outs = Outs([len(x) for x in b.sealed], shifts(len(b), out_shift))
    rc = call_seal(c, ins.ptrs, b.lens, dk, outs.ptrs)
    assert rc == 0, _native.strerror(rc)
    torch.cuda.synchronize()
    outs.check(b.sealed)
    ins.check(b.plains)
    return ins, outs


def run_open(c, b, in_shift=0, out_shift=0, sealed=None, want_status=None, dk=None):
    """one open call over the sealed messages (or `sealed`): the status words (guarded, all
    defined), every output -- the plaintext, or len zero bytes where the wanted status is 1 --,
    the inputs and all guards compared whole.  -> (outs, status)"""
    dk = dk or DevKeys(b)
    n = len(b)
    sealed = sealed or b.sealed
    want_status = [0] * n if want_status is None else want_status
    ins = Ins(sealed, shifts(n, in_shift))
    outs = Outs(b.lens, shifts(n, out_shift))
    status = Outs([4 * n])
    rc = call_open(c, ins.ptrs, b.lens, dk, outs.ptrs, status.ptrs[0])
    assert rc == 0, _native.strerror(rc)
    torch.cuda.synchronize()
    status.check([np.array(want_status, dtype=np.int32).view(np.uint8)])
    outs.check([np.zeros(len(p), np.uint8) if s else p for p, s in zip(b.plains, want_status)])
    ins.check(sealed)
    return outs, status


def boundary_batch(ag):
    """every boundary length at every (source shift, output shift) pair of 0, 1, 8, 15: the messages
    and the two shift lists.  480 messages: 60 workgroups, one pass."""
    lens, s_in, s_out = [], [], []
    for n in BOUNDARY_LENGTHS:
        for a in SHIFTS:
            for b in SHIFTS:
                lens.append(n)
                s_in.append(a)
                s_out.append(b)
    return Messages(ag, lens, 20261025), s_in, s_out


def run_boundary(c, batch):
    b, s_in, s_out = batch
    dk = DevKeys(b, shift=5)
    ins = Ins(b.plains, s_in)
    outs = Outs([len(x) for x in b.sealed], s_out)
    assert call_seal(c, ins.ptrs, b.lens, dk, outs.ptrs) == 0
    torch.cuda.synchronize()
    outs.check(b.sealed)
    ins.check(b.plains)
    cins = Ins(b.sealed, s_in)
    plains = Outs(b.lens, s_out)
    status = Outs([4 * len(b)])
    assert call_open(c, cins.ptrs, b.lens, dk, plains.ptrs, status.ptrs[0]) == 0
    torch.cuda.synchronize()
    status.check([np.zeros(4 * len(b), np.uint8)])
    plains.check(b.plains)
    cins.check(b.sealed)


def tampered(ag, seed=20261026):
    """Six tampers, each between two good messages of the same call: a flipped first ciphertext
    bit, a flipped last ciphertext bit, a flipped tag bit, a wrong key, a wrong nonce, and an empty
    message with a wrong tag.  -> (messages, sealed inputs, keys, nonces, wanted status)"""
    lens = [40, 100, 33, 16, 7, 1500, 64, 32, 48, 5, 20, 0, 9]
    b = Messages(ag, lens, seed)
    sealed = [x.copy() for x in b.sealed]
    keys, nonces = list(b.keys), list(b.nonces)
    sealed[1][0] ^= 0x80                      # first ciphertext bit
    sealed[3][15] ^= 0x01                     # last ciphertext bit
    sealed[5][1500 + 9] ^= 0x10               # a tag bit
    keys[7] = bytes([keys[7][0] ^ 1]) + keys[7][1:]
    nonces[9] = nonces[9][:11] + bytes([nonces[9][11] ^ 0x80])
    sealed[11][3] ^= 0x04                     # the tag of an empty message
    want = [g % 2 for g in range(len(lens))]  # 1, 3, .. 11 tampered, their neighbours good
    assert lens[11] == 0 and lens[3] == 16
    return b, sealed, keys, nonces, want


def main():
    L = _native.load(os.path.join(ROOT, "uplink_amd", "lib", "checked", "libuplink_ec_checked.so"))
    print("build", L.ec_build_id().decode(), flush=True)
    if len(sys.argv) > 1 and sys.argv[1] == "--build-id":
        return 0
    from oracle import aesgcm as ag
    c = Ctx(29, 80, 256, L)
    run_boundary(c, boundary_batch(ag))
    b, sealed, keys, nonces, want = tampered(ag)
    run_open(c, b, ("mix", 1, 0), ("mix", 1, 2), sealed=sealed, want_status=want, dk=DevKeys(b, 3, keys, nonces))
    c.close()
    print("ok", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
