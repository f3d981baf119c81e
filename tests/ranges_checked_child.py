"""Harness of tests/test_ranges.py, and -- run as a program -- the child process
of its test_checked_library: ec_gcm_open_ranges_sized against the bounds-checked
build of the library (every load of gcm_open_ranged compared with the nb*B bytes
of the segment's covered blocks, every store with the `length` bytes of its
output, every status store with the status words; one outside is skipped and
reported on stderr as "uplink_ec checked: ...").  Prints the library's build id
first, then "ok".  Sources and outputs sit in windows of 0xCD-filled buffers with
64-byte guards, at byte offsets 0, 1, 8 and 15 from a 16-byte boundary, and every
output, input and guard is compared whole.  Expected bytes are oracle.aesgcm's
over the test's own bytes:
decrypt_blocks(key, increment(nonce, fb), covered blocks, ib)[head : head+len]."""
import ctypes
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
from uplink_amd.streams import calc_encompassing_blocks  # noqa: E402
from gcm_sized_checked_child import IN_BLOCK, TAG, Ctx, DevKeys, Ins, Outs  # noqa: E402,F401

IB = IN_BLOCK
SHIFTS = [0, 1, 8, 15]


def cut_edge_specs(ib=IB):
    """(first block, head, length) of the cut-edge batch: heads 0, 1, 15, 16, 17 and ib-1 crossed
    with ends on a block boundary, 1 byte past one and 1 byte short of one; lengths 0, 1 and 2
    inside one 16-byte slot, across a slot boundary and across a block boundary; ranges inside one
    block, across two, across all six, and a whole 6-block segment.  First blocks cycle 0, 1, 3."""
    cuts = []
    for head in (0, 1, 15, 16, 17, ib - 1):
        for end in (2 * ib, 2 * ib + 1, 2 * ib - 1):
            cuts.append((head, end - head))
    cuts += [(5, 0), (5, 1), (5, 2), (15, 1), (15, 2), (ib - 1, 2), (32, 0)]
    cuts += [(100, 1000), (7000, 1000), (1, 5 * ib + 10), (0, 6 * ib)]
    return [((0, 1, 3)[g % 3], h, n) for g, (h, n) in enumerate(cuts)]


class Ranges:
    """Ranges (first block, head, length) at in_block, each under a random key and nonce of its
    own: the covered blocks' random plaintext, the oracle's ciphertext of them under
    nonce + first block, and the expected output -- the oracle's own decryption of that ciphertext,
    cut; read-only"""

    def __init__(self, ag, specs, in_block, seed, nonces=None):
        rng = np.random.default_rng(seed)
        self.in_block = in_block
        self.fb = [s[0] for s in specs]
        self.head = [s[1] for s in specs]
        self.length = [s[2] for s in specs]
        self.nblocks = [calc_encompassing_blocks(h, n, in_block)[1] for _, h, n in specs]
        self.keys = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in specs]
        self.nonces = list(nonces) if nonces else [rng.integers(0, 256, 12, dtype=np.uint8).tobytes() for _ in specs]
        self.ciphers, self.want = [], []
        for g, nb in enumerate(self.nblocks):
            if nb == 0:
                self.ciphers.append(np.zeros(0, np.uint8))
                self.want.append(np.zeros(0, np.uint8))
                continue
            start = ag.increment(self.nonces[g], self.fb[g])
            plain = rng.integers(0, 256, nb * in_block, dtype=np.uint8)
            threads = 8 if nb > 8 else 1
            cipher = ag.encrypt_blocks(self.keys[g], start, plain, in_block, threads=threads).reshape(-1)
            back, bad = ag.decrypt_blocks(self.keys[g], start, cipher, in_block, threads=threads)
            assert bad == -1
            self.ciphers.append(cipher)
            self.want.append(np.array(back[self.head[g]:self.head[g] + self.length[g]]))
            assert len(self.want[-1]) == self.length[g]
        for a in self.ciphers + self.want:
            a.setflags(write=False)

    def __len__(self):
        return len(self.fb)

    def pick(self, order):
        b = object.__new__(Ranges)
        b.in_block = self.in_block
        for name in ("fb", "head", "length", "nblocks", "keys", "nonces", "ciphers", "want"):
            setattr(b, name, [getattr(self, name)[g] for g in order])
        return b


def stats(c):
    v = [ctypes.c_ulonglong() for _ in range(2)]
    assert c.L.ec_gcm_ranged_stats(c.ctx, *[ctypes.byref(x) for x in v]) == 0
    return [x.value for x in v]  # open launches, passes


def call_ranges(c, in_ptrs, fb, nblocks, head, length, in_block, dk, out_ptrs, status_ptr, stream=None, null=()):
    """-> rc.  null: names of arguments passed as NULL"""
    nseg = len(nblocks)
    a = lambda t, v: (t * max(nseg, 1))(*v)  # noqa: E731
    sz = lambda name, v: None if name in null else a(ctypes.c_size_t, v)  # noqa: E731
    st = (stream or torch.cuda.current_stream()).cuda_stream
    return c.L.ec_gcm_open_ranges_sized(
        c.ctx, nseg, None if "cipher" in null else a(ctypes.c_void_p, in_ptrs), sz("first_block", fb),
        sz("nblocks", nblocks), sz("head", head), sz("length", length), in_block,
        None if "keys" in null else dk.keys.data_ptr(), None if "nonces" in null else dk.nonces.data_ptr(),
        None if "out" in null else a(ctypes.c_void_p, out_ptrs), None if "status" in null else status_ptr, st)


def shifts(n, which):
    """n window offsets from a 16-byte boundary: one value for all, or "mix": 0, 1, 8, 15 in turn
    (rot: where the turn starts)"""
    if isinstance(which, tuple):
        return [SHIFTS[(g // which[1] + which[2]) % 4] for g in range(n)]
    return [which] * n


def run_ranges(c, b, in_shift=0, out_shift=0, ciphers=None, want_status=None, dk=None):
    """one call over the ranges: the status words (guarded, all defined), every output that
    verified, the inputs and all guards compared whole.  -> (outs, status)"""
    dk = dk or DevKeys(c.L, b)
    nseg = len(b)
    ciphers = ciphers or b.ciphers
    want_status = [-1] * nseg if want_status is None else want_status
    ins = Ins(ciphers, shifts(nseg, in_shift))
    outs = Outs(b.length, shifts(nseg, out_shift))
    status = Outs([4 * nseg])
    rc = call_ranges(c, ins.ptrs, b.fb, b.nblocks, b.head, b.length, b.in_block, dk, outs.ptrs, status.ptrs[0])
    assert rc == 0, _native.strerror(rc)
    torch.cuda.synchronize()
    status.check([np.array(want_status, dtype=np.int32).view(np.uint8)])
    outs.check(b.want, skip=[g for g, s in enumerate(want_status) if s >= 0])
    ins.check(ciphers)
    return outs, status


def corrupted(b):
    """the cut-edge batch with: a tag bit in covered block 1 of range 0, inside the wanted bytes;
    a ciphertext bit in the head of block 0 of the head-17 range and one in the last block of a
    range that ends 1 byte past a block boundary, both OUTSIDE the wanted bytes; tag bits in
    blocks 4 and 2 of the range across all six.  -> (ciphertexts, the status words they must give:
    the smallest absolute number of a failing covered block)"""
    ob = b.in_block + TAG
    cs = [x.copy() for x in b.ciphers]
    want = [-1] * len(cs)
    g = 0  # head 0, two whole blocks
    assert b.nblocks[g] == 2 and b.length[g] == 2 * b.in_block
    cs[g][1 * ob + b.in_block + 7] ^= 0x04
    want[g] = b.fb[g] + 1
    g = next(i for i in range(len(cs)) if b.head[i] == 17 and b.nblocks[i] == 3)
    cs[g][3] ^= 0x80  # byte 3 of block 0: before the head
    want[g] = b.fb[g]
    g = next(i for i in range(len(cs)) if b.head[i] == 1 and b.head[i] + b.length[i] == 2 * b.in_block + 1)
    assert b.nblocks[g] == 3
    cs[g][2 * ob + 100] ^= 0x01  # byte 100 of block 2, of which only byte 0 is wanted
    want[g] = b.fb[g] + 2
    g = next(i for i in range(len(cs)) if b.nblocks[i] == 6 and b.head[i] == 1)
    cs[g][4 * ob + b.in_block] ^= 0x10
    cs[g][2 * ob + b.in_block + 15] ^= 0x01
    want[g] = b.fb[g] + 2
    return cs, want


def main():
    L = _native.load(os.path.join(ROOT, "uplink_amd", "lib", "checked", "libuplink_ec_checked.so"))
    print("build", L.ec_build_id().decode(), flush=True)
    if len(sys.argv) > 1 and sys.argv[1] == "--build-id":
        return 0
    from oracle import aesgcm as ag
    c = Ctx(29, 80, 256, L)
    cut = Ranges(ag, cut_edge_specs(), IB, 20261022)
    dk = DevKeys(c.L, cut)
    run_ranges(c, cut, dk=dk)
    run_ranges(c, cut, ("mix", 1, 0), ("mix", 4, 1), dk=dk)
    for s in (1, 8, 15):
        run_ranges(c, cut, s, 16 - s, dk=dk)
    cs, want = corrupted(cut)
    run_ranges(c, cut, ciphers=cs, want_status=want, dk=dk)
    run_ranges(c, cut, ("mix", 1, 1), ("mix", 4, 0), ciphers=cs, want_status=want, dk=dk)
    c.close()
    print("ok", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
