"""Harness of tests/test_gcm_sized.py, and -- run as a program -- the child
process of its test_checked_library: ec_gcm_seal_segments_sized and
ec_gcm_open_segments_sized against the bounds-checked build of the library
(every global load and store of gcm_blocks_sized and of the pad launch compared
with the segment's declared extent, every status store with the status words;
one outside is skipped and reported on stderr as "uplink_ec checked: ...").
Prints the library's build id first, then "ok".  `capped` as its argument: the
block-count batch with a 1100-block segment added, with blocks of 7408 and of 16
bytes, for a run with UPLINK_GCM_GRID_PER_CU=1 (a grid of 256 shared in
proportion, so the large segment's waves loop).  Expected bytes are oracle.aesgcm's over the test's own bytes."""
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
from sized_checked_child import Ctx, Outs  # noqa: E402,F401
from encode_sized_checked_child import Ins  # noqa: E402,F401

TAG = 16
IN_BLOCK = 7408  # 29*256 - 16 (project.go:84)
# a wave short of a workgroup, exactly one, one over, two and one over, a skipped segment,
# ragged 10.25 and 32.5 workgroups
EDGE_BLOCKS = [1, 3, 4, 5, 0, 8, 9, 41, 130]
# one segment far larger than the target grid's waves beside small ones: its waves loop
CAPPED_BLOCKS = [1, 40000, 5, 700]


class Batch:
    """Segments of nblocks[g] blocks of in_block bytes, each under a random key and nonce of its
    own: the padded plaintexts and the oracle's ciphertexts (encrypt_blocks); read-only"""

    def __init__(self, ag, nblocks, in_block, seed, nonces=None):
        rng = np.random.default_rng(seed)
        self.nblocks, self.in_block = list(nblocks), in_block
        self.keys = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in nblocks]
        self.nonces = list(nonces) if nonces else [rng.integers(0, 256, 12, dtype=np.uint8).tobytes() for _ in nblocks]
        self.plains = [rng.integers(0, 256, nb * in_block, dtype=np.uint8) for nb in nblocks]
        self.ciphers = [ag.encrypt_blocks(k, n, p, in_block, threads=8).reshape(-1) if nb else np.zeros(0, np.uint8)
                        for k, n, p, nb in zip(self.keys, self.nonces, self.plains, nblocks)]
        for a in self.plains + self.ciphers:
            a.setflags(write=False)

    def pick(self, order):
        """the batch with its segments in another order (or a subset)"""
        b = object.__new__(Batch)
        b.in_block = self.in_block
        for name in ("nblocks", "keys", "nonces", "plains", "ciphers"):
            setattr(b, name, [getattr(self, name)[g] for g in order])
        return b


class DevKeys:
    """the batch's prepared keys and nonces on the device"""

    def __init__(self, L, batch):
        kb = L.ec_gcm_key_bytes()
        self.keys = torch.empty(max(len(batch.keys), 1) * kb, dtype=torch.uint8, device="cuda")
        host = np.frombuffer(b"".join(batch.keys), dtype=np.uint8)
        rc = L.ec_gcm_prepare_keys(host.ctypes.data, len(batch.keys), self.keys.data_ptr(),
                                   torch.cuda.current_stream().cuda_stream)
        assert rc == 0, _native.strerror(rc)
        self.nonces = torch.from_numpy(np.frombuffer(b"".join(batch.nonces), dtype=np.uint8).copy()).cuda()


def stats(c):
    v = [ctypes.c_ulonglong() for _ in range(3)]
    assert c.L.ec_gcm_sized_stats(c.ctx, *[ctypes.byref(x) for x in v]) == 0
    return [x.value for x in v]  # seal launches, open launches, passes


def call_seal(c, in_ptrs, nblocks, in_block, dk, out_ptrs, data_len=None, stream=None, null=()):
    """-> rc.  null: names of arguments passed as NULL"""
    nseg = len(nblocks)
    a = lambda t, v: (t * max(nseg, 1))(*v)  # noqa: E731
    st = (stream or torch.cuda.current_stream()).cuda_stream
    return c.L.ec_gcm_seal_segments_sized(
        c.ctx, nseg, None if "plain" in null else a(ctypes.c_void_p, in_ptrs),
        None if "nblocks" in null else a(ctypes.c_size_t, nblocks),
        None if data_len is None else a(ctypes.c_size_t, data_len), in_block,
        None if "keys" in null else dk.keys.data_ptr(), None if "nonces" in null else dk.nonces.data_ptr(),
        None if "out" in null else a(ctypes.c_void_p, out_ptrs), st)


def call_open(c, in_ptrs, nblocks, in_block, dk, out_ptrs, status_ptr, stream=None, null=()):
    nseg = len(nblocks)
    a = lambda t, v: (t * max(nseg, 1))(*v)  # noqa: E731
    st = (stream or torch.cuda.current_stream()).cuda_stream
    return c.L.ec_gcm_open_segments_sized(
        c.ctx, nseg, None if "cipher" in null else a(ctypes.c_void_p, in_ptrs),
        None if "nblocks" in null else a(ctypes.c_size_t, nblocks), in_block,
        None if "keys" in null else dk.keys.data_ptr(), None if "nonces" in null else dk.nonces.data_ptr(),
        None if "out" in null else a(ctypes.c_void_p, out_ptrs), None if "status" in null else status_ptr, st)


def run_seal(c, b, dk=None):
    """one seal call over the batch, plaintexts and ciphertexts in windows of 0xCD-filled buffers
    with 64-byte guards: every output, every input and all guards compared whole"""
    dk = dk or DevKeys(c.L, b)
    ins = Ins(b.plains)
    outs = Outs([len(x) for x in b.ciphers])
    rc = call_seal(c, ins.ptrs, b.nblocks, b.in_block, dk, outs.ptrs)
    assert rc == 0, _native.strerror(rc)
    torch.cuda.synchronize()
    outs.check(b.ciphers)
    ins.check(b.plains)
    return ins, outs


def run_open(c, b, ciphers=None, want_status=None, dk=None):
    """one open call over the batch's ciphertexts (or `ciphers`): the status words (guarded, all
    defined), the plaintext of every segment that verified, the inputs and all guards"""
    dk = dk or DevKeys(c.L, b)
    nseg = len(b.nblocks)
    ciphers = ciphers or b.ciphers
    want_status = [-1] * nseg if want_status is None else want_status
    ins = Ins(ciphers)
    outs = Outs([len(x) for x in b.plains])
    status = Outs([4 * nseg])
    rc = call_open(c, ins.ptrs, b.nblocks, b.in_block, dk, outs.ptrs, status.ptrs[0])
    assert rc == 0, _native.strerror(rc)
    torch.cuda.synchronize()
    status.check([np.array(want_status, dtype=np.int32).view(np.uint8)])
    outs.check(b.plains, skip=[g for g, s in enumerate(want_status) if s >= 0])
    ins.check(ciphers)
    return outs, status


def corrupted(b):
    """the block-count batch (EDGE_BLOCKS order) with a tag bit flipped in blocks 7 and 2 of the
    9-block segment, a ciphertext bit in block 0 of the 1-block segment and a tag bit in block 129
    of the 130-block segment: (ciphertexts, the status words they must give)"""
    ob = b.in_block + TAG
    cs = [x.copy() for x in b.ciphers]
    want = [-1] * len(cs)
    g9, g1, g130 = b.nblocks.index(9), b.nblocks.index(1), b.nblocks.index(130)
    cs[g9][7 * ob + b.in_block + 3] ^= 0x10
    cs[g9][2 * ob + b.in_block + 15] ^= 0x01
    want[g9] = 2
    cs[g1][100] ^= 0x80
    want[g1] = 0
    cs[g130][129 * ob + b.in_block] ^= 0x02
    want[g130] = 129
    return cs, want


def main():
    L = _native.load(os.path.join(ROOT, "uplink_amd", "lib", "checked", "libuplink_ec_checked.so"))
    print("build", L.ec_build_id().decode(), flush=True)
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "--build-id":
        return 0
    from oracle import aesgcm as ag
    c = Ctx(29, 80, 256, L)
    edge = Batch(ag, EDGE_BLOCKS, IN_BLOCK, 20261021)
    order = list(range(len(EDGE_BLOCKS)))
    if mode == "capped":  # (UPLINK_GCM_GRID_PER_CU=1 in the environment)
        run_seal(c, Batch(ag, EDGE_BLOCKS + [1100], IN_BLOCK, 20261021))
        run_seal(c, Batch(ag, EDGE_BLOCKS + [1100], 16, 31))
    else:
        for o in (order, order[::-1]):
            run_seal(c, edge.pick(o))
        run_seal(c, Batch(ag, CAPPED_BLOCKS, 16, 32))
        run_open(c, edge)
        cs, want = corrupted(edge)
        run_open(c, edge, cs, want)
    c.close()
    print("ok", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
