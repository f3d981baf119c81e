"""Harness of tests/test_sha256.py, and -- run as a program -- the child process
of its test_checked_library: ec_sha256_pieces_list and ec_sha256_segments_sized
against the bounds-checked build of the library (every load of the lanes kernel
compared with its own piece's extent, every digest store with the declared
output range and every state load and store with the staging block; one outside
is skipped and reported on stderr as "uplink_ec checked: ...").  Prints the
library's build id first, then "ok".  Expected digests are hashlib.sha256's over
the test's own bytes."""
import ctypes
import hashlib
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
from sized_checked_child import Ctx, Outs, encode_segments  # noqa: E402,F401
from encode_sized_checked_child import Ins, call_encode, expected, piece_sizes  # noqa: E402,F401

# every padding edge: the 0x80 and the length in one block (<= 55 bytes over a block), the length
# in a block of its own (56 .. 63 over), whole blocks, and two longer pieces (262,400 = 1025 * 256)
EDGE_LENS = [0, 1, 55, 56, 57, 63, 64, 65, 119, 120, 121, 127, 128, 129, 4096, 262400]
# RS(29,80) ess 256, pieces of 256 .. 262,400 bytes; 0: a skipped segment
UPLOAD_STRIPES = [1, 3, 41, 1025, 0]
LAUNCH_BLOCKS = 16384  # sha_list_geom.hpp kLaunchBlocks


def sha(data) -> np.ndarray:
    return np.frombuffer(hashlib.sha256(bytes(data)).digest(), dtype=np.uint8)


def blocks_of(ln: int) -> int:
    """FIPS 180-4 §5.1.1: the message, 0x80, zeros and the 64-bit length, in 64-byte blocks"""
    return (ln + 8) // 64 + 1


def launches_of(lens, launch_blocks=LAUNCH_BLOCKS) -> int:
    """launches one pass over pieces of these lengths takes: the longest piece's blocks, launch_blocks at a time"""
    return -(-max(blocks_of(x) for x in lens) // launch_blocks)


def edge_pieces(lens=EDGE_LENS, seed=20261021):
    """(pieces, their digests by hashlib): read-only arrays"""
    rng = np.random.default_rng(seed)
    pieces = [rng.integers(0, 256, ln, dtype=np.uint8) for ln in lens]
    hashes = [sha(p) for p in pieces]
    for a in pieces + hashes:
        a.setflags(write=False)
    return pieces, hashes


def stats(c):
    v = [ctypes.c_ulonglong() for _ in range(3)]
    assert c.L.ec_sha256_list_stats(c.ctx, *[ctypes.byref(x) for x in v]) == 0
    return [x.value for x in v]  # fast pieces, bytewise pieces, launches


def call_list(c, ptrs, lens, hash_ptr, stream=None):
    npieces = len(lens)
    st = (stream or torch.cuda.current_stream()).cuda_stream
    return c.L.ec_sha256_pieces_list(c.ctx, npieces, (ctypes.c_void_p * max(npieces, 1))(*ptrs),
                                     (ctypes.c_size_t * max(npieces, 1))(*lens), hash_ptr, st)


def run_list(c, pieces, hashes, shift=None):
    """one ec_sha256_pieces_list call over the pieces in windows of one 0xCD-filled buffer with
    64-byte guards, into a guarded hash buffer; hashes, inputs and guards compared whole"""
    ins = Ins(pieces, shift)
    out = Outs([32 * len(pieces)])
    rc = call_list(c, ins.ptrs, [len(p) for p in pieces], out.ptrs[0])
    assert rc == 0, _native.strerror(rc)
    torch.cuda.synchronize()
    out.check([np.concatenate(hashes)])
    ins.check(pieces)
    return ins, out


def upload_batch(O, k, n, ess, stripes, seed):
    """per stripe count: (the padded segment, its n pieces by the oracle's encode_segment, their
    [n, 32] digests by hashlib)"""
    segs, refs = encode_segments(O, k, n, ess, stripes, seed)
    hashes = []
    for r in refs:
        h = np.stack([sha(row) for row in r]) if r.shape[1] else np.zeros((n, 32), np.uint8)
        h.setflags(write=False)
        hashes.append(h)
    return segs, refs, hashes


def call_sha_sized(c, seg_ptrs, stripes, piece_ptrs, hash_ptr, parity_only=False, stream=None):
    nseg = len(stripes)
    a = lambda t, v: (t * max(nseg, 1))(*v)  # noqa: E731
    st = (stream or torch.cuda.current_stream()).cuda_stream
    return c.L.ec_sha256_segments_sized(c.ctx, nseg, None if seg_ptrs is None else a(ctypes.c_void_p, seg_ptrs),
                                        a(ctypes.c_size_t, stripes), a(ctypes.c_void_p, piece_ptrs),
                                        _native.EC_FLAG_PARITY_ONLY if parity_only else 0, hash_ptr, st)


def run_upload_batch(c, segs, refs, hashes, stripes, parity_only=False):
    """one ec_encode_segments_sized and one ec_sha256_segments_sized over the batch: pieces, the
    [nseg][n][32] digests (a skipped segment's rows stay 0xCD), inputs and all guards compared whole"""
    ins = Ins(segs)
    outs = Outs(piece_sizes(c, stripes, parity_only))
    rc = call_encode(c, ins.ptrs, stripes, outs.ptrs, parity_only=parity_only)
    assert rc == 0, _native.strerror(rc)
    flat = Outs([32 * c.n * len(stripes)])  # [nseg][n][32], guarded
    rc = call_sha_sized(c, ins.ptrs, stripes, outs.ptrs, flat.ptrs[0], parity_only=parity_only)
    assert rc == 0, _native.strerror(rc)
    torch.cuda.synchronize()
    outs.check(expected(c, refs, parity_only))
    ins.check(segs)
    want = np.concatenate([np.full(32 * c.n, 0xCD, np.uint8) if s == 0 else h.reshape(-1)
                           for s, h in zip(stripes, hashes)])
    flat.check([want])
    return flat


def main():
    L = _native.load(os.path.join(ROOT, "uplink_amd", "lib", "checked", "libuplink_ec_checked.so"))
    print("build", L.ec_build_id().decode(), flush=True)
    if len(sys.argv) > 1 and sys.argv[1] == "--build-id":
        return 0
    from oracle import oracle as O
    O.build()
    k, n, ess = 29, 80, 256
    c = Ctx(k, n, ess, L)
    pieces, hashes = edge_pieces()
    run_list(c, pieces, hashes)
    segs, refs, hs = upload_batch(O, k, n, ess, UPLOAD_STRIPES, 2983)
    run_upload_batch(c, segs, refs, hs, UPLOAD_STRIPES, parity_only=True)
    # the carried state's loads and stores: short pieces at two blocks per launch
    assert L.ec_sha256_set_launch_blocks(c.ctx, 2) == 0
    pieces, hashes = edge_pieces(list(range(0, 331, 11)), 5)
    run_list(c, pieces, hashes)
    assert L.ec_sha256_set_launch_blocks(c.ctx, 0) == 0
    c.close()
    print("ok", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
