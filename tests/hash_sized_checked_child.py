"""Harness of tests/test_hash_sized.py, and -- run as a program -- the child
process of its test_checked_library: ec_blake3_pieces_list and
ec_hash_segments_sized against the bounds-checked build of the library (every
load of the list kernels compared with its own piece's extent, every hash and
node store with the declared output range; one outside is skipped and reported
on stderr as "uplink_ec checked: ...").  Prints the library's build id first,
then "ok".  Expected hashes are oracle.blake3's over the test's own bytes."""
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
from sized_checked_child import Ctx, Outs, encode_segments  # noqa: E402,F401
from encode_sized_checked_child import Ins, call_encode, expected, piece_sizes  # noqa: E402,F401

# block, chunk and group edges; two-, three- and nine-group parents folds (the last is the
# production piece: 9060 stripes of 256 bytes)
EDGE_LENS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2048, 2049, 255 * 1024, 256 * 1024 - 1, 256 * 1024, 256 * 1024 + 1,
             257 * 1024, 512 * 1024 + 1024, 2319360]
# RS(29,80) ess 256: 4 stripes are one chunk, 1024 stripes one 256-chunk group; 0: a skipped segment
UPLOAD_STRIPES = [1, 3, 4, 5, 0, 41, 130, 1023, 1024, 1025]


def edge_pieces(ob, lens=EDGE_LENS, seed=20261020):
    """(pieces, their hashes by the oracle): read-only arrays"""
    rng = np.random.default_rng(seed)
    pieces = [rng.integers(0, 256, ln, dtype=np.uint8) for ln in lens]
    hashes = [np.frombuffer(ob.blake3(p), dtype=np.uint8) for p in pieces]
    for a in pieces + hashes:
        a.setflags(write=False)
    return pieces, hashes


def stats(c):
    v = [ctypes.c_ulonglong() for _ in range(4)]
    assert c.L.ec_hash_list_stats(c.ctx, *[ctypes.byref(x) for x in v]) == 0
    return [x.value for x in v]  # fast, byte, parents, oversize


def call_list(c, ptrs, lens, hash_ptr, stream=None):
    npieces = len(lens)
    st = (stream or torch.cuda.current_stream()).cuda_stream
    return c.L.ec_blake3_pieces_list(c.ctx, npieces, (ctypes.c_void_p * max(npieces, 1))(*ptrs),
                                     (ctypes.c_size_t * max(npieces, 1))(*lens), hash_ptr, st)


def run_list(c, pieces, hashes, shift=None):
    """one ec_blake3_pieces_list call over the pieces in windows of one 0xCD-filled buffer with
    64-byte guards, into a guarded hash buffer; hashes, inputs and guards compared whole"""
    ins = Ins(pieces, shift)
    out = Outs([32 * len(pieces)])
    rc = call_list(c, ins.ptrs, [len(p) for p in pieces], out.ptrs[0])
    assert rc == 0, _native.strerror(rc)
    torch.cuda.synchronize()
    out.check([np.concatenate(hashes)])
    ins.check(pieces)
    return ins, out


def upload_batch(O, ob, k, n, ess, stripes, seed):
    """per stripe count: (the padded segment, its n pieces by the oracle's encode_segment, their
    [n, 32] hashes by the oracle's BLAKE3)"""
    segs, refs = encode_segments(O, k, n, ess, stripes, seed)
    hashes = []
    for r in refs:
        h = ob.blake3_many(np.ascontiguousarray(r), threads=8) if r.shape[1] else np.zeros((n, 32), np.uint8)
        h.setflags(write=False)
        hashes.append(h)
    return segs, refs, hashes


def call_hash_sized(c, seg_ptrs, stripes, piece_ptrs, hash_ptr, parity_only=False, stream=None):
    nseg = len(stripes)
    a = lambda t, v: (t * max(nseg, 1))(*v)  # noqa: E731
    st = (stream or torch.cuda.current_stream()).cuda_stream
    return c.L.ec_hash_segments_sized(c.ctx, nseg, None if seg_ptrs is None else a(ctypes.c_void_p, seg_ptrs),
                                      a(ctypes.c_size_t, stripes), a(ctypes.c_void_p, piece_ptrs),
                                      _native.EC_FLAG_PARITY_ONLY if parity_only else 0, hash_ptr, st)


def run_upload_batch(c, segs, refs, hashes, stripes, parity_only=False):
    """one ec_encode_segments_sized and one ec_hash_segments_sized over the batch: pieces, the
    [nseg][n][32] hashes (a skipped segment's rows stay 0xCD), inputs and all guards compared whole"""
    ins = Ins(segs)
    outs = Outs(piece_sizes(c, stripes, parity_only))
    rc = call_encode(c, ins.ptrs, stripes, outs.ptrs, parity_only=parity_only)
    assert rc == 0, _native.strerror(rc)
    flat = Outs([32 * c.n * len(stripes)])  # [nseg][n][32], guarded
    rc = call_hash_sized(c, ins.ptrs, stripes, outs.ptrs, flat.ptrs[0], parity_only=parity_only)
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
    from oracle import blake3 as ob
    from oracle import oracle as O
    O.build()
    k, n, ess = 29, 80, 256
    c = Ctx(k, n, ess, L)
    pieces, hashes = edge_pieces(ob)
    run_list(c, pieces, hashes)
    run_list(c, pieces[::-1], hashes[::-1])
    segs, refs, hs = upload_batch(O, ob, k, n, ess, UPLOAD_STRIPES, 2982)
    for o in (list(range(len(segs))), list(range(len(segs)))[::-1]):
        for parity_only in (False, True):
            run_upload_batch(c, [segs[g] for g in o], [refs[g] for g in o], [hs[g] for g in o],
                             [UPLOAD_STRIPES[g] for g in o], parity_only=parity_only)
    c.close()
    print("ok", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
