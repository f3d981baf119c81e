"""Harness of tests/test_encode_sized.py, and -- run as a program -- the child
process of its test_checked_library: ec_encode_segments_sized against the
bounds-checked build of the library (every DMA source and every store of
rs_encode_sized compared with the segment's own input and piece extents; one
outside is skipped and reported on stderr as "uplink_ec checked: ...").  Prints
the library's build id first, then "ok"."""
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
from sized_checked_child import GUARD, Ctx, Outs, encode_segments  # noqa: E402,F401

# RS(29,80) ess 256, a block is 4 stripes: a quarter block, one stripe under a block, exactly
# a block and one over, two blocks and one over, a skipped segment, ragged 10.25 and 32.5 blocks
BLOCK_STRIPES = [1, 3, 4, 5, 8, 9, 0, 41, 130]


class Ins(Outs):
    """The segments in windows of one 0xCD-filled buffer (as Outs): compared whole after a
    call, so a write to an input or next to it shows"""

    def __init__(self, segs, shift=None, sizes=None):
        super().__init__(sizes or [len(s) for s in segs], shift)
        host = self.expect([s if len(s) == sz else np.concatenate([s, np.full(sz - len(s), 0xCD, np.uint8)])
                            for s, sz in zip(segs, self.sizes)])
        self.buf.copy_(torch.from_numpy(host))


def piece_sizes(c, stripes, parity_only=False):
    rows = c.n - c.k if parity_only else c.n
    return [rows * s * c.ess for s in stripes]


def expected(c, refs, parity_only=False):
    """per segment the bytes of its piece buffer"""
    return [np.ascontiguousarray(r[c.k:] if parity_only else r).reshape(-1) for r in refs]


def call_encode(c, in_ptrs, stripes, out_ptrs, data_len=None, parity_only=False, stream=None, null=()):
    """-> rc.  null: names of array arguments passed as NULL"""
    nseg = len(stripes)
    a = lambda t, v: (t * max(nseg, 1))(*v)  # noqa: E731
    st = (stream or torch.cuda.current_stream()).cuda_stream
    return c.L.ec_encode_segments_sized(
        c.ctx, nseg, None if "segs" in null else a(ctypes.c_void_p, in_ptrs),
        None if "nstripes" in null else a(ctypes.c_size_t, stripes),
        None if data_len is None else a(ctypes.c_size_t, data_len),
        None if "pieces" in null else a(ctypes.c_void_p, out_ptrs), _native.EC_FLAG_PARITY_ONLY if parity_only else 0, st)


def run_batch(c, segs, refs, stripes, parity_only=False, in_shift=None, out_shift=None):
    """encode the batch and compare every piece buffer and every input whole, guards included"""
    ins = Ins(segs, in_shift)
    outs = Outs(piece_sizes(c, stripes, parity_only), out_shift)
    rc = call_encode(c, ins.ptrs, stripes, outs.ptrs, parity_only=parity_only)
    assert rc == 0, _native.strerror(rc)
    torch.cuda.synchronize()
    outs.check(expected(c, refs, parity_only))
    ins.check(segs)
    return ins, outs


def block_batches():
    """(name, indices into BLOCK_STRIPES) of the block-edge batches: in order (54 blocks),
    reversed (a tile's two blocks in other segments), without the 1-stripe segment (53
    blocks: the last tile has no second block)"""
    o = list(range(len(BLOCK_STRIPES)))
    return [("in order", o), ("reversed", o[::-1]), ("53 blocks", o[1:])]


def main():
    L = _native.load(os.path.join(ROOT, "uplink_amd", "lib", "checked", "libuplink_ec_checked.so"))
    print("build", L.ec_build_id().decode(), flush=True)
    if len(sys.argv) > 1 and sys.argv[1] == "--build-id":
        return 0
    from oracle import oracle as O
    O.build()
    k, n, ess = 29, 80, 256
    segs, refs = encode_segments(O, k, n, ess, BLOCK_STRIPES, 2981)
    c = Ctx(k, n, ess, L)
    for _, o in block_batches():
        run_batch(c, [segs[g] for g in o], [refs[g] for g in o], [BLOCK_STRIPES[g] for g in o])
    o = block_batches()[1][1]
    run_batch(c, [segs[g] for g in o], [refs[g] for g in o], [BLOCK_STRIPES[g] for g in o], parity_only=True)
    c.close()
    c = Ctx(k, n, ess, L)  # a single tile whose only block is ragged
    run_batch(c, segs[:1], refs[:1], [1])
    c.close()
    print("ok", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
