"""Harness of tests/test_sized.py, and -- run as a program -- the child process
of its test_checked_library: the sized share-set calls against the
bounds-checked build of the library (every DMA source and every store of
rs_matmul_sized compared with the segment's own share and output extents; one
outside is skipped and reported on stderr as "uplink_ec checked: ...").  Prints
the library's build id first, then "ok"."""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from uplink_amd import _native  # noqa: E402

GUARD = 64
# less than half a tile; the vB boundary at 64 chunks; one tile minus, exactly and plus one
# stripe; two tiles exactly and plus one; a ragged 5.1 tiles; a skipped segment; 16.25 tiles
EDGE_STRIPES = [1, 4, 5, 7, 8, 9, 16, 17, 41, 0, 130]


class Ctx:
    def __init__(self, k, n, ess, lib=None):
        self.L = lib or _native.load()
        self.k, self.n, self.ess = k, n, ess
        self.ctx = ctypes.c_void_p()
        assert self.L.ec_create(k, n, ess, ctypes.byref(self.ctx)) == 0

    def close(self):
        torch.cuda.synchronize()
        self.L.ec_destroy(self.ctx)


def encode_segments(oracle, k, n, ess, stripes, seed):
    """per stripe count: (the segment, its n pieces [n, stripes*ess] by the oracle); 0 stripes: empty"""
    rng = np.random.default_rng(seed)
    f = oracle.FEC(k, n)
    segs, refs = [], []
    for s in stripes:
        seg = rng.integers(0, 256, s * k * ess, dtype=np.uint8)
        ref = f.encode_segment(seg, ess, threads=8) if s else np.zeros((n, 0), dtype=np.uint8)
        seg.setflags(write=False)
        ref.setflags(write=False)
        segs.append(seg)
        refs.append(ref)
    return segs, refs


def to_device(refs):
    return [torch.tensor(r).cuda() for r in refs]  # (copies: the references stay read-only)


class Outs:
    """One 0xCD-filled device buffer with a window per segment (sizes[g] bytes, shift[g]
    bytes past 16-byte alignment), GUARD bytes before, between and after"""

    def __init__(self, sizes, shift=None):
        self.sizes = list(sizes)
        shift = shift or [0] * len(self.sizes)
        self.offs, at = [], GUARD
        for sz, sh in zip(self.sizes, shift):
            self.offs.append(at + sh)
            at += sh + sz + GUARD + (-(sh + sz) % 16)
        self.buf = torch.full((at,), 0xCD, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.ptrs = [self.buf.data_ptr() + o if sz else None for o, sz in zip(self.offs, self.sizes)]

    def expect(self, segs):
        """the whole buffer with window g holding segs[g] (None: untouched)"""
        want = np.full(self.buf.numel(), 0xCD, dtype=np.uint8)
        for g, sg in enumerate(segs):
            if sg is not None:
                assert len(sg) == self.sizes[g]
                want[self.offs[g]:self.offs[g] + self.sizes[g]] = sg
        return want

    def check(self, segs, skip=()):
        """the whole buffer, guards included; windows in `skip` may hold anything"""
        got = self.buf.cpu().numpy()
        want = self.expect(segs)
        for g in skip:
            got[self.offs[g]:self.offs[g] + self.sizes[g]] = want[self.offs[g]:self.offs[g] + self.sizes[g]]
        if not np.array_equal(got, want):
            w = int(np.flatnonzero(got != want)[0])
            g = max([i for i, o in enumerate(self.offs) if o - GUARD <= w], default=0)
            raise AssertionError(f"first difference at byte {w} (window {g}, offset {w - self.offs[g]} of "
                                 f"{self.sizes[g]}): {got[w]:#x} != {want[w]:#x}")


def call_sized(c, pieces, sets, stripes, outs=None, decode=False, want_rc=True, stream=None, null_stripes=False):
    """sets[g]: share numbers of segment g, its pieces pieces[g][number] (tensors; None: a NULL
    pointer).  Returns (rc, outs, per-segment codes or None)."""
    nseg = len(sets)
    outs = outs or Outs([s * c.k * c.ess for s in stripes])
    flat = [x for s in sets for x in s]
    ptrs = [None if pieces[g][x] is None else pieces[g][x].data_ptr() for g, s in enumerate(sets) for x in s]
    a_ns = (ctypes.c_int * nseg)(*[len(s) for s in sets])
    a_nums = (ctypes.c_int * max(len(flat), 1))(*flat)
    a_ptrs = (ctypes.c_void_p * max(len(flat), 1))(*ptrs)
    a_st = None if null_stripes else (ctypes.c_size_t * nseg)(*stripes)
    a_outs = (ctypes.c_void_p * nseg)(*outs.ptrs)
    st = (stream or torch.cuda.current_stream()).cuda_stream
    if not decode:
        return c.L.ec_rebuild_segments_sized(c.ctx, nseg, a_ns, a_nums, a_ptrs, a_st, a_outs, st), outs, None
    codes = (ctypes.c_int * nseg)(*[99] * nseg) if want_rc else None
    rc = c.L.ec_decode_segments_sized(c.ctx, nseg, a_ns, a_nums, a_ptrs, a_st, a_outs, codes, st)
    return rc, outs, (list(codes) if want_rc else None)


def shuffled_subset(rng, n, count):
    return [int(x) for x in rng.permutation(n)[:count]]


def missing_set(rng, k, n, m):
    """a shuffled k-subset with exactly m data shares missing"""
    data = shuffled_subset(rng, k, k - m)
    parity = [k + int(x) for x in rng.permutation(n - k)[:m]]
    both = data + parity
    return [both[i] for i in rng.permutation(k)]


def edge_sets(rng, k=29, n=80):
    """the share sets of the tile-edge batch (one per EDGE_STRIPES entry): shuffled
    k-subsets of their own, one with every data share present, one all parity {51..79},
    one with more than k shares; the skipped segment has too few"""
    sets = [shuffled_subset(rng, n, k) for _ in EDGE_STRIPES]
    sets[3] = shuffled_subset(rng, k, k)
    sets[5] = [51 + x for x in shuffled_subset(rng, k, k)]
    sets[8] = shuffled_subset(rng, n, k + 6)
    sets[9] = [7, 3, 60]
    return sets


def main():
    L = _native.load(os.path.join(ROOT, "uplink_amd", "lib", "checked", "libuplink_ec_checked.so"))
    print("build", L.ec_build_id().decode(), flush=True)
    if len(sys.argv) > 1 and sys.argv[1] == "--build-id":
        return 0
    from oracle import oracle as O
    O.build()
    k, n, ess = 29, 80, 256
    segs, refs = encode_segments(O, k, n, ess, EDGE_STRIPES, 2980)
    d = to_device(refs)
    c = Ctx(k, n, ess, L)
    rng = np.random.default_rng(11)
    sets = edge_sets(rng)
    order = list(range(len(sets)))
    for o in (order, order[::-1]):
        rc, outs, _ = call_sized(c, [d[g] for g in o], [sets[g] for g in o], [EDGE_STRIPES[g] for g in o])
        assert rc == 0, rc
        torch.cuda.synchronize()
        outs.check([segs[g] for g in o])
    # a Decode batch: k + 2 shares each, clean, then one piece of the 9-stripe segment damaged in
    # its last 16-byte chunk
    pick = [0, 5, 8, 7]  # 1, 9, 41, 17 stripes
    dsets = [shuffled_subset(rng, n, k + 2) for _ in pick]
    dp = [d[g].clone() for g in pick]
    st = [EDGE_STRIPES[g] for g in pick]
    for damage in (False, True):
        if damage:
            dp[1][dsets[1][4]][-3] ^= 0x5A
        rc, outs, codes = call_sized(c, dp, dsets, st, decode=True)
        assert rc == 0 and codes == [0, 0, 0, 0], (rc, codes)
        outs.check([segs[g] for g in pick])
        for i, g in enumerate(pick):
            assert torch.equal(dp[i].cpu(), torch.from_numpy(np.array(refs[g]))), g
    c.close()
    print("ok", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
