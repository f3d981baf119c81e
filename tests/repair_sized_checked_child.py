"""Harness of tests/test_repair_sized.py, and -- run as a program -- the child
process of its test_checked_library: ec_repair_segments_sized against the
bounds-checked build of the library (every DMA source and every row store of
rs_repair_sized compared with the segment's own share and output extents; one
outside is skipped and reported on stderr as "uplink_ec checked: ...").  Prints
the library's build id first, then "ok"."""
import ctypes
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import sized_checked_child as S  # noqa: E402
from uplink_amd import _native  # noqa: E402

Ctx, Outs, encode_segments, to_device, shuffled_subset = S.Ctx, S.Outs, S.encode_segments, S.to_device, S.shuffled_subset
CHECK = _native.EC_FLAG_CHECK_SHARES
# RS(29,80) ess 256, 8 stripes per tile: less than half a tile; the vB boundary at 64 chunks; one
# tile minus, exactly and plus one stripe; two tiles exactly and plus one; a ragged 5.1 tiles; a
# segment of no stripes (skipped); 16.25 tiles; and one more of 8 stripes that gets no targets
EDGE_STRIPES = S.EDGE_STRIPES + [8]
# targets per segment of the tile-edge batch: 1 .. all 51 lost, every wave class
EDGE_TARGETS = [1, 51, 14, 15, 24, 25, 32, 33, 45, 2, 8, 0]


def call_repair_sized(c, pieces, sets, targets, stripes, outs=None, flags=0, status=None, stream=None,
                      null_stripes=False):
    """sets[g] / targets[g]: share and target numbers of segment g, its pieces pieces[g][number]
    (tensors; None: a NULL pointer), its outputs one window of `outs` per target.  Returns (rc, outs)."""
    nseg = len(sets)
    outs = outs or Outs([stripes[g] * c.ess for g, t in enumerate(targets) for _ in t])
    flat = [x for s in sets for x in s]
    tflat = [x for t in targets for x in t]
    ptrs = [None if pieces[g][x] is None else pieces[g][x].data_ptr() for g, s in enumerate(sets) for x in s]
    rc = c.L.ec_repair_segments_sized(
        c.ctx, nseg, (ctypes.c_int * nseg)(*[len(s) for s in sets]), (ctypes.c_int * max(len(flat), 1))(*flat),
        (ctypes.c_void_p * max(len(flat), 1))(*ptrs), (ctypes.c_int * nseg)(*[len(t) for t in targets]),
        (ctypes.c_int * max(len(tflat), 1))(*tflat), (ctypes.c_void_p * max(len(tflat), 1))(*outs.ptrs),
        None if null_stripes else (ctypes.c_size_t * nseg)(*stripes), flags,
        status.data_ptr() if status is not None else None, (stream or torch.cuda.current_stream()).cuda_stream)
    return rc, outs


def expected(refs, targets):
    """the windows' contents: the oracle's piece per target (None where the segment has no bytes)"""
    return [refs[g][t] if refs[g].shape[1] else None for g, ts in enumerate(targets) for t in ts]


def random_case(rng, k, n, count, extra=0):
    """a shuffled (k + extra)-subset and `count` shuffled targets among the other pieces"""
    perm = [int(x) for x in rng.permutation(n)]
    nums, rest = perm[:k + extra], perm[k + extra:]
    assert count <= len(rest)
    return nums, rest[:count]


def edge_cases(rng, extra=0, k=29, n=80):
    """share and target sets of the tile-edge batch, one per EDGE_STRIPES entry: shuffled sets of
    their own; the segment of no stripes has too few shares, which nobody looks at"""
    cases = [random_case(rng, k, n, min(cnt, n - k - extra), extra) for cnt in EDGE_TARGETS]
    cases[9] = ([7, 3, 60], [1, 2])
    return [s for s, _ in cases], [t for _, t in cases]


def edge_pieces(d):
    """the device pieces per segment as call_repair_sized takes them; the segment of no stripes: NULL"""
    return [{x: (t[x] if t.shape[1] else None) for x in range(t.shape[0])} for t in d]


def pieces_unchanged(d, refs):
    for g, (t, r) in enumerate(zip(d, refs)):
        assert np.array_equal(t.cpu().numpy(), r), f"the pieces of segment {g} were written"


def main():
    L = _native.load(os.path.join(ROOT, "uplink_amd", "lib", "checked", "libuplink_ec_checked.so"))
    print("build", L.ec_build_id().decode(), flush=True)
    if len(sys.argv) > 1 and sys.argv[1] == "--build-id":
        return 0
    from oracle import oracle as O
    O.build()
    k, n, ess = 29, 80, 256
    _, refs = encode_segments(O, k, n, ess, EDGE_STRIPES, 2980)
    d = to_device(refs)
    c = Ctx(k, n, ess, L)
    order = list(range(len(EDGE_STRIPES)))
    for o, extra in ((order, 0), (order[::-1], 0), (order, 3)):
        sets, targets = edge_cases(np.random.default_rng(11 + extra), extra)
        status = torch.full((len(o),), 7, dtype=torch.int32, device="cuda") if extra else None
        rc, outs = call_repair_sized(c, edge_pieces([d[g] for g in o]), [sets[g] for g in o], [targets[g] for g in o],
                                     [EDGE_STRIPES[g] for g in o], flags=CHECK if extra else 0, status=status)
        assert rc == 0, rc
        torch.cuda.synchronize()
        outs.check(expected([refs[g] for g in o], [targets[g] for g in o]))
        assert status is None or status.cpu().tolist() == [0] * len(o)
    pieces_unchanged(d, refs)
    c.close()
    print("ok", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
