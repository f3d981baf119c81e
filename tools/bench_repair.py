#!/usr/bin/env python3
"""Segment repair, direct against the two-step path (DESIGN.md "Segment repair").

32 RS(29,80) 64 MiB segments per launch, ess 256, each with a fresh seeded
29-subset of its pieces; the targets are the 51 other pieces, the first 45 of
them, and the first 3.

  * direct: ec_repair_segments_sets, one call per launch.
  * two-step: ec_rebuild_segments_sets into stripe-major segments, then
    ec_encode_segments with EC_FLAG_PARITY_ONLY, then a gather of the wanted
    rows (data pieces out of the rebuilt segment, parity pieces out of the
    parity buffer) into the layout the direct call writes.

Both run in this process on the same inputs, alternating in blocks, each block
timed by HIP events on the stream, until each has at least --seconds of work;
every shape is warmed first.  The two-step path's two launches are also timed
without the gather (its floor, whatever gathers the rows).  The direct call's
outputs must equal the two-step path's.  Prints one JSON line.  Run on the GPU box:
    python tools/bench_repair.py [--seconds S] [--nseg N] [--dump-outputs DIR]"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from uplink_amd import _native  # noqa: E402

K, N, ESS = 29, 80, 256
NSTRIPES = (64 * 2**20 + 4 + K * ESS - 1) // (K * ESS)
SPAD, PLEN = NSTRIPES * K * ESS, NSTRIPES * ESS
PEAK = 8000.0  # GB/s, HBM3E peak the other tools' fractions use
POOL = 4       # share-set draws cycled over the launches of a block


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0, help="device time per path and target count, at least")
    ap.add_argument("--nseg", type=int, default=32)
    ap.add_argument("--targets", type=int, nargs="*", default=[51, 45, 3])
    ap.add_argument("--rounds", type=int, default=4, help="alternations of the two paths per target count")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the byte sums of every regenerated piece of the last direct launch per target count "
                         "as DIR/repair_bytesum_m<targets>.npy (float64 [nseg][targets])")
    ap.add_argument("--lib", default=_native.LIB_PATH, help="another build of libuplink_ec.so (A/B runs of library variants)")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    L = _native.load(args.lib)
    ctx = ctypes.c_void_p()
    assert L.ec_create(K, N, ESS, ctypes.byref(ctx)) == 0
    dev = torch.device("cuda", 0)
    nseg = args.nseg
    st = torch.cuda.current_stream()
    sptr = st.cuda_stream
    segs = torch.randint(0, 256, (nseg, SPAD), dtype=torch.uint8, device=dev)
    pcs = torch.empty((nseg, N, PLEN), dtype=torch.uint8, device=dev)
    assert L.ec_encode_segments(ctx, segs.data_ptr(), nseg, NSTRIPES, pcs.data_ptr(), 0, sptr) == 0
    torch.cuda.synchronize()
    del segs
    mmax = max(args.targets)
    direct = torch.empty((nseg, mmax, PLEN), dtype=torch.uint8, device=dev)
    rebuilt = torch.empty((nseg, SPAD), dtype=torch.uint8, device=dev)
    parity = torch.empty((nseg, N - K, PLEN), dtype=torch.uint8, device=dev)
    gathered = torch.empty((nseg, mmax, PLEN), dtype=torch.uint8, device=dev)
    rng = np.random.default_rng(2980)

    def draw(m):
        """per segment a fresh 29-subset (shuffled) and its first m other pieces"""
        out = []
        for _ in range(nseg):
            perm = [int(x) for x in rng.permutation(N)]
            out.append((perm[:K], sorted(perm[K:])[:m]))
        return out

    def direct_args(cases):
        m = len(cases[0][1])
        flat = [x for s, _ in cases for x in s]
        tflat = [x for _, t in cases for x in t]
        return (nseg, (ctypes.c_int * nseg)(*[K] * nseg), (ctypes.c_int * len(flat))(*flat),
                (ctypes.c_void_p * len(flat))(*[pcs[g, x].data_ptr() for g, (s, _) in enumerate(cases) for x in s]),
                (ctypes.c_int * nseg)(*[m] * nseg), (ctypes.c_int * len(tflat))(*tflat),
                (ctypes.c_void_p * len(tflat))(*[direct[g, i].data_ptr() for g in range(nseg) for i in range(m)]))

    def two_args(cases):
        flat = [x for s, _ in cases for x in s]
        sets = (nseg, (ctypes.c_int * nseg)(*[K] * nseg), (ctypes.c_int * len(flat))(*flat),
                (ctypes.c_void_p * len(flat))(*[pcs[g, x].data_ptr() for g, (s, _) in enumerate(cases) for x in s]))
        optr = (ctypes.c_void_p * nseg)(*[rebuilt[g].data_ptr() for g in range(nseg)])
        # the gather's index tensors, made ahead of the timed calls
        gat = []
        for g, (_, t) in enumerate(cases):
            dt = [x for x in t if x < K]
            pt = [x - K for x in t if x >= K]
            gat.append((torch.tensor(dt, dtype=torch.long, device=dev), len(dt),
                        torch.tensor(pt, dtype=torch.long, device=dev), len(pt)))
        return sets, optr, gat

    def go_direct(a):
        rc = L.ec_repair_segments_sets(ctx, a[0], a[1], a[2], a[3], a[4], a[5], a[6], NSTRIPES, 0, None, sptr)
        assert rc == 0, _native.strerror(rc)

    def go_two(a, gather=True):
        sets, optr, gat = a
        rc = L.ec_rebuild_segments_sets(ctx, sets[0], sets[1], sets[2], sets[3], NSTRIPES, optr, sptr)
        assert rc == 0, _native.strerror(rc)
        rc = L.ec_encode_segments(ctx, rebuilt.data_ptr(), nseg, NSTRIPES, parity.data_ptr(),
                                  _native.EC_FLAG_PARITY_ONLY, sptr)
        assert rc == 0, _native.strerror(rc)
        if not gather:
            return
        for g, (di, nd, pi, npar) in enumerate(gat):
            if nd:  # data piece t: share t of every stripe of the rebuilt segment
                src = rebuilt[g].view(NSTRIPES, K, ESS).index_select(1, di)
                gathered[g, :nd].view(nd, NSTRIPES, ESS).copy_(src.permute(1, 0, 2))
            if npar:
                torch.index_select(parity[g], 0, pi, out=gathered[g, nd:nd + npar])

    def timed(fn, arg_pool, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for i in range(reps):
            fn(arg_pool[i % len(arg_pool)])
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / reps

    res, ok_all = {}, True
    for m in args.targets:
        pools = [draw(m) for _ in range(POOL)]
        d_pool = [direct_args(c) for c in pools]
        t_pool = [two_args(c) for c in pools]
        # warm-up of both paths on this shape, and the comparison of their outputs (sorted targets:
        # data pieces first, then parity, the order the gather writes)
        for a, b in zip(d_pool, t_pool):
            go_direct(a)
            go_two(b)
        direct.zero_()
        gathered.fill_(0xFF)
        go_direct(d_pool[-1])
        go_two(t_pool[-1])
        torch.cuda.synchronize()
        equal = bool(torch.equal(direct[:, :m], gathered[:, :m]))
        if args.dump_outputs:
            os.makedirs(args.dump_outputs, exist_ok=True)
            sums = torch.stack([direct[g, :m].sum(dim=1, dtype=torch.float64) for g in range(nseg)])
            np.save(os.path.join(args.dump_outputs, f"repair_bytesum_m{m}.npy"), sums.cpu().numpy())
        # reps per block from a first measurement, so that `rounds` blocks give the asked seconds
        td, tt = timed(go_direct, d_pool, 4), timed(go_two, t_pool, 4)
        rd = max(4, int(np.ceil(args.seconds / args.rounds / td)))
        rt = max(4, int(np.ceil(args.seconds / args.rounds / tt)))
        per_d, per_t, per_n = [], [], []
        while len(per_d) < args.rounds or min(sum(per_d) * rd, sum(per_t) * rt) < args.seconds:
            per_d.append(timed(go_direct, d_pool, rd))
            per_t.append(timed(go_two, t_pool, rt))
            # (the two launches alone, the gather left out: the two-step path's floor)
            per_n.append(timed(lambda a: go_two(a, gather=False), t_pool, max(4, rt // 4)))
        td, tt, tn = float(np.median(per_d)), float(np.median(per_t)), float(np.median(per_n))
        alg = nseg * (K + m) * PLEN
        faster = td < tt
        ok_all = ok_all and faster and equal
        res[str(m)] = {"direct_us_per_call": round(td * 1e6, 1), "two_step_us_per_call": round(tt * 1e6, 1),
                       "direct_us_rounds": [round(x * 1e6, 1) for x in per_d],
                       "two_step_us_rounds": [round(x * 1e6, 1) for x in per_t],
                       "direct_seconds_timed": round(sum(per_d) * rd, 3), "two_step_seconds_timed": round(sum(per_t) * rt, 3),
                       "two_step_without_gather_us_per_call": round(tn * 1e6, 1),
                       "two_step_over_direct": round(tt / td, 3), "two_launches_over_direct": round(tn / td, 3), "algorithmic_GBps": round(alg / td / 1e9, 1),
                       "frac_of_peak": round(alg / td / 1e9 / PEAK, 4), "outputs_equal": equal, "direct_faster": faster}
    torch.cuda.synchronize()
    L.ec_destroy(ctx)
    print(json.dumps({"tool": "bench_repair", "code": [K, N], "ess": ESS, "nstripes": NSTRIPES, "segments_per_call": nseg,
                      "build": L.ec_build_id().decode(), "targets": res, "pass": bool(ok_all)}))
    return 0 if ok_all else 1


if __name__ == "__main__":
    sys.exit(main())
