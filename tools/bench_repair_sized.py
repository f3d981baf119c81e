#!/usr/bin/env python3
"""Segment repair of a queue of segments of different sizes in one call
(ec_repair_segments_sized) against what a caller does without it: its queue
sorted by size and one ec_repair_segments_sets call per distinct size
(DESIGN.md §4l).  RS(29,80), ess 256.

Per segment a seeded count of healthy pieces in 29..35 (at most the repair
threshold of the 29/35/65/80 scheme), a shuffled set of that many piece
numbers, and as targets every other piece: SegmentRepairer's rule, 45..51
targets, so every segment is in the 8-wave class.  All healthy pieces are
given; without the share check the call reads the 29 it chooses.

  queue   256 segments with stripe counts seeded log-uniform in 8..560 (64 KiB
          - 4 MiB of plaintext: small objects are one short segment each and
          the last segment of every object has its own size, so short segments
          dominate a repair queue by count and the sizes hardly repeat) plus 8
          of 9060 stripes (the full 64 MiB segments of large objects, which
          dominate it by bytes), in seeded order
  equal   32 x 9060 stripes through both calls, one call each: what the lookup
          of a tile's segment through the map costs

The arms alternate in this process on the same inputs, each block timed by HIP
events on the stream, until each has at least --seconds of device time and
--rounds blocks; every shape is warmed first, and every arm's outputs must
equal the other's and the pieces the engine's encode wrote.  Reported per
workload and arm: device us per batch (median, min-max over the blocks), host
wall us per batch (the time the calls take to return), and the ratios; for
`equal` also the difference of the medians next to the existing call's own
run-to-run spread (max - min of its blocks).  Prints one JSON line.  Run on the
GPU box:
    python tools/bench_repair_sized.py [--seconds S] [--workloads queue equal]"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from uplink_amd import _native, eestream, repair  # noqa: E402

K, N, ESS = 29, 80, 256
REPAIR, OPTIMAL = 35, 65
BIG = 9060


class _Sizes:
    """The scheme's counts, for SegmentRepairer's thresholds (no context of its own)."""

    def total_count(self):
        return N

    def required_count(self):
        return K


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0, help="device time per arm and workload, at least")
    ap.add_argument("--rounds", type=int, default=7, help="alternations of the two arms per workload, at least")
    ap.add_argument("--workloads", nargs="*", default=["queue", "equal"])
    ap.add_argument("--lib", default=_native.LIB_PATH, help="another build of libuplink_ec.so (A/B runs of library variants)")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    L = _native.load(args.lib)
    ctx = ctypes.c_void_p()
    assert L.ec_create(K, N, ESS, ctypes.byref(ctx)) == 0
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream()
    sptr = st.cuda_stream
    rng = np.random.default_rng(2980)
    rep = repair.SegmentRepairer(eestream.RedundancyStrategy(_Sizes(), REPAIR, OPTIMAL))
    small = [int(round(x)) for x in np.exp(rng.uniform(np.log(8), np.log(560), 256))]
    queue = small + [BIG] * 8
    queue = [queue[i] for i in rng.permutation(len(queue))]
    shapes = {"queue": queue, "equal": [BIG] * 32}

    def make(stripes):
        """per segment: its healthy piece numbers, those pieces, its targets, and the targets' pieces as encoded"""
        out = []
        for s in stripes:
            seg = torch.randint(0, 256, (s * K * ESS,), dtype=torch.uint8, device=dev)
            pcs = torch.empty((N, s * ESS), dtype=torch.uint8, device=dev)
            assert L.ec_encode_segments(ctx, seg.data_ptr(), 1, s, pcs.data_ptr(), 0, sptr) == 0
            healthy = [int(x) for x in rng.permutation(N)[:int(rng.integers(K, REPAIR + 1))]]
            targets = rep.targets(healthy)
            assert len(targets) == N - len(healthy)
            out.append((healthy, pcs[healthy].clone(), targets, pcs[targets].clone()))
            torch.cuda.synchronize()
            del pcs, seg
        return out

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        wall = (time.perf_counter() - t0) / reps
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / reps, wall

    def call_args(data, stripes, outs, idx):
        """the arguments both calls share for segments idx of the workload"""
        flat = [x for g in idx for x in data[g][0]]
        tflat = [x for g in idx for x in data[g][2]]
        n = len(idx)
        return (n, (ctypes.c_int * n)(*[len(data[g][0]) for g in idx]), (ctypes.c_int * len(flat))(*flat),
                (ctypes.c_void_p * len(flat))(*[data[g][1][i].data_ptr() for g in idx for i in range(len(data[g][0]))]),
                (ctypes.c_int * n)(*[len(data[g][2]) for g in idx]), (ctypes.c_int * len(tflat))(*tflat),
                (ctypes.c_void_p * len(tflat))(*[outs[g][i].data_ptr() for g in idx for i in range(len(data[g][2]))]),
                (ctypes.c_size_t * n)(*[stripes[g] for g in idx]))

    res, all_equal = {}, True
    for name in args.workloads:
        stripes = shapes[name]
        nseg = len(stripes)
        data = make(stripes)
        outs_a = [torch.zeros((len(t), s * ESS), dtype=torch.uint8, device=dev) for (_, _, t, _), s in zip(data, stripes)]
        outs_b = [torch.full((len(t), s * ESS), 0xFF, dtype=torch.uint8, device=dev)
                  for (_, _, t, _), s in zip(data, stripes)]
        a = call_args(data, stripes, outs_a, list(range(nseg)))
        # the queue sorted by size: one ec_repair_segments_sets call per distinct size
        by_size = {}
        for g, s in enumerate(stripes):
            by_size.setdefault(s, []).append(g)
        b_calls = [(s, call_args(data, stripes, outs_b, idx)) for s, idx in sorted(by_size.items())]

        def go_sized():
            rc = L.ec_repair_segments_sized(ctx, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], 0, None, sptr)
            assert rc == 0, _native.strerror(rc)

        def go_per_size():
            for s, b in b_calls:
                rc = L.ec_repair_segments_sets(ctx, b[0], b[1], b[2], b[3], b[4], b[5], b[6], s, 0, None, sptr)
                assert rc == 0, _native.strerror(rc)

        for _ in range(3):
            go_sized()
            go_per_size()
        torch.cuda.synchronize()
        equal = all(torch.equal(x, y) and torch.equal(x, want) for x, y, (_, _, _, want) in zip(outs_a, outs_b, data))
        all_equal = all_equal and equal
        ta, tb = timed(go_sized, 3)[0], timed(go_per_size, 3)[0]
        ra = max(3, int(np.ceil(args.seconds / args.rounds / ta)))
        rb = max(3, int(np.ceil(args.seconds / args.rounds / tb)))
        per_a, per_b, wall_a, wall_b = [], [], [], []
        while len(per_a) < args.rounds or min(sum(per_a) * ra, sum(per_b) * rb) < args.seconds:
            t, w = timed(go_sized, ra)
            per_a.append(t), wall_a.append(w)
            t, w = timed(go_per_size, rb)
            per_b.append(t), wall_b.append(w)
        # bytes the repair has to move: the 29 basis pieces in, the targets out
        alg = float(sum((K + len(t)) * s * ESS for (_, _, t, _), s in zip(data, stripes)))

        def arm(per, wall, reps):
            med = float(np.median(per))
            return {"device_us_per_batch": round(med * 1e6, 1),
                    "device_us_min_max": [round(min(per) * 1e6, 1), round(max(per) * 1e6, 1)],
                    "device_us_blocks": [round(x * 1e6, 1) for x in per],
                    "host_wall_us_per_batch": round(float(np.median(wall)) * 1e6, 1),
                    "algorithmic_GBps": round(alg / med / 1e9, 1), "blocks": len(per), "batches_per_block": reps,
                    "seconds_timed": round(sum(per) * reps, 3)}

        A, B = arm(per_a, wall_a, ra), arm(per_b, wall_b, rb)
        r = {"segments": nseg, "distinct_sizes": len(by_size), "stripes_total": int(sum(stripes)),
             "stripes_min_max": [min(stripes), max(stripes)],
             "targets_min_max": [min(len(d[2]) for d in data), max(len(d[2]) for d in data)],
             "sized": A, "sets_per_size": B, "sets_calls_per_batch": len(b_calls),
             "sets_over_sized_device": round(B["device_us_per_batch"] / A["device_us_per_batch"], 3),
             "sets_over_sized_host_wall": round(B["host_wall_us_per_batch"] / A["host_wall_us_per_batch"], 3),
             "sized_host_wall_us_per_segment": round(A["host_wall_us_per_batch"] / nseg, 2),
             "outputs_equal": bool(equal)}
        if len(by_size) == 1:
            spread = B["device_us_min_max"][1] - B["device_us_min_max"][0]
            diff = A["device_us_per_batch"] - B["device_us_per_batch"]
            r.update({"sized_minus_sets_device_us": round(diff, 1), "sets_spread_device_us": round(spread, 1),
                      "sized_slower_by_more_than_the_spread": bool(diff > spread)})
        res[name] = r
        del data, outs_a, outs_b, a, b_calls
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    L.ec_destroy(ctx)
    print(json.dumps({"tool": "bench_repair_sized", "code": [K, N], "ess": ESS, "build": L.ec_build_id().decode(),
                      "workloads": res, "outputs_equal": bool(all_equal)}))
    return 0 if all_equal else 1


if __name__ == "__main__":
    sys.exit(main())
