#!/usr/bin/env python3
"""Encode of segments of different sizes in one call (ec_encode_segments_sized)
against the forms available without it.  RS(29,80), ess 256,
the three workloads of tools/bench_sized.py (the same seeded draw).

  small   256 segments, stripe counts seeded log-uniform in 8..560 (64 KiB - 4 MiB),
          against one ec_encode_segments call per segment on the same stream
          with no host waits between
  mixed   the 24 smallest of those, smallest first, plus 8 of 9040 stripes,
          against the same per-segment calls
  equal   32 x 9040 stripes, against one ec_encode_segments call with nseg = 32

The arms alternate in this process on the same inputs, each block timed by HIP
events on the stream, until each has at least --seconds of device time; every
shape is warmed first and every arm's pieces must equal the other's.  Reported
per workload and arm: device us per batch (median, min-max over the blocks),
host wall us per batch (the time the calls take to return), algorithmic GB/s
(sum of nstripes * (k + n) * ess over the device time: the segment read, its n
pieces written), the ratios, and whether the sized call's device time was below
the other arm's in every alternation.  Prints one JSON line.  Run on the GPU box:
    python tools/bench_encode_sized.py [--seconds S] [--workloads small mixed equal]"""
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
from uplink_amd import _native  # noqa: E402

K, N, ESS = 29, 80, 256
BIG = 9040


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0, help="device time per arm and workload, at least")
    ap.add_argument("--rounds", type=int, default=5, help="alternations of the two arms per workload, at least")
    ap.add_argument("--workloads", nargs="*", default=["small", "mixed", "equal"])
    args = ap.parse_args()
    torch.cuda.set_device(0)
    L = _native.load()
    ctx = ctypes.c_void_p()
    assert L.ec_create(K, N, ESS, ctypes.byref(ctx)) == 0
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream()
    sptr = st.cuda_stream
    rng = np.random.default_rng(2980)
    small = sorted(int(round(x)) for x in np.exp(rng.uniform(np.log(8), np.log(560), 256)))
    small_order = [small[i] for i in rng.permutation(256)]
    shapes = {"small": small_order, "mixed": small[:24] + [BIG] * 8, "equal": [BIG] * 32}

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

    res, all_equal = {}, True
    for name in args.workloads:
        stripes = shapes[name]
        nseg = len(stripes)
        # (the equal workload's segments in one buffer: the uniform call takes them by stride)
        seg_all = torch.randint(0, 256, (sum(stripes) * K * ESS,), dtype=torch.uint8, device=dev)
        out_a = torch.zeros(sum(stripes) * N * ESS, dtype=torch.uint8, device=dev)
        out_b = torch.full((sum(stripes) * N * ESS,), 0xFF, dtype=torch.uint8, device=dev)
        starts = np.concatenate([[0], np.cumsum(stripes)])[:-1]
        in_ptrs = [seg_all.data_ptr() + int(s0) * K * ESS for s0 in starts]
        a_ptrs = [out_a.data_ptr() + int(s0) * N * ESS for s0 in starts]
        b_ptrs = [out_b.data_ptr() + int(s0) * N * ESS for s0 in starts]
        c_in = (ctypes.c_void_p * nseg)(*in_ptrs)
        c_st = (ctypes.c_size_t * nseg)(*stripes)
        c_out = (ctypes.c_void_p * nseg)(*a_ptrs)

        def go_sized():
            rc = L.ec_encode_segments_sized(ctx, nseg, c_in, c_st, None, c_out, 0, sptr)
            assert rc == 0, _native.strerror(rc)

        def go_per_segment():
            for g in range(nseg):
                rc = L.ec_encode_segments(ctx, in_ptrs[g], 1, stripes[g], b_ptrs[g], 0, sptr)
                assert rc == 0, _native.strerror(rc)

        def go_one_uniform_call():
            rc = L.ec_encode_segments(ctx, in_ptrs[0], nseg, BIG, b_ptrs[0], 0, sptr)
            assert rc == 0, _native.strerror(rc)

        other, other_name = (go_one_uniform_call, "one ec_encode_segments call, nseg = 32") if name == "equal" else \
            (go_per_segment, "one ec_encode_segments call per segment")
        for _ in range(3):
            go_sized()
            other()
        torch.cuda.synchronize()
        equal = bool(torch.equal(out_a, out_b))
        all_equal = all_equal and equal
        ta, tb = timed(go_sized, 3)[0], timed(other, 3)[0]
        ra = max(3, int(np.ceil(args.seconds / args.rounds / ta)))
        rb = max(3, int(np.ceil(args.seconds / args.rounds / tb)))
        per_a, per_b, wall_a, wall_b = [], [], [], []
        while len(per_a) < args.rounds or min(sum(per_a) * ra, sum(per_b) * rb) < args.seconds:
            t, w = timed(go_sized, ra)
            per_a.append(t), wall_a.append(w)
            t, w = timed(other, rb)
            per_b.append(t), wall_b.append(w)
        alg = float(sum(stripes)) * (K + N) * ESS

        def arm(per, wall, reps):
            med = float(np.median(per))
            return {"device_us_per_batch": round(med * 1e6, 1),
                    "device_us_min_max": [round(min(per) * 1e6, 1), round(max(per) * 1e6, 1)],
                    "host_wall_us_per_batch": round(float(np.median(wall)) * 1e6, 1),
                    "algorithmic_GBps": round(alg / med / 1e9, 1), "blocks": len(per), "batches_per_block": reps,
                    "seconds_timed": round(sum(per) * reps, 3)}

        A, B = arm(per_a, wall_a, ra), arm(per_b, wall_b, rb)
        res[name] = {"segments": nseg, "stripes_total": int(sum(stripes)), "stripes_min_max": [min(stripes), max(stripes)],
                     "sized": A, "other": B, "other_is": other_name,
                     "other_over_sized_device": round(B["device_us_per_batch"] / A["device_us_per_batch"], 3),
                     "other_over_sized_host_wall": round(B["host_wall_us_per_batch"] / A["host_wall_us_per_batch"], 3),
                     "sized_below_other_in_every_alternation": bool(all(a < b for a, b in zip(per_a, per_b))),
                     "other_spread": round(max(per_b) / min(per_b), 3),
                     "pieces_equal": equal}
        del seg_all, out_a, out_b
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    q, s = ctypes.c_ulonglong(), ctypes.c_ulonglong()
    L.ec_encoder_queue_stats(ctx, ctypes.byref(q), ctypes.byref(s))
    L.ec_destroy(ctx)
    print(json.dumps({"tool": "bench_encode_sized", "code": [K, N], "ess": ESS, "build": L.ec_build_id().decode(),
                      "encoder_launches": {"queued": q.value, "static_tiles": s.value},
                      "workloads": res, "pieces_equal": bool(all_equal)}))
    return 0 if all_equal else 1


if __name__ == "__main__":
    sys.exit(main())
