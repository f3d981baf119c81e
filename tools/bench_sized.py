#!/usr/bin/env python3
"""Share-set Rebuild of segments of different sizes in one call
(ec_rebuild_segments_sized) against the forms available without it
(DESIGN.md §4h).  RS(29,80), ess 256, a fresh seeded 29-subset per segment.

  small   256 segments, stripe counts seeded log-uniform in 8..560 (64 KiB - 4 MiB),
          against one ec_rebuild_segments_sets call per segment on the same
          stream with no host waits between
  mixed   the 24 smallest of those, smallest first, plus 8 of 9040 stripes,
          against the same per-segment calls
  equal   32 x 9040 stripes, against one ec_rebuild_segments_sets call

The arms alternate in this process on the same inputs, each block timed by HIP
events on the stream, until each has at least --seconds of device time; every
shape is warmed first and every arm's outputs must equal the other's and the
segments the pieces were encoded from.  Reported per workload and arm: device
us per batch (median, min-max over the blocks), host wall us per batch (the
time the calls take to return), algorithmic GB/s (sum of 2 * nstripes * k * ess
over the device time) and the ratios.  Prints one JSON line.  Run on the GPU box:
    python tools/bench_sized.py [--seconds S] [--workloads small mixed equal]"""
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
    small = sorted(int(round(x)) for x in np.exp(rng.uniform(np.log(8), np.log(560), 256)))
    small_order = [small[i] for i in rng.permutation(256)]
    shapes = {"small": small_order, "mixed": small[:24] + [BIG] * 8, "equal": [BIG] * 32}

    def make(stripes):
        """per segment: the segment, the k chosen pieces' numbers and tensors (only those are kept)"""
        out = []
        for s in stripes:
            seg = torch.randint(0, 256, (s * K * ESS,), dtype=torch.uint8, device=dev)
            pcs = torch.empty((N, s * ESS), dtype=torch.uint8, device=dev)
            assert L.ec_encode_segments(ctx, seg.data_ptr(), 1, s, pcs.data_ptr(), 0, sptr) == 0
            nums = [int(x) for x in rng.permutation(N)[:K]]
            keep = pcs[nums].clone()
            out.append((seg, nums, keep))
            torch.cuda.synchronize()
            del pcs
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

    res, all_equal = {}, True
    for name in args.workloads:
        stripes = shapes[name]
        nseg = len(stripes)
        data = make(stripes)
        outs_a = [torch.zeros(s * K * ESS, dtype=torch.uint8, device=dev) for s in stripes]
        outs_b = [torch.full((s * K * ESS,), 0xFF, dtype=torch.uint8, device=dev) for s in stripes]
        flat = [x for _, nums, _ in data for x in nums]
        ptrs = [keep[i].data_ptr() for _, _, keep in data for i in range(K)]
        a_ns = (ctypes.c_int * nseg)(*[K] * nseg)
        a_nums = (ctypes.c_int * len(flat))(*flat)
        a_ptrs = (ctypes.c_void_p * len(ptrs))(*ptrs)
        a_st = (ctypes.c_size_t * nseg)(*stripes)
        a_outs = (ctypes.c_void_p * nseg)(*[o.data_ptr() for o in outs_a])
        b_outs = (ctypes.c_void_p * nseg)(*[o.data_ptr() for o in outs_b])
        one = (ctypes.c_int * 1)(K)
        per_seg = [((ctypes.c_int * K)(*flat[g * K:(g + 1) * K]), (ctypes.c_void_p * K)(*ptrs[g * K:(g + 1) * K]),
                    stripes[g], (ctypes.c_void_p * 1)(outs_b[g].data_ptr())) for g in range(nseg)]

        def go_sized():
            rc = L.ec_rebuild_segments_sized(ctx, nseg, a_ns, a_nums, a_ptrs, a_st, a_outs, sptr)
            assert rc == 0, _native.strerror(rc)

        def go_per_segment():
            for nums, pp, s, o in per_seg:
                rc = L.ec_rebuild_segments_sets(ctx, 1, one, nums, pp, s, o, sptr)
                assert rc == 0, _native.strerror(rc)

        def go_one_sets_call():
            rc = L.ec_rebuild_segments_sets(ctx, nseg, a_ns, a_nums, a_ptrs, BIG, b_outs, sptr)
            assert rc == 0, _native.strerror(rc)

        other, other_name = (go_one_sets_call, "one ec_rebuild_segments_sets call") if name == "equal" else \
            (go_per_segment, "one ec_rebuild_segments_sets call per segment")
        for _ in range(3):
            go_sized()
            other()
        torch.cuda.synchronize()
        equal = all(torch.equal(a, b) and torch.equal(a, seg) for a, b, (seg, _, _) in zip(outs_a, outs_b, data))
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
        alg = 2.0 * sum(stripes) * K * ESS

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
                     "sized_host_wall_us_per_segment": round(A["host_wall_us_per_batch"] / nseg, 2),
                     "outputs_equal": bool(equal)}
        del data, outs_a, outs_b
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    L.ec_destroy(ctx)
    print(json.dumps({"tool": "bench_sized", "code": [K, N], "ess": ESS, "build": L.ec_build_id().decode(),
                      "workloads": res, "outputs_equal": bool(all_equal)}))
    return 0 if all_equal else 1


if __name__ == "__main__":
    sys.exit(main())
