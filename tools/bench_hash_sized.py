#!/usr/bin/env python3
"""Piece hashes of uploads of different sizes in one call (ec_hash_segments_sized)
against what the library offered before it: ec_hash_segments once per segment
(DESIGN.md §4j, §5).  RS(29,80), ess 256, two seeded batches:

  large   64 uploads, sizes log-uniform between 1 KiB and 64 MiB
  small   256 uploads, sizes log-uniform between 4 KiB and 64 KiB

Each upload is padded as PadReader pads it (uploads.upload_geometry) and encoded
parity only; both arms then hash all n pieces of every upload from the same
buffers (data pieces in place from the stripe-major segment, parity pieces from
the encoder's output), on one stream with no host waits between the calls.  The
arms alternate in one process on the same inputs, each block timed by HIP events
on the stream, until each has at least --seconds of device time; every shape is
warmed first and the two arms' hashes must be equal.  Reported per batch and arm:
device us per batch (median, min-max over the blocks), host wall us per batch,
GB/s hashed (n pieces of nstripes * ess bytes per upload over the device time;
the uniform segment form measures 2.7 TB/s), and the ratio.

Every batch runs in a child process of its own under a time limit (--limit
seconds); the parent never opens the GPU.  Prints one JSON line.  Run on the GPU box:
    python tools/bench_hash_sized.py [--seconds S] [--batches large small]"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

K, N, ESS = 29, 80, 256
STRIPE = K * ESS
BATCHES = {"large": (64, 1 << 10, 64 << 20, 2990), "small": (256, 4 << 10, 64 << 10, 2991)}


def stripes_of(size):
    """uploads.upload_geometry's stripe count (PadReader: at least 4 bytes of padding)"""
    return (size + 4 + (STRIPE - (size + 4) % STRIPE) % STRIPE) // STRIPE


def draw(name):
    count, lo, hi, seed = BATCHES[name]
    rng = np.random.default_rng(seed)
    sizes = [int(round(x)) for x in np.exp(rng.uniform(np.log(lo), np.log(hi), count))]
    return sizes, [stripes_of(s) for s in sizes]


def worker(name, seconds, rounds):
    import torch

    from uplink_amd import _native
    torch.cuda.set_device(0)
    L = _native.load()
    ctx = ctypes.c_void_p()
    assert L.ec_create(K, N, ESS, ctypes.byref(ctx)) == 0
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream()
    sptr = st.cuda_stream
    sizes, stripes = draw(name)
    nseg = len(stripes)
    total = sum(stripes)
    seg_all = torch.randint(0, 256, (total * STRIPE,), dtype=torch.uint8, device=dev)
    par_all = torch.empty(total * (N - K) * ESS, dtype=torch.uint8, device=dev)
    starts = [int(x) for x in np.concatenate([[0], np.cumsum(stripes)])[:-1]]
    in_ptrs = [seg_all.data_ptr() + s0 * STRIPE for s0 in starts]
    par_ptrs = [par_all.data_ptr() + s0 * (N - K) * ESS for s0 in starts]
    c_in = (ctypes.c_void_p * nseg)(*in_ptrs)
    c_par = (ctypes.c_void_p * nseg)(*par_ptrs)
    c_st = (ctypes.c_size_t * nseg)(*stripes)
    rc = L.ec_encode_segments_sized(ctx, nseg, c_in, c_st, None, c_par, _native.EC_FLAG_PARITY_ONLY, sptr)
    assert rc == 0, _native.strerror(rc)
    h_a = torch.zeros((nseg, N, 32), dtype=torch.uint8, device=dev)
    h_b = torch.full((nseg, N, 32), 0xFF, dtype=torch.uint8, device=dev)
    hb_ptrs = [h_b[g].data_ptr() for g in range(nseg)]

    def go_sized():
        rc = L.ec_hash_segments_sized(ctx, nseg, c_in, c_st, c_par, _native.EC_FLAG_PARITY_ONLY, h_a.data_ptr(), sptr)
        assert rc == 0, _native.strerror(rc)

    def go_per_segment():
        for g in range(nseg):
            rc = L.ec_hash_segments(ctx, in_ptrs[g], par_ptrs[g], 1, stripes[g], hb_ptrs[g], sptr)
            assert rc == 0, _native.strerror(rc)

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

    for _ in range(3):
        go_sized()
        go_per_segment()
    torch.cuda.synchronize()
    equal = bool(torch.equal(h_a, h_b))
    ta, tb = timed(go_sized, 3)[0], timed(go_per_segment, 3)[0]
    ra = max(3, int(np.ceil(seconds / rounds / ta)))
    rb = max(3, int(np.ceil(seconds / rounds / tb)))
    per_a, per_b, wall_a, wall_b = [], [], [], []
    while len(per_a) < rounds or min(sum(per_a) * ra, sum(per_b) * rb) < seconds:
        t, w = timed(go_sized, ra)
        per_a.append(t), wall_a.append(w)
        t, w = timed(go_per_segment, rb)
        per_b.append(t), wall_b.append(w)
    hashed = float(total) * N * ESS

    def arm(per, wall, reps):
        med = float(np.median(per))
        return {"device_us_per_batch": round(med * 1e6, 1),
                "device_us_min_max": [round(min(per) * 1e6, 1), round(max(per) * 1e6, 1)],
                "host_wall_us_per_batch": round(float(np.median(wall)) * 1e6, 1),
                "hashed_GBps": round(hashed / med / 1e9, 1), "blocks": len(per), "batches_per_block": reps,
                "seconds_timed": round(sum(per) * reps, 3)}

    A, B = arm(per_a, wall_a, ra), arm(per_b, wall_b, rb)
    v = [ctypes.c_ulonglong() for _ in range(4)]
    L.ec_hash_list_stats(ctx, *[ctypes.byref(x) for x in v])
    torch.cuda.synchronize()
    L.ec_destroy(ctx)
    print(json.dumps({"uploads": nseg, "bytes_min_max": [min(sizes), max(sizes)], "stripes_total": total,
                      "hashed_bytes": int(hashed), "sized_one_call": A, "per_segment_calls": B,
                      "per_segment_over_sized_device": round(B["device_us_per_batch"] / A["device_us_per_batch"], 3),
                      "per_segment_over_sized_host_wall": round(B["host_wall_us_per_batch"] / A["host_wall_us_per_batch"], 3),
                      "sized_below_per_segment_in_every_alternation": bool(all(a < b for a, b in zip(per_a, per_b))),
                      "list_launches_fast_byte_parents_oversize": [x.value for x in v],
                      "hashes_equal": equal, "build": L.ec_build_id().decode()}))
    return 0 if equal else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0, help="device time per arm and batch, at least")
    ap.add_argument("--rounds", type=int, default=5, help="alternations of the two arms per batch, at least")
    ap.add_argument("--batches", nargs="*", default=["large", "small"])
    ap.add_argument("--limit", type=float, default=240.0, help="time limit of one batch's child process, seconds")
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker, args.seconds, args.rounds)
    res, ok = {}, True
    for name in args.batches:
        cmd = ["timeout", "-k", "10", str(int(args.limit)), sys.executable, os.path.abspath(__file__), "--worker", name,
               "--seconds", str(args.seconds), "--rounds", str(args.rounds)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:  # nothing more on the GPU after a step that failed or ran out of time
            sys.stderr.write(r.stdout + r.stderr)
            res[name] = {"failed": r.returncode}
            ok = False
            break
        res[name] = json.loads(r.stdout.strip().splitlines()[-1])
        ok = ok and res[name]["hashes_equal"]
    print(json.dumps({"tool": "bench_hash_sized", "code": [K, N], "ess": ESS, "batches": res, "hashes_equal": ok}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
