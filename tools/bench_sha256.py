#!/usr/bin/env python3
"""SHA-256 piece hashes on the GPU (ec_sha256_segments_sized) against what a
caller who needs SHA-256 did before: copy every piece to the host and hash it
there.  RS(29,80), ess 256, segments of 9,040 stripes, so that a
piece is 2,314,240 bytes (a 64 MiB segment's); batches of 1, 8, 32 and 128
segments, i.e. 80 .. 10,240 pieces, each piece one serial chain on one lane.

Per batch, in one process: the segments are encoded by one
ec_encode_segments_sized (all n pieces, so that the host arm finds every piece
as one row); the GPU arm is one ec_sha256_segments_sized call over the batch,
timed by HIP events on the stream (warmed once, then --reps calls, the median);
the host arm copies each segment's pieces into pinned host memory and hashes
its 80 rows with hashlib.sha256 on 16 threads.  The copy and the hashing are
timed apart and not overlapped: `host_hash_s` is the hashing alone (the D2H
copy is NOT in it), `d2h_s` the copies alone; a caller that pipelines them pays
the larger of the two at best.  Every digest of the GPU arm is compared with
the host arm's.  Reported: device seconds per call, GB/s, launches per call and
seconds per launch, nanoseconds per 64-byte block of one chain, and the ratios.

Every batch runs in a child process of its own under a time limit (--limit
seconds); the parent never opens the GPU and starts nothing after a step that
failed.  Writes the result as JSON (--out) and a log beside it, and prints one
JSON line.  Run on the GPU box:
    python tools/bench_sha256.py [--batches 1 8 32 128] [--out profiles/sha256/bench_sha256.json]"""
from __future__ import annotations

import argparse
import ctypes
import hashlib
import json
import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

K, N, ESS = 29, 80, 256
STRIPES = 9040                 # 9040 * 256 = 2,314,240 bytes per piece
PLEN = STRIPES * ESS
THREADS = 16


def worker(nseg, reps):
    import torch

    from uplink_amd import _native
    torch.cuda.set_device(0)
    torch.manual_seed(20261021 + nseg)
    L = _native.load()
    ctx = ctypes.c_void_p()
    assert L.ec_create(K, N, ESS, ctypes.byref(ctx)) == 0
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream()
    sptr = st.cuda_stream
    segs = [torch.randint(0, 256, (STRIPES * K * ESS,), dtype=torch.uint8, device=dev) for _ in range(nseg)]
    pieces = [torch.empty((N, PLEN), dtype=torch.uint8, device=dev) for _ in range(nseg)]
    c_in = (ctypes.c_void_p * nseg)(*[t.data_ptr() for t in segs])
    c_out = (ctypes.c_void_p * nseg)(*[t.data_ptr() for t in pieces])
    c_st = (ctypes.c_size_t * nseg)(*[STRIPES] * nseg)
    rc = L.ec_encode_segments_sized(ctx, nseg, c_in, c_st, None, c_out, 0, sptr)
    assert rc == 0, _native.strerror(rc)
    hashes = torch.zeros((nseg, N, 32), dtype=torch.uint8, device=dev)

    def stats():
        v = [ctypes.c_ulonglong() for _ in range(3)]
        L.ec_sha256_list_stats(ctx, *[ctypes.byref(x) for x in v])
        return [x.value for x in v]

    def go():
        rc = L.ec_sha256_segments_sized(ctx, nseg, c_in, c_st, c_out, 0, hashes.data_ptr(), sptr)
        assert rc == 0, _native.strerror(rc)

    go()  # warm: the staging block, the code object
    torch.cuda.synchronize()
    s0 = stats()
    per, wall = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        t0 = time.perf_counter()
        go()
        wall.append(time.perf_counter() - t0)  # the call returns before the GPU has run it
        e1.record(st)
        e1.synchronize()
        per.append(e0.elapsed_time(e1) * 1e-3)
    s1 = stats()
    launches = (s1[2] - s0[2]) // reps
    got = hashes.cpu().numpy()
    # the host arm: what the caller did before -- every piece to the host, hashlib on 16 threads
    pinned = torch.empty((N, PLEN), dtype=torch.uint8).pin_memory()
    rows = pinned.numpy()
    d2h_s = hash_s = 0.0
    equal = True
    with ThreadPoolExecutor(THREADS) as pool:
        for g in range(nseg):
            t0 = time.perf_counter()
            pinned.copy_(pieces[g], non_blocking=True)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            digs = list(pool.map(lambda r: hashlib.sha256(r).digest(), rows))  # (hashlib releases the GIL)
            t2 = time.perf_counter()
            d2h_s += t1 - t0
            hash_s += t2 - t1
            equal = equal and b"".join(digs) == got[g].tobytes()
    torch.cuda.synchronize()
    L.ec_destroy(ctx)
    hashed = float(nseg) * N * PLEN
    med = float(np.median(per))
    blocks = (PLEN + 8) // 64 + 1
    print(json.dumps({
        "segments": nseg, "pieces": nseg * N, "waves": -(-nseg * N // 64), "piece_bytes": PLEN,
        "hashed_bytes": int(hashed), "blocks_per_piece": blocks,
        "gpu_device_s_per_call": round(med, 6), "gpu_device_s_min_max": [round(min(per), 6), round(max(per), 6)],
        "gpu_host_wall_s_per_call": round(float(np.median(wall)), 6), "gpu_GBps": round(hashed / med / 1e9, 2),
        "launches_per_call": int(launches), "gpu_s_per_launch": round(med / max(launches, 1), 6),
        "ns_per_block_of_one_chain": round(med / blocks * 1e9, 1),
        "host_threads": THREADS, "host_hash_s": round(hash_s, 4), "host_hash_GBps": round(hashed / hash_s / 1e9, 2),
        "d2h_s": round(d2h_s, 4), "d2h_GBps": round(hashed / d2h_s / 1e9, 2), "d2h_in_host_hash_s": False,
        "host_hash_over_gpu": round(hash_s / med, 3), "host_hash_plus_d2h_over_gpu": round((hash_s + d2h_s) / med, 3),
        "digests_checked": nseg * N, "digests_equal": bool(equal), "pieces_fast_bytewise": [s1[0] - s0[0], s1[1] - s0[1]],
        "reps": reps, "build": L.ec_build_id().decode()}))
    return 0 if equal else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", nargs="*", type=int, default=[1, 8, 32, 128], help="segments per batch")
    ap.add_argument("--reps", type=int, default=3, help="timed GPU calls per batch")
    ap.add_argument("--limit", type=float, default=240.0, help="time limit of one batch's child process, seconds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sha256", "bench_sha256.json"))
    ap.add_argument("--worker", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker is not None:
        return worker(args.worker, args.reps)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    log = open(os.path.splitext(args.out)[0] + ".log", "w")
    res, ok = {}, True
    for nseg in args.batches:
        cmd = ["timeout", "-k", "10", str(int(args.limit)), sys.executable, os.path.abspath(__file__), "--worker",
               str(nseg), "--reps", str(args.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        log.write(f"## {nseg} segments: exit {r.returncode}\n{r.stdout}{r.stderr}\n")
        log.flush()
        if r.returncode != 0:  # nothing more on the GPU after a step that failed or ran out of time
            sys.stderr.write(r.stdout + r.stderr)
            res[str(nseg)] = {"failed": r.returncode}
            ok = False
            break
        res[str(nseg)] = json.loads(r.stdout.strip().splitlines()[-1])
        ok = ok and res[str(nseg)]["digests_equal"]
    done = [v for v in res.values() if "failed" not in v]
    ahead = [v["segments"] for v in done if v["host_hash_over_gpu"] > 1.0]
    out = {"tool": "bench_sha256", "code": [K, N], "ess": ESS, "stripes": STRIPES, "piece_bytes": PLEN,
           "batches": res, "digests_equal": ok,
           "smallest_batch_where_gpu_beats_host_hashing_alone": min(ahead) if ahead else None}
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    log.close()
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
