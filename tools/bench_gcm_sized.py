#!/usr/bin/env python3
"""Developer measurement of AES-256-GCM with a size per segment
(ec_gcm_seal_segments_sized), inputs resident in HBM, one process,
device events around `--iters` calls, the variants of a case alternated over
`--repeats` rounds so that drift hits both alike:

  a  8 x 9059 blocks of 7408 B: the uniform call against the sized call
  b  64 segments, sizes log-uniform from 4 KiB to 64 MiB (seeded): the sized
     call against one ec_gcm_seal_segments_strided call per segment
  c  1024 one-block segments: the small-object case, the sized call alone

Prints one JSON line: per case and variant the device and wall microseconds of
every round, their median and their spread (max - min) / median."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from uplink_amd import _native  # noqa: E402
from uplink_amd import encryption as E  # noqa: E402
from uplink_amd.uploads import cipher_geometry  # noqa: E402

IB = 7408
WINDOW_S = 0.25  # (--window-s)


class Ctx:
    def __init__(self):
        self.ctx = ctypes.c_void_p()
        assert _native.load().ec_create(29, 80, 256, ctypes.byref(self.ctx)) == 0


def measure(variants, iters, repeats, st):
    """variants: {name: callable queuing one call on st} -> {name: {...}}"""
    res = {k: {"device_us": [], "wall_us": []} for k in variants}
    slowest = 0.0
    for f in variants.values():  # warm: staging pools, code objects, clocks
        t_end = time.time() + 0.2
        while time.time() < t_end:
            f()
        st.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            f()
        st.synchronize()
        slowest = max(slowest, (time.perf_counter() - t0) / 3)
    iters = max(iters, int(WINDOW_S / slowest) + 1)  # a timed window of at least WINDOW_S per variant
    for r in res.values():
        r["iters"] = iters
    for _ in range(repeats):
        for name, f in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            st.synchronize()
            t0 = time.perf_counter()
            e0.record(st)
            for _ in range(iters):
                f()
            e1.record(st)
            e1.synchronize()
            t1 = time.perf_counter()
            res[name]["device_us"].append(e0.elapsed_time(e1) * 1e3 / iters)
            res[name]["wall_us"].append((t1 - t0) * 1e6 / iters)
    for r in res.values():
        for k in ("device_us", "wall_us"):
            v = r[k]
            r[k + "_median"] = statistics.median(v)
            r[k + "_spread"] = (max(v) - min(v)) / statistics.median(v)
    return res


def batch(nblocks, seed):
    """per-segment plaintext and ciphertext tensors, prepared keys, nonces"""
    rng = np.random.default_rng(seed)
    n = len(nblocks)
    keys = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(n)]
    d_keys = E.prepare_keys(keys)
    d_nonces = torch.from_numpy(rng.integers(0, 256, 12 * n, dtype=np.uint8)).cuda()
    g = torch.Generator(device="cuda").manual_seed(seed)
    plains = [torch.randint(0, 256, (nb * IB,), dtype=torch.uint8, device="cuda", generator=g) for nb in nblocks]
    outs = [torch.empty(nb * (IB + 16), dtype=torch.uint8, device="cuda") for nb in nblocks]
    return d_keys, d_nonces, plains, outs


def main():
    global WINDOW_S
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--cases", default="abc")
    ap.add_argument("--out", default=None, help="also write the JSON to this file")
    ap.add_argument("--window-s", type=float, default=WINDOW_S, help="least work per timed window")
    args = ap.parse_args()
    WINDOW_S = args.window_s
    torch.cuda.set_device(0)
    L = _native.load()
    c = Ctx()
    st = torch.cuda.Stream()
    kb = L.ec_gcm_key_bytes()
    out = {"build": L.ec_build_id().decode(), "iters": args.iters, "repeats": args.repeats}

    if "a" in args.cases:
        nseg, nb = 8, 9059
        rng = np.random.default_rng(3)
        d_keys = E.prepare_keys([rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(nseg)])
        d_nonces = torch.from_numpy(rng.integers(0, 256, 12 * nseg, dtype=np.uint8)).cuda()
        g = torch.Generator(device="cuda").manual_seed(2)
        plain = torch.randint(0, 256, (nseg, nb * IB), dtype=torch.uint8, device="cuda", generator=g)
        ct = torch.empty((nseg, nb * (IB + 16)), dtype=torch.uint8, device="cuda")
        ct2 = torch.empty_like(ct)
        rows, rows2 = [plain[i] for i in range(nseg)], [ct2[i] for i in range(nseg)]
        res = measure({
            "uniform": lambda: E.seal_segments(plain, nseg, nb, IB, d_keys, d_nonces, ct, stream=st),
            "sized": lambda: E.seal_segments_sized(c, rows, [nb] * nseg, IB, d_keys, d_nonces, rows2, stream=st),
        }, args.iters, args.repeats, st)
        torch.cuda.synchronize()
        assert torch.equal(ct, ct2)
        res["workload"] = f"{nseg} x {nb} blocks of {IB} B"
        res["sized_over_uniform_device"] = res["sized"]["device_us_median"] / res["uniform"]["device_us_median"]
        out["a"] = res
        del plain, ct, ct2, rows, rows2

    if "b" in args.cases:
        rng = np.random.default_rng(20261021)
        sizes = [int(x) for x in np.exp(rng.uniform(np.log(4096), np.log(64 << 20), 64))]
        nblocks = [cipher_geometry(s)[0] for s in sizes]
        d_keys, d_nonces, plains, outs = batch(nblocks, 4)
        outs2 = [torch.empty_like(o) for o in outs]
        s_raw = st.cuda_stream

        def per_segment():
            for g, nb in enumerate(nblocks):
                rc = L.ec_gcm_seal_segments_strided(plains[g].data_ptr(), 0, 1, nb, IB, d_keys.data_ptr() + g * kb,
                                                    d_nonces.data_ptr() + 12 * g, outs2[g].data_ptr(), 0, s_raw)
                assert rc == 0

        res = measure({
            "sized": lambda: E.seal_segments_sized(c, plains, nblocks, IB, d_keys, d_nonces, outs, stream=st),
            "per_segment": per_segment,
        }, max(args.iters // 2, 1), args.repeats, st)
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(outs, outs2))
        res["workload"] = (f"64 segments, sizes log-uniform 4 KiB .. 64 MiB (seed 20261021): {sum(nblocks)} blocks, "
                           f"{sum(nblocks) * IB / 1e6:.1f} MB of plaintext, largest {max(nblocks)} blocks")
        res["per_segment_over_sized_device"] = res["per_segment"]["device_us_median"] / res["sized"]["device_us_median"]
        res["per_segment_over_sized_wall"] = res["per_segment"]["wall_us_median"] / res["sized"]["wall_us_median"]
        out["b"] = res
        del plains, outs, outs2

    if "c" in args.cases:
        nblocks = [1] * 1024
        d_keys, d_nonces, plains, outs = batch(nblocks, 5)
        res = measure({
            "sized": lambda: E.seal_segments_sized(c, plains, nblocks, IB, d_keys, d_nonces, outs, stream=st),
        }, args.iters, args.repeats, st)
        res["workload"] = f"1024 segments of one block of {IB} B"
        res["GBps_plaintext"] = 1024 * IB / res["sized"]["device_us_median"] / 1e3
        res["segments_per_s"] = 1024 / res["sized"]["device_us_median"] * 1e6
        out["c"] = res

    v = [ctypes.c_ulonglong() for _ in range(3)]
    L.ec_gcm_sized_stats(c.ctx, *[ctypes.byref(x) for x in v])
    out["sized_stats"] = [x.value for x in v]
    torch.cuda.synchronize()
    L.ec_destroy(c.ctx)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
