#!/usr/bin/env python3
"""Developer measurement of the one-shot message cipher (ec_gcm_seal_messages,
DESIGN.md §4n), inputs resident in HBM, one process, device events and the wall
clock around every timed window, the variants of a case alternated over
`--repeats` rounds so that drift hits all alike:

  a  16384 messages of 4096 bytes, a key each, through ec_gcm_seal_messages,
     alternated with the only way the block cipher can do it: ec_gcm_prepare_keys
     of the 16384 keys (a 20 KB table each, built on the host and copied in
     synchronously) plus ec_gcm_seal_segments_sized with nblocks = 1 and
     in_block = 4096.  The key preparation is inside the timed window: a key per
     message is the workload.  With --parent-lib PATH that way is also run from
     that other build of the library (the parent commit's), twice, so that its
     own run-to-run spread stands beside the comparison.  The two ways seal the
     same bytes (compared).
  b  65536 EncryptKey messages of 32 bytes.
  c  16384 messages of seeded random length 0..4096 at odd addresses.

Each case also runs a single-thread OpenSSL loop over the same lists through
oracle.aesgcm.seal (one Python call per message: labelled cpu_openssl_1thread, a
host figure for scale, not a competitor on equal terms).

The timed quantity is wall_us: from the first call of a window to the stream's
completion, host time and device time together, per call.  device_us is the
device events' share of it.  Prints one JSON line: per case and variant the
microseconds of every round, their median and their spread (max - min) / median.
The condition on case a is evaluated and printed (`a.verdict`)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import torch  # noqa: E402

from uplink_amd import _native  # noqa: E402
from uplink_amd import encryption as E  # noqa: E402

TAG = 16


class Ctx:
    def __init__(self, L):
        self.L = L
        self.ctx = ctypes.c_void_p()
        assert L.ec_create(29, 80, 256, ctypes.byref(self.ctx)) == 0


def other_lib(path):
    """another build of the library beside the process's own, with the parent's exports bound"""
    L = ctypes.CDLL(path)
    for name in ("ec_create", "ec_destroy", "ec_gcm_key_bytes", "ec_gcm_prepare_keys", "ec_gcm_seal_segments_sized",
                 "ec_build_id"):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = _native.SIGNATURES[name]
    return L


def measure(variants, repeats, st, window_s):
    """variants: {name: callable queuing one call on st}.  Every variant gets its own number of
    calls per window: at least one, and enough to fill window_s."""
    res = {k: {"device_us": [], "wall_us": []} for k in variants}
    iters = {}
    for name, f in variants.items():  # warm: staging pools, code objects, clocks
        f()
        st.synchronize()
        t0 = time.perf_counter()
        f()
        st.synchronize()
        one = time.perf_counter() - t0
        iters[name] = max(1, int(window_s / one))
        res[name]["iters"] = iters[name]
    for _ in range(repeats):
        for name, f in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            st.synchronize()
            t0 = time.perf_counter()
            e0.record(st)
            for _ in range(iters[name]):
                f()
            e1.record(st)
            e1.synchronize()
            t1 = time.perf_counter()
            res[name]["device_us"].append(e0.elapsed_time(e1) * 1e3 / iters[name])
            res[name]["wall_us"].append((t1 - t0) * 1e6 / iters[name])
    for r in res.values():
        for k in ("device_us", "wall_us"):
            v = r[k]
            r[k + "_median"] = statistics.median(v)
            r[k + "_spread"] = (max(v) - min(v)) / statistics.median(v)
    return res


class Batch:
    """n messages: keys and nonces (host and device), plaintexts and outputs as windows of two
    device buffers, every window `shift` bytes past a 16-byte boundary"""

    def __init__(self, lens, seed, shift=0):
        rng = np.random.default_rng(seed)
        self.lens = [int(x) for x in lens]
        n = len(self.lens)
        self.h_keys = rng.integers(0, 256, 32 * n, dtype=np.uint8)
        self.h_nonces = rng.integers(0, 256, 12 * n, dtype=np.uint8)
        self.d_keys = torch.from_numpy(self.h_keys).cuda()
        self.d_nonces = torch.from_numpy(self.h_nonces).cuda()
        slot = lambda x: (x + shift + 15) // 16 * 16 + 16  # noqa: E731
        self.in_off = np.concatenate([[0], np.cumsum([slot(x) for x in self.lens])]).astype(np.int64)
        self.out_off = np.concatenate([[0], np.cumsum([slot(x + TAG) for x in self.lens])]).astype(np.int64)
        g = torch.Generator(device="cuda").manual_seed(seed)
        self.plain = torch.randint(0, 256, (int(self.in_off[-1]) + 16,), dtype=torch.uint8, device="cuda", generator=g)
        self.out = torch.zeros(int(self.out_off[-1]) + 16, dtype=torch.uint8, device="cuda")
        assert self.plain.data_ptr() % 16 == 0 and self.out.data_ptr() % 16 == 0
        self.shift = shift
        self.c_in = (ctypes.c_void_p * n)(*[self.plain.data_ptr() + int(o) + shift for o in self.in_off[:-1]])
        self.c_out = (ctypes.c_void_p * n)(*[self.out.data_ptr() + int(o) + shift for o in self.out_off[:-1]])
        self.c_len = (ctypes.c_size_t * n)(*self.lens)

    def seal(self, c, st):
        rc = c.L.ec_gcm_seal_messages(c.ctx, len(self.lens), self.c_in, self.c_len, self.d_keys.data_ptr(),
                                      self.d_nonces.data_ptr(), self.c_out, st.cuda_stream)
        assert rc == 0, rc

    def message(self, buf, off, i, extra):
        at = int(off[i]) + self.shift
        return buf[at:at + self.lens[i] + extra]

    def check(self, ag, count=64):
        """`count` messages, spread over the list, against the oracle"""
        out, plain = self.out.cpu().numpy(), self.plain.cpu().numpy()
        n = len(self.lens)
        for i in sorted({int(x) for x in np.linspace(0, n - 1, min(count, n))}):
            want = bytes(ag.seal(self.h_keys[32 * i:32 * i + 32].tobytes(), self.h_nonces[12 * i:12 * i + 12].tobytes(),
                                 self.message(plain, self.in_off, i, 0).tobytes()))
            assert self.message(out, self.out_off, i, TAG).tobytes() == want, i

    def openssl_loop(self, ag):
        """single thread, one oracle call per message -> microseconds for the whole list"""
        plain = self.plain.cpu().numpy()
        msgs = [(self.h_keys[32 * i:32 * i + 32].tobytes(), self.h_nonces[12 * i:12 * i + 12].tobytes(),
                 self.message(plain, self.in_off, i, 0).tobytes()) for i in range(len(self.lens))]
        t0 = time.perf_counter()
        for k, n, p in msgs:
            ag.seal(k, n, p)
        return (time.perf_counter() - t0) * 1e6


class BlockWay:
    """the parent's way for equal messages of `size` bytes (a multiple of 16), through library L:
    prepare the n keys, then the sized seal with one block per segment"""

    def __init__(self, L, b, size):
        self.c = Ctx(L)
        n = len(b.lens)
        self.n, self.size, self.b = n, size, b
        self.d_sched = torch.empty(n * L.ec_gcm_key_bytes(), dtype=torch.uint8, device="cuda")
        self.out = torch.zeros(n * (size + TAG), dtype=torch.uint8, device="cuda")
        self.c_out = (ctypes.c_void_p * n)(*[self.out.data_ptr() + i * (size + TAG) for i in range(n)])
        self.c_nb = (ctypes.c_size_t * n)(*[1] * n)

    def __call__(self, st):
        L, b = self.c.L, self.b
        rc = L.ec_gcm_prepare_keys(b.h_keys.ctypes.data, self.n, self.d_sched.data_ptr(), st.cuda_stream)
        assert rc == 0, rc
        rc = L.ec_gcm_seal_segments_sized(self.c.ctx, self.n, b.c_in, self.c_nb, None, self.size,
                                          self.d_sched.data_ptr(), b.d_nonces.data_ptr(), self.c_out, st.cuda_stream)
        assert rc == 0, rc

    def check(self):
        """the same sealed bytes as the message call's"""
        want = torch.stack([self.b.message(self.b.out, self.b.out_off, i, TAG) for i in range(0, self.n, 257)])
        got = torch.stack([self.out[i * (self.size + TAG):(i + 1) * (self.size + TAG)] for i in range(0, self.n, 257)])
        assert torch.equal(want, got)


def case_a(c, st, args, ag):
    n, size = args.messages, 4096
    b = Batch([size] * n, 11)
    variants = {"messages": lambda: b.seal(c, st)}
    own = BlockWay(c.L, b, size)
    variants["prepare_keys_plus_sized"] = lambda: own(st)
    parent = None
    if args.parent_lib:
        parent = BlockWay(other_lib(args.parent_lib), b, size)
        variants["parent_prepare_keys_plus_sized"] = lambda: parent(st)
        variants["parent_prepare_keys_plus_sized_again"] = lambda: parent(st)
    res = measure(variants, args.repeats, st, args.window_s)
    torch.cuda.synchronize()
    b.check(ag)
    own.check()
    if parent:
        parent.check()
        res["parent_build"] = parent.c.L.ec_build_id().decode()
    res["workload"] = f"{n} messages of {size} B, a key each"
    new, old = res["messages"], res["parent_prepare_keys_plus_sized" if parent else "prepare_keys_plus_sized"]
    res["GBps_plaintext_wall"] = {k: n * size / res[k]["wall_us_median"] / 1e3 for k in variants}
    res["GBps_plaintext_device_messages"] = n * size / new["device_us_median"] / 1e3
    gap = (old["wall_us_median"] - new["wall_us_median"]) / old["wall_us_median"]
    res["verdict"] = {"compared_with": "parent library" if parent else "this library's block calls",
                      "messages_wall_us_median": new["wall_us_median"], "block_way_wall_us_median": old["wall_us_median"],
                      "relative_gap": gap, "spreads": [new["wall_us_spread"], old["wall_us_spread"]],
                      "messages_faster_by_more_than_the_spreads": gap > new["wall_us_spread"] + old["wall_us_spread"]}
    if parent:
        again = res["parent_prepare_keys_plus_sized_again"]
        res["parent_again_over_parent_wall"] = again["wall_us_median"] / old["wall_us_median"]
    res["cpu_openssl_1thread_us"] = b.openssl_loop(ag)
    return res


def case_list(c, st, args, ag, lens, seed, shift, workload):
    b = Batch(lens, seed, shift)
    res = measure({"messages": lambda: b.seal(c, st)}, args.repeats, st, args.window_s)
    torch.cuda.synchronize()
    b.check(ag)
    res["workload"] = workload
    total = sum(b.lens)
    res["messages_per_second_wall"] = len(b.lens) / res["messages"]["wall_us_median"] * 1e6
    res["GBps_plaintext_wall"] = total / res["messages"]["wall_us_median"] / 1e3
    res["cpu_openssl_1thread_us"] = b.openssl_loop(ag)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--cases", default="abc")
    ap.add_argument("--messages", type=int, default=16384, help="cases a and c: messages")
    ap.add_argument("--keys", type=int, default=65536, help="case b: EncryptKey messages")
    ap.add_argument("--parent-lib", default=None, help="case a: another build of libuplink_ec.so to run the block way from")
    ap.add_argument("--lib", default=None, help="the library to measure instead of the tree's (an A/B build)")
    ap.add_argument("--out", default=None, help="also write the JSON to this file")
    ap.add_argument("--window-s", type=float, default=0.25, help="least work per timed window")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    L = _native.load(args.lib) if args.lib else _native.load()
    from oracle import aesgcm as ag
    c = Ctx(L)
    st = torch.cuda.Stream()
    out = {"build": L.ec_build_id().decode(), "lib": args.lib or "tree", "repeats": args.repeats}
    if "a" in args.cases:
        out["a"] = case_a(c, st, args, ag)
        torch.cuda.empty_cache()
    if "b" in args.cases:
        out["b"] = case_list(c, st, args, ag, [32] * args.keys, 12, 0, f"{args.keys} EncryptKey messages of 32 B")
    if "c" in args.cases:
        lens = np.random.default_rng(13).integers(0, 4097, args.messages)
        out["c"] = case_list(c, st, args, ag, lens, 13, 5,
                             f"{args.messages} messages of seeded random length 0..4096, windows 5 bytes past 16")
    v = [ctypes.c_ulonglong() for _ in range(4)]
    L.ec_gcm_messages_stats(c.ctx, *[ctypes.byref(x) for x in v])
    out["messages_stats"] = [x.value for x in v]
    torch.cuda.synchronize()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    t0 = time.time()
    main()
    print(f"# {time.time() - t0:.1f} s", file=sys.stderr)
