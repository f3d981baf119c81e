#!/usr/bin/env python3
"""Developer measurement of ranged downloads (ec_gcm_open_ranges_sized,
uplink_amd/downloads.py download_ranges), inputs resident in HBM,
one process, device events around `--iters` calls, the variants of a case
alternated over `--repeats` rounds so that drift hits all alike
(tools/bench_gcm_sized.py measure):

  a  64 segments of 9060 blocks of 7408 B, valid ciphertext: the aligned ranged
     open over whole block runs (head 0, length nb*ib) against
     ec_gcm_open_segments_sized on the same bytes, the ranged open of the same
     blocks with head 6608 (a multiple of 16: still the aligned path) and with
     head 6609 (the bytewise path).  With --parent-lib PATH the sized open
     of that other build of the library (the parent commit's) is alternated with
     them in the same process, twice, so that its own run-to-run spread and the
     difference between two runs of the same code stand beside the comparison.
  w  256 ranges of 1 MiB at random offsets of 64 MiB segments under RS(29,80)
     through download_ranges (piece ranges in, plaintext out), beside
     --whole-count whole 64 MiB segments through decode_downloads +
     open_downloads, whose time is SCALED to 256 downloads.

Prints one JSON line: per case and variant the device and wall microseconds of
every round, their median and their spread (max - min) / median."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import torch  # noqa: E402

import bench_gcm_sized as B  # noqa: E402
from uplink_amd import _native, downloads, eestream  # noqa: E402
from uplink_amd import encryption as E  # noqa: E402
from uplink_amd.uploads import cipher_geometry  # noqa: E402

IB = 7408
BLOCK = IB + 16
SEGMENT = 64 << 20


class Lib:
    """another build of the library beside the process's own: its context and its sized open"""

    def __init__(self, path):
        self.L = ctypes.CDLL(path)
        for name in ("ec_create", "ec_destroy", "ec_gcm_open_segments_sized", "ec_build_id"):
            fn = getattr(self.L, name)
            fn.restype, fn.argtypes = _native.SIGNATURES[name]
        self.ctx = ctypes.c_void_p()
        assert self.L.ec_create(29, 80, 256, ctypes.byref(self.ctx)) == 0

    def open_sized(self, ciphers, nblocks, d_keys, d_nonces, outs, status, st):
        n = len(nblocks)
        rc = self.L.ec_gcm_open_segments_sized(
            self.ctx, n, (ctypes.c_void_p * n)(*[x.data_ptr() for x in ciphers]), (ctypes.c_size_t * n)(*nblocks), IB,
            d_keys.data_ptr(), d_nonces.data_ptr(), (ctypes.c_void_p * n)(*[x.data_ptr() for x in outs]),
            status.data_ptr(), st.cuda_stream)
        assert rc == 0, rc


def add_to_nonce(nonce: bytes, amount: int) -> bytes:
    """encryption.Increment: little-endian add, wrapping at the top"""
    return ((int.from_bytes(nonce, "little") + amount) % (1 << (8 * len(nonce)))).to_bytes(len(nonce), "little")


def sealed_batch(c, nblocks, first_blocks, seed):
    """per segment random plaintext blocks sealed under nonce + first block: (keys, nonces, plains, ciphers)"""
    rng = np.random.default_rng(seed)
    n = len(nblocks)
    d_keys = E.prepare_keys([rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(n)])
    nonces = [rng.integers(0, 256, 12, dtype=np.uint8).tobytes() for _ in range(n)]
    d_nonces = torch.from_numpy(np.frombuffer(b"".join(nonces), dtype=np.uint8).copy()).cuda()
    d_start = torch.from_numpy(np.frombuffer(b"".join(add_to_nonce(x, fb) for x, fb in zip(nonces, first_blocks)),
                                             dtype=np.uint8).copy()).cuda()
    g = torch.Generator(device="cuda").manual_seed(seed)
    plains = [torch.randint(0, 256, (nb * IB,), dtype=torch.uint8, device="cuda", generator=g) for nb in nblocks]
    ciphers = [torch.empty(nb * BLOCK, dtype=torch.uint8, device="cuda") for nb in nblocks]
    E.seal_segments_sized(c, plains, nblocks, IB, d_keys, d_start, ciphers)
    torch.cuda.synchronize()
    return d_keys, d_nonces, plains, ciphers


def ranged_stats(L, c):
    v = [ctypes.c_ulonglong() for _ in range(2)]
    L.ec_gcm_ranged_stats(c.ctx, *[ctypes.byref(x) for x in v])
    return [x.value for x in v]


def case_a(L, c, st, args, parent):
    nseg, nb, head = args.segments, 9060, 6608
    nblocks = [nb] * nseg
    d_keys, d_nonces, plains, ciphers = sealed_batch(c, nblocks, [0] * nseg, 6)
    mk = lambda n: [torch.empty(n, dtype=torch.uint8, device="cuda") for _ in range(nseg)]  # noqa: E731
    o_sized, o_ranged, o_parent = mk(nb * IB), mk(nb * IB), mk(nb * IB)
    cut_len = (nb - 1) * IB  # from 6608 bytes into the first block to 6608 bytes into the last
    o_cut = mk(cut_len)
    status = [torch.empty(nseg, dtype=torch.int32, device="cuda") for _ in range(4)]
    zeros, whole = [0] * nseg, [nb * IB] * nseg
    variants = {}
    if parent:
        variants["parent_sized"] = lambda: parent.open_sized(ciphers, nblocks, d_keys, d_nonces, o_parent, status[3], st)
    variants["sized"] = lambda: E.open_segments_sized(c, ciphers, nblocks, IB, d_keys, d_nonces, o_sized, status[0],
                                                      stream=st)
    variants["ranged_aligned"] = lambda: E.open_ranges_sized(c, ciphers, zeros, nblocks, zeros, whole, IB, d_keys,
                                                             d_nonces, o_ranged, status[1], stream=st)
    variants["ranged_head6608"] = lambda: E.open_ranges_sized(c, ciphers, zeros, nblocks, [head] * nseg,
                                                              [cut_len] * nseg, IB, d_keys, d_nonces, o_cut, status[2],
                                                              stream=st)
    # (6608 is a multiple of 16: with aligned buffers that is still the aligned path; 6609 is not)
    o_odd = mk(cut_len)
    status.append(torch.empty(nseg, dtype=torch.int32, device="cuda"))
    variants["ranged_head6609"] = lambda: E.open_ranges_sized(c, ciphers, zeros, nblocks, [head + 1] * nseg,
                                                              [cut_len] * nseg, IB, d_keys, d_nonces, o_odd, status[4],
                                                              stream=st)
    if parent:
        variants["parent_sized_again"] = variants["parent_sized"]
    res = B.measure(variants, args.iters, args.repeats, st)
    torch.cuda.synchronize()
    for s in status[:3] + status[4:] + (status[3:4] if parent else []):
        assert s.cpu().tolist() == [-1] * nseg
    for g in range(nseg):
        assert torch.equal(o_sized[g], plains[g]) and torch.equal(o_ranged[g], plains[g])
        assert torch.equal(o_cut[g], plains[g][head:head + cut_len])
        assert torch.equal(o_odd[g], plains[g][head + 1:head + 1 + cut_len])
        assert not parent or torch.equal(o_parent[g], plains[g])
    med = lambda k: res[k]["device_us_median"]  # noqa: E731
    res["workload"] = f"{nseg} x {nb} blocks of {IB} B, valid ciphertext"
    res["GBps_plaintext"] = {k: nseg * nb * IB / med(k) / 1e3 for k in variants}
    res["ranged_aligned_over_sized_device"] = med("ranged_aligned") / med("sized")
    res["ranged_head6608_over_aligned_device"] = med("ranged_head6608") / med("ranged_aligned")
    res["ranged_head6609_bytewise_over_aligned_device"] = med("ranged_head6609") / med("ranged_aligned")
    if parent:
        res["parent_build"] = parent.L.ec_build_id().decode()
        res["ranged_aligned_over_parent_sized_device"] = med("ranged_aligned") / med("parent_sized")
        res["sized_over_parent_sized_device"] = med("sized") / med("parent_sized")
        res["parent_again_over_parent_device"] = med("parent_sized_again") / med("parent_sized")
    return res


def case_w(L, c, st, args):
    k, n, ess = 29, 80, 256
    scheme = eestream.RSScheme(eestream.new_fec(k, n), ess)
    codec = eestream.SegmentCodec(scheme)
    rng = np.random.default_rng(20261022)
    nr, length = args.ranges, 1 << 20
    geos = [downloads.range_geometry(SEGMENT, int(rng.integers(0, SEGMENT - length + 1)), length, scheme)
            for _ in range(nr)]
    assert all(g.skip == 0 and g.nstripes == g.nblocks for g in geos)  # a block is a stripe
    nblocks = [g.nblocks for g in geos]
    d_keys, d_nonces, plains, ciphers = sealed_batch(scheme, nblocks, [g.first_block for g in geos], 7)
    pieces = [torch.empty((n, g.piece_length), dtype=torch.uint8, device="cuda") for g in geos]
    codec.encode_segments_sized(ciphers, nblocks, pieces)
    torch.cuda.synchronize()
    ranges = [(g, {int(x): p[int(x)] for x in rng.permutation(n)[:k]}) for g, p in zip(geos, pieces)]
    got = {}

    def ranged():
        got["r"] = downloads.download_ranges(scheme, ranges, d_keys, d_nonces, stream=st)

    # the same downloads served as whole segments: --whole-count of them, scaled
    wc = args.whole_count
    wnb = cipher_geometry(SEGMENT)[0]
    wk, wn, wplains, wciphers = sealed_batch(scheme, [wnb] * wc, [0] * wc, 8)
    wpieces = [torch.empty((n, wnb * ess), dtype=torch.uint8, device="cuda") for _ in range(wc)]
    codec.encode_segments_sized(wciphers, [wnb] * wc, wpieces)
    torch.cuda.synchronize()
    wsets = [(wnb * BLOCK, {int(x): p[int(x)] for x in rng.permutation(n)[:k]}) for p in wpieces]

    def whole():
        encs = downloads.decode_downloads(scheme, wsets, stream=st)
        got["w"] = downloads.open_downloads(scheme, [(SEGMENT, e) for e in encs], wk, wn, stream=st)

    res = B.measure({"download_ranges": ranged, "whole_segments": whole}, args.iters, args.repeats, st)
    torch.cuda.synchronize()
    outs, status = got["r"]
    assert status.cpu().tolist() == [-1] * nr
    for g, o, p in zip(geos, outs, plains):
        assert torch.equal(o, p[g.head:g.head + g.length])
    wouts, wstatus = got["w"]
    assert wstatus.cpu().tolist() == [-1] * wc
    assert all(torch.equal(o, p[:SEGMENT]) for o, p in zip(wouts, wplains))
    r, w = res["download_ranges"], res["whole_segments"]
    res["workload"] = (f"{nr} ranges of 1 MiB at random offsets of 64 MiB segments, RS(29,80), {sum(nblocks)} blocks, "
                       f"{sum(g.piece_length for g in geos) * k / 1e6:.1f} MB of piece ranges in")
    res["bytewise_ranges"] = sum(g.head % 16 != 0 for g in geos)
    res["ranges_wall_ms"] = r["wall_us_median"] / 1e3
    res["ranges_device_ms"] = r["device_us_median"] / 1e3
    res["ranges_GBps_plaintext_wall"] = nr * length / r["wall_us_median"] / 1e3
    res["ranges_GBps_plaintext_device"] = nr * length / r["device_us_median"] / 1e3
    res["whole_count_timed"] = wc
    res["whole_wall_ms_scaled_to_ranges"] = w["wall_us_median"] / 1e3 * nr / wc
    res["whole_device_ms_scaled_to_ranges"] = w["device_us_median"] / 1e3 * nr / wc
    res["whole_is_scaled"] = f"timed on {wc} whole segments, multiplied by {nr}/{wc}"
    res["whole_over_ranges_wall"] = res["whole_wall_ms_scaled_to_ranges"] / res["ranges_wall_ms"]
    torch.cuda.synchronize()
    scheme.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--cases", default="aw")
    ap.add_argument("--segments", type=int, default=64, help="case a: segments of 9060 blocks")
    ap.add_argument("--ranges", type=int, default=256, help="case w: ranges of 1 MiB")
    ap.add_argument("--whole-count", type=int, default=4, help="case w: whole segments timed, then scaled")
    ap.add_argument("--parent-lib", default=None, help="case a: another build of libuplink_ec.so to alternate with")
    ap.add_argument("--out", default=None, help="also write the JSON to this file")
    ap.add_argument("--window-s", type=float, default=B.WINDOW_S, help="least work per timed window")
    args = ap.parse_args()
    B.WINDOW_S = args.window_s
    torch.cuda.set_device(0)
    L = _native.load()
    c = B.Ctx()
    st = torch.cuda.Stream()
    out = {"build": L.ec_build_id().decode(), "iters": args.iters, "repeats": args.repeats}
    if "a" in args.cases:
        parent = Lib(args.parent_lib) if args.parent_lib else None
        out["a"] = case_a(L, c, st, args, parent)
        if parent:
            torch.cuda.synchronize()
            parent.L.ec_destroy(parent.ctx)
        torch.cuda.empty_cache()
    if "w" in args.cases:
        out["w"] = case_w(L, c, st, args)
    out["ranged_stats"] = ranged_stats(L, c)
    torch.cuda.synchronize()
    L.ec_destroy(c.ctx)
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
