"""bench.py --dump-outputs and the plain / --full split: what a plain run
prints and writes, and that the written arrays are what the timed path
computed (the rebuilt segments are the inputs, the pieces the oracle's)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_options_default_to_a_plain_run(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"


def test_dump_offsets_fixed_and_bounded():
    p, s = bench.dump_offsets(bench.PIECE, bench.S_PAD, 64)
    p2, s2 = bench.dump_offsets(bench.PIECE, bench.S_PAD, 64)
    assert np.array_equal(p, p2) and np.array_equal(s, s2)  # the same in every run
    assert len(p) == 1024 and len(s) == 16384
    assert len(set(p.tolist())) == len(p) and p.min() >= 0 and p.max() < bench.PIECE
    assert len(set(s.tolist())) == len(s) and s.min() >= 0 and s.max() < bench.S_PAD
    for rows in (1, 64, 256, 4096):  # float32 samples + float64 sums of `rows` segments: under 64 MB
        p, s = bench.dump_offsets(bench.PIECE, bench.S_PAD, rows)
        assert rows * (4 * (bench.N * len(p) + len(s)) + 8 * (bench.N + 1)) <= 64 * 1000 * 1000


def test_dump_outputs_on_host_tensors(tmp_path):
    """The arrays of every slot's last launch, and only those: launches of
    3, 3 and 2 segments over a pool of 2 leave 2 segments in slot 0 (the
    third launch) and 3 in slot 1."""
    rng = np.random.default_rng(5)
    pool, b, n, plen, slen = 2, 3, 5, 300, 700
    pieces = [torch.from_numpy(rng.integers(0, 256, (b, n, plen), dtype=np.uint8)) for _ in range(pool)]
    outs = [torch.from_numpy(rng.integers(0, 256, (b, slen), dtype=np.uint8)) for _ in range(pool)]
    bench.dump_outputs(str(tmp_path / "a"), [3, 3, 2], pool, pieces, outs)
    bench.dump_outputs(str(tmp_path / "b"), [3, 3, 2], pool, pieces, outs)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(f"{kind}_{what}_slot{s}.npy" for kind in ("pieces", "rebuilt")
                           for what in ("bytesum", "sample") for s in (0, 1))
    p_off, s_off = bench.dump_offsets(plen, slen, 5, n)
    for slot, nb in ((0, 2), (1, 3)):
        got = {k: np.load(tmp_path / "a" / f"{k}_slot{slot}.npy")
               for k in ("pieces_bytesum", "pieces_sample", "rebuilt_bytesum", "rebuilt_sample")}
        p, o = pieces[slot].numpy()[:nb], outs[slot].numpy()[:nb]
        assert got["pieces_bytesum"].dtype == np.float64 and got["rebuilt_bytesum"].dtype == np.float64
        assert got["pieces_sample"].dtype == np.float32 and got["rebuilt_sample"].dtype == np.float32
        assert np.array_equal(got["pieces_bytesum"], p.sum(axis=2, dtype=np.int64))
        assert np.array_equal(got["rebuilt_bytesum"], o.sum(axis=1, dtype=np.int64))
        assert np.array_equal(got["pieces_sample"], p[:, :, p_off])
        assert np.array_equal(got["rebuilt_sample"], o[:, s_off])
    for nm in names:
        assert np.array_equal(np.load(tmp_path / "a" / nm), np.load(tmp_path / "b" / nm))


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(oracle, tmp_path):
    """A plain run (no --full) of 2 timed steps of 8 segments in launches of
    4: the line carries the headline and ms_per_step and none of the --full
    legs; the dumped arrays are those of the inputs (rebuilt segments) and of
    the oracle's encode (pieces)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--settle-s", "0", "--total-segments", "8", "--batch", "4", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["metric"].startswith("GiB/s erasure encode+decode") and line["unit"] == "GiB/s"
    assert line["higher_is_better"] is True and line["dtype"] == "u8" and line["full"] is False
    assert line["steps"] == 2 and line["segments_timed_this_rank"] == 16
    assert line["ms_per_step"] > 0
    # value is the payload of the timed steps over their wall time, ms_per_step that wall time per step
    assert line["value"] == pytest.approx(8 * bench.S_PAD / 2**30 / (line["ms_per_step"] * 1e-3), rel=2e-3)
    assert line["kernels"]["encode"]["avg_us"] > 0 and line["kernels"]["decode"]["avg_us"] > 0
    for key in ("verified", "cpu_baseline", "other_configs", "fresh_share_sets"):
        assert key not in line
    assert set(line["kernels"]) == {"encode", "decode"}

    from uplink_amd.shard import segment_seed
    p_off, s_off = bench.dump_offsets(bench.PIECE, bench.S_PAD, 8)
    total = 0
    for slot in (0, 1):
        segs = bench.padded_segments(4, segment_seed(slot * 4), torch.device("cuda", 0)).cpu().numpy()
        got = {k: np.load(out / f"{k}_slot{slot}.npy")
               for k in ("pieces_bytesum", "pieces_sample", "rebuilt_bytesum", "rebuilt_sample")}
        total += sum(a.nbytes for a in got.values())
        assert got["rebuilt_sample"].shape == (4, len(s_off)) and got["pieces_sample"].shape == (4, 80, len(p_off))
        assert np.array_equal(got["rebuilt_bytesum"], segs.sum(axis=1, dtype=np.int64))
        assert np.array_equal(got["rebuilt_sample"], segs[:, s_off])
        ref = oracle.FEC(bench.K, bench.N).encode_segment(segs[slot], bench.ESS, threads=8)  # one segment per slot
        assert np.array_equal(got["pieces_bytesum"][slot], ref.sum(axis=1, dtype=np.int64))
        assert np.array_equal(got["pieces_sample"][slot], ref[:, p_off])
    assert len(os.listdir(out)) == 8 and total <= 64 * 1000 * 1000
