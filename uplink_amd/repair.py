"""Segment repair on the engine (include/uplink_ec.h ec_repair_segments_sets):
the pieces a segment has lost, regenerated from any k of those it still has,
without the decoded segment in between.

What it stands in for: the repair and graceful-exit callers that sit on top of
ecclient.Client (private/ecclient/client.go:36-44) fetch k pieces with Get,
decode, and encode again for PutSingleResult / PutPiece (client.go:77-101).
Here piece t is computed straight from the basis shares (Lagrange
interpolation at t's point), a share set and a target set per segment, many
segments in one stream-ordered pass.

  repair_segments      the regenerated pieces of a batch of segments (optionally
                       with every surplus share checked against the basis, flagged
                       segments corrected through Decode and repaired again; and
                       the piece hashes PutPiece sends, piecestore/upload.go:270:
                       BLAKE3 or, by hash_algo, SHA-256)
  repair_segments_sized  the same for segments of different sizes in one call
                       (ec_repair_segments_sized): a repair queue holds segments of as
                       many sizes as there are objects
  SegmentRepairer      which pieces to regenerate, by ecclient.put's threshold rule
                       (client.go:113-116), and the repair of those
"""
from __future__ import annotations

import ctypes
from typing import Dict, Iterable, List, Sequence

from . import _native as N
from .eestream import NotEnoughShares, SegmentCodec, _raise


def _ctx_of(scheme_or_ctx):
    return scheme_or_ctx.ctx if hasattr(scheme_or_ctx, "ctx") else scheme_or_ctx


def _flatten(segments):
    """(nshares, nums, piece addresses, ntargets, targets) of a batch, as the C call takes them."""
    nsh, nums, ptrs, ntg, tgts = [], [], [], [], []
    for snums, pieces, targets in segments:
        snums, pieces, targets = list(snums), list(pieces), list(targets)
        if len(snums) != len(pieces):
            raise ValueError("nums and pieces differ in length")
        nsh.append(len(snums))
        nums += [int(x) for x in snums]
        ptrs += [SegmentCodec._addr(p) for p in pieces]
        ntg.append(len(targets))
        tgts += [int(t) for t in targets]
    return nsh, nums, ptrs, ntg, tgts


def _carr(ctype, values):
    return (ctype * max(len(values), 1))(*values)


def repair_call(ctx, segments, out_ptrs: Sequence[int], nstripes: int, flags: int = 0, status=None, stream=None) -> int:
    """ec_repair_segments_sets on raw arguments; returns its code.  segments:
    (nums, pieces, targets) each, pieces and out_ptrs device tensors or addresses."""
    nsh, nums, ptrs, ntg, tgts = _flatten(segments)
    out_ptrs = [SegmentCodec._addr(p) for p in out_ptrs]
    if len(out_ptrs) != len(tgts):
        raise ValueError("one output per target")
    return N.load().ec_repair_segments_sets(
        ctx, len(nsh), _carr(ctypes.c_int, nsh), _carr(ctypes.c_int, nums), _carr(ctypes.c_void_p, ptrs),
        _carr(ctypes.c_int, ntg), _carr(ctypes.c_int, tgts), _carr(ctypes.c_void_p, out_ptrs), nstripes, flags,
        SegmentCodec._addr(status) if status is not None else None, SegmentCodec._stream(stream))


def repair_segments(scheme_or_ctx, segments, *, check: bool = False, hash_pieces: bool = False, hash_algo=None,
                    stream=None):
    """Regenerate the pieces `targets` of every segment of `segments`, each a
    (nums, pieces, targets): the piece numbers it still has, their device
    tensors (torch uint8, nstripes*ess bytes each, any order) and the piece
    numbers wanted.  Returns, per segment, a [len(targets), nstripes*ess] uint8
    device tensor whose row i is piece targets[i]; with hash_pieces, a pair of
    that list and a list of [len(targets), 32] tensors of their hashes: BLAKE3,
    or the algorithm hash_algo names (piecehash.PieceHashAlgorithm).

    check: every share beyond the k the repair is computed from is compared
    with them in the same pass.  A segment where one disagrees is corrected as
    Decode corrects it (its piece tensors are rewritten in place, as infectious
    corrects share.Data) and repaired once more; infectious' TooManyErrors /
    NotEnoughShares are raised as eestream words them.  With check the call
    returns after the status has been read; without it, it is asynchronous on
    `stream`."""
    import torch

    ctx = _ctx_of(scheme_or_ctx)
    lib = N.load()
    segments = [(list(a), list(b), list(c)) for a, b, c in segments]
    ess = lib.ec_share_size(ctx)
    k = lib.ec_required(ctx)
    if ess <= 0 or k <= 0:
        _raise(None, N.EC_ERR_INVALID_ARG)
    plen = None
    for _, pieces, _ in segments:
        for p in pieces:
            if plen is None:
                plen = p.numel()
            elif p.numel() != plen:
                _raise(ctx, N.EC_ERR_SHARE_SIZE)
    if plen is None:
        return ([], []) if hash_pieces else []
    if plen % ess:
        _raise(ctx, N.EC_ERR_INVALID_ARG)
    nstripes = plen // ess
    dev = segments[0][1][0].device
    ts = stream if hasattr(stream, "cuda_stream") else None
    with torch.cuda.stream(ts) if ts is not None else _Null():
        outs = [torch.empty((len(t), plen), dtype=torch.uint8, device=dev) for _, _, t in segments]
        rows = [o[i] for o in outs for i in range(o.shape[0])]
        status = torch.empty(len(segments), dtype=torch.int32, device=dev) if check else None
        flags = N.EC_FLAG_CHECK_SHARES if check else 0
        _raise(ctx, repair_call(ctx, segments, rows, nstripes, flags, status, stream))

        def read(t):  # (waits for the stream; a raw stream handle is not one torch's copy follows)
            if stream is not None and ts is None:
                torch.cuda.synchronize()
            return t.cpu().tolist()

        if check:
            bad = [g for g, s in enumerate(read(status)) if s]
            if bad:
                scratch = torch.empty(nstripes * k * ess, dtype=torch.uint8, device=dev)
                st = SegmentCodec._stream(stream)
                for g in bad:
                    nums, pieces, _ = segments[g]
                    rc = lib.ec_decode_segments(ctx, len(nums), _carr(ctypes.c_int, nums),
                                                _carr(ctypes.c_void_p, [p.data_ptr() for p in pieces]), nstripes,
                                                scratch.data_ptr(), st)
                    _raise(ctx, rc)
                again = [segments[g] for g in bad]
                st2 = torch.empty(len(bad), dtype=torch.int32, device=dev)
                rows2 = [outs[g][i] for g in bad for i in range(outs[g].shape[0])]
                _raise(ctx, repair_call(ctx, again, rows2, nstripes, flags, st2, stream))
                if any(read(st2)):  # (corrected shares are codewords: not expected)
                    _raise(ctx, N.EC_ERR_TOO_MANY_ERRORS)
        if not hash_pieces:
            return outs
        # every regenerated row in one list call: they have one length and differ in where they lie
        from .piecehash import DEFAULT_ALGORITHM, hash_pieces_list
        algo = DEFAULT_ALGORITHM if hash_algo is None else hash_algo
        flat = hash_pieces_list(ctx, rows, stream=stream, algo=algo) if rows else None
        hashes, at = [], 0
        for o in outs:
            cnt = o.shape[0]
            hashes.append(flat[at:at + cnt] if cnt else torch.empty((0, 32), dtype=torch.uint8, device=dev))
            at += cnt
        return outs, hashes


def repair_call_sized(ctx, segments, out_ptrs: Sequence[int], nstripes_list: Sequence[int], flags: int = 0, status=None,
                      stream=None) -> int:
    """ec_repair_segments_sized on raw arguments; returns its code.  As
    repair_call with a stripe count per segment."""
    nsh, nums, ptrs, ntg, tgts = _flatten(segments)
    out_ptrs = [SegmentCodec._addr(p) for p in out_ptrs]
    if len(out_ptrs) != len(tgts):
        raise ValueError("one output per target")
    nstripes_list = [int(x) for x in nstripes_list]
    if len(nstripes_list) != len(nsh):
        raise ValueError("one stripe count per segment")
    if any(x < 0 for x in nstripes_list):
        raise ValueError("a negative stripe count")
    return N.load().ec_repair_segments_sized(
        ctx, len(nsh), _carr(ctypes.c_int, nsh), _carr(ctypes.c_int, nums), _carr(ctypes.c_void_p, ptrs),
        _carr(ctypes.c_int, ntg), _carr(ctypes.c_int, tgts), _carr(ctypes.c_void_p, out_ptrs),
        _carr(ctypes.c_size_t, nstripes_list), flags, SegmentCodec._addr(status) if status is not None else None,
        SegmentCodec._stream(stream))


def _sizes_of(scheme_or_ctx, ctx):
    """(ess, k) of a scheme or of a raw context"""
    if hasattr(scheme_or_ctx, "erasure_share_size"):
        return scheme_or_ctx.erasure_share_size(), scheme_or_ctx.required_count()
    lib = N.load()
    return lib.ec_share_size(ctx), lib.ec_required(ctx)


def repair_segments_sized(scheme_or_ctx, segments, *, check: bool = False, hash_pieces: bool = False, hash_algo=None,
                          stream=None):
    """repair_segments for segments of different sizes, in one engine call
    (ec_repair_segments_sized): a repair queue holds segments of as many sizes
    as there are objects.  Each segment's piece length is that of its own
    tensors; lengths that differ within one segment are EC_ERR_SHARE_SIZE, a
    length that is no multiple of the share size EC_ERR_INVALID_ARG, both
    raised before anything is queued.  Returns, per segment, its own
    [len(targets), piece_len] uint8 device tensor (with hash_pieces, also the
    [len(targets), 32] hashes, by hash_algo as repair_segments), each allocated
    on its own.

    check: as repair_segments; flagged segments are corrected through Decode
    with their own stripe count and repaired again in one sized call."""
    import torch

    ctx = _ctx_of(scheme_or_ctx)
    segments = [(list(a), list(b), list(c)) for a, b, c in segments]
    ess, k = _sizes_of(scheme_or_ctx, ctx)
    if ess <= 0 or k <= 0:
        _raise(None, N.EC_ERR_INVALID_ARG)
    plens, dev = [], None
    for _, pieces, _ in segments:
        plen = pieces[0].numel() if pieces else 0
        for p in pieces:
            if p.numel() != plen:
                _raise(ctx, N.EC_ERR_SHARE_SIZE)
        if plen % ess:
            _raise(ctx, N.EC_ERR_INVALID_ARG)
        if pieces and dev is None:
            dev = pieces[0].device
        plens.append(plen)
    if dev is None:
        return ([], []) if hash_pieces else []
    lib = N.load()
    stripes = [p // ess for p in plens]
    ts = stream if hasattr(stream, "cuda_stream") else None
    with torch.cuda.stream(ts) if ts is not None else _Null():
        # one allocation per segment: each is 16-byte aligned, so each stays in the pass
        outs = [torch.empty((len(t), p), dtype=torch.uint8, device=dev) for (_, _, t), p in zip(segments, plens)]
        rows = [o[i] for o in outs for i in range(o.shape[0])]
        status = torch.empty(len(segments), dtype=torch.int32, device=dev) if check else None
        flags = N.EC_FLAG_CHECK_SHARES if check else 0
        _raise(ctx, repair_call_sized(ctx, segments, rows, stripes, flags, status, stream))

        def read(t):  # (waits for the stream; a raw stream handle is not one torch's copy follows)
            if stream is not None and ts is None:
                torch.cuda.synchronize()
            return t.cpu().tolist()

        if check:
            bad = [g for g, s in enumerate(read(status)) if s]
            if bad:
                scratch = torch.empty(max(plens[g] for g in bad) * k, dtype=torch.uint8, device=dev)
                st = SegmentCodec._stream(stream)
                for g in bad:
                    nums, pieces, _ = segments[g]
                    rc = lib.ec_decode_segments(ctx, len(nums), _carr(ctypes.c_int, nums),
                                                _carr(ctypes.c_void_p, [p.data_ptr() for p in pieces]), stripes[g],
                                                scratch.data_ptr(), st)
                    _raise(ctx, rc)
                again = [segments[g] for g in bad]
                st2 = torch.empty(len(bad), dtype=torch.int32, device=dev)
                rows2 = [outs[g][i] for g in bad for i in range(outs[g].shape[0])]
                _raise(ctx, repair_call_sized(ctx, again, rows2, [stripes[g] for g in bad], flags, st2, stream))
                if any(read(st2)):  # (corrected shares are codewords: not expected)
                    _raise(ctx, N.EC_ERR_TOO_MANY_ERRORS)
        if not hash_pieces:
            return outs
        # every regenerated row of the batch in one list call, a length per piece
        from .piecehash import DEFAULT_ALGORITHM, hash_pieces_list
        algo = DEFAULT_ALGORITHM if hash_algo is None else hash_algo
        flat = hash_pieces_list(ctx, rows, stream=stream, algo=algo) if rows else None
        hashes, at = [], 0
        for o in outs:
            cnt = o.shape[0]
            hashes.append(flat[at:at + cnt] if cnt else torch.empty((0, 32), dtype=torch.uint8, device=dev))
            at += cnt
        return outs, hashes


class _Null:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


class SegmentRepairer:
    """Which pieces of a segment to regenerate, and their repair.

    The rule is ecclient.put's (client.go:113-116): a segment whose healthy
    pieces number at most the repair threshold (and fewer than the optimal
    threshold) is not acceptable as it stands.  Such a segment gets every piece
    it lacks regenerated, up to the total count; one above the repair threshold
    is left alone."""

    def __init__(self, redundancy):
        self.rs = redundancy

    def needs_repair(self, healthy: Iterable[int]) -> bool:
        h = len(self._healthy(healthy))
        return h <= self.rs.repair_threshold() and h < self.rs.optimal_threshold()

    def _healthy(self, healthy: Iterable[int]) -> List[int]:
        nums = sorted(int(x) for x in healthy)
        if len(set(nums)) != len(nums):
            raise ValueError("a healthy piece number is repeated")
        for x in nums:
            if x < 0 or x >= self.rs.total_count():
                raise ValueError(f"invalid share id: {x}")
        return nums

    def targets(self, healthy: Iterable[int]) -> List[int]:
        """Piece numbers to regenerate given the healthy ones ([] above the
        repair threshold); fewer healthy pieces than the required count cannot
        be repaired (infectious.NotEnoughShares)."""
        nums = self._healthy(healthy)
        if len(nums) < self.rs.required_count():
            raise NotEnoughShares("infectious: must specify at least the number of required shares")
        if not self.needs_repair(nums):
            return []
        have = set(nums)
        return [t for t in range(self.rs.total_count()) if t not in have]

    def repair(self, segments: Sequence[Dict[int, object]], *, check: bool = False, hash_pieces: bool = False,
               hash_algo=None, stream=None):
        """segments: per segment a dict {piece number: device tensor} of its
        healthy pieces.  Returns per segment a dict {piece number: regenerated
        tensor} (empty where no repair is needed); with hash_pieces, also a dict
        {piece number: 32-byte hash tensor} per segment (BLAKE3, or hash_algo's)."""
        return self._repair(repair_segments, segments, check, hash_pieces, hash_algo, stream)

    def repair_sized(self, segments: Sequence[Dict[int, object]], *, check: bool = False, hash_pieces: bool = False,
                     hash_algo=None, stream=None):
        """repair for segments of different sizes (repair_segments_sized): each
        segment's pieces have the segment's own length."""
        return self._repair(repair_segments_sized, segments, check, hash_pieces, hash_algo, stream)

    def _repair(self, call, segments, check, hash_pieces, hash_algo, stream):
        batch, tg = [], []
        for seg in segments:
            nums = list(seg.keys())
            t = self.targets(nums)
            tg.append(t)
            batch.append((nums, [seg[x] for x in nums], t))
        res = call(self.rs, batch, check=check, hash_pieces=hash_pieces, hash_algo=hash_algo, stream=stream)
        outs, hashes = res if hash_pieces else (res, None)
        pieces = [{t: o[i] for i, t in enumerate(ts)} for ts, o in zip(tg, outs)]
        if not hash_pieces:
            return pieces
        return pieces, [{t: h[i] for i, t in enumerate(ts)} for ts, h in zip(tg, hashes)]
