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

from typing import Dict, Iterable, List, Sequence

from . import _batch as B
from . import _native as N
from .eestream import NotEnoughShares, _raise


def _call_args(segments, out_ptrs):
    """(nseg, nshares[], nums[], pieces[], ntargets[], targets[], outputs[]) of a batch, as both C calls take them"""
    nsh, nums, ptrs, ntg, tgts = [], [], [], [], []
    for snums, pieces, targets in segments:
        snums, pieces, targets = list(snums), list(pieces), list(targets)
        if len(snums) != len(pieces):
            raise ValueError("nums and pieces differ in length")
        nsh.append(len(snums))
        nums += snums
        ptrs += pieces
        ntg.append(len(targets))
        tgts += targets
    return (len(nsh), B.int_array(nsh), B.int_array(nums), B.ptr_array(ptrs), B.int_array(ntg), B.int_array(tgts),
            B.ptr_array(out_ptrs, len(tgts), "output", "target"))


def repair_call(ctx, segments, out_ptrs: Sequence[int], nstripes: int, flags: int = 0, status=None, stream=None) -> int:
    """ec_repair_segments_sets on raw arguments; returns its code.  segments:
    (nums, pieces, targets) each, pieces and out_ptrs device tensors or addresses."""
    return N.load().ec_repair_segments_sets(ctx, *_call_args(segments, out_ptrs), nstripes, flags,
                                            None if status is None else B.addr(status), B.stream_handle(stream))


def repair_call_sized(ctx, segments, out_ptrs: Sequence[int], nstripes_list: Sequence[int], flags: int = 0, status=None,
                      stream=None) -> int:
    """ec_repair_segments_sized on raw arguments; returns its code.  As
    repair_call with a stripe count per segment."""
    args = _call_args(segments, out_ptrs)
    return N.load().ec_repair_segments_sized(ctx, *args, B.size_array(nstripes_list, args[0], "stripe count"), flags,
                                             None if status is None else B.addr(status), B.stream_handle(stream))


def _repair(ctx, call, segments, plens, ess, k, check, hash_pieces, hash_algo, stream):
    """The repair of a validated batch, behind both public forms: plens[g] is
    the piece length of segment g (a multiple of ess) and call(segments, rows,
    stripe counts, flags, status) the raw call over the batch or a part of it."""
    import torch

    dev = next((p.device for _, pieces, _ in segments for p in pieces), None)
    if dev is None:  # nothing to repair from
        return ([], []) if hash_pieces else []
    stripes = [p // ess for p in plens]
    flags = N.EC_FLAG_CHECK_SHARES if check else 0
    with B.stream_scope(stream):
        # one allocation per segment: each is 16-byte aligned, so each stays in the pass
        outs = [torch.empty((len(t), p), dtype=torch.uint8, device=dev) for (_, _, t), p in zip(segments, plens)]
        rows = [o[i] for o in outs for i in range(o.shape[0])]
        status = torch.empty(len(segments), dtype=torch.int32, device=dev) if check else None
        _raise(ctx, call(segments, rows, stripes, flags, status))
        bad = [g for g, s in enumerate(B.read_back(status, stream)) if s] if check else []
        if bad:
            # a flagged segment is corrected as Decode corrects it, its pieces rewritten in place, with
            # its own stripe count (the scratch takes the largest); then those segments are repaired again
            scratch = torch.empty(max(plens[g] for g in bad) * k, dtype=torch.uint8, device=dev)
            for g in bad:
                nums, pieces, _ = segments[g]
                rc = N.load().ec_decode_segments(ctx, len(nums), B.int_array(nums), B.ptr_array(pieces), stripes[g],
                                                 scratch.data_ptr(), B.stream_handle(stream))
                _raise(ctx, rc)
            again = torch.empty(len(bad), dtype=torch.int32, device=dev)
            rows2 = [outs[g][i] for g in bad for i in range(outs[g].shape[0])]
            _raise(ctx, call([segments[g] for g in bad], rows2, [stripes[g] for g in bad], flags, again))
            if any(B.read_back(again, stream)):  # (corrected shares are codewords: not expected)
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
    ctx = B.ctx_of(scheme_or_ctx)
    lib = N.load()
    segments = [(list(a), list(b), list(c)) for a, b, c in segments]
    ess, k = lib.ec_share_size(ctx), lib.ec_required(ctx)
    if ess <= 0 or k <= 0:
        _raise(None, N.EC_ERR_INVALID_ARG)
    lens = {p.numel() for _, pieces, _ in segments for p in pieces}
    if len(lens) > 1:  # one piece length for the whole batch
        _raise(ctx, N.EC_ERR_SHARE_SIZE)
    plen = lens.pop() if lens else 0
    if plen % ess:
        _raise(ctx, N.EC_ERR_INVALID_ARG)

    def call(segs, rows, stripes, flags, status):
        return repair_call(ctx, segs, rows, plen // ess, flags, status, stream)

    return _repair(ctx, call, segments, [plen] * len(segments), ess, k, check, hash_pieces, hash_algo, stream)


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
    ctx = B.ctx_of(scheme_or_ctx)
    segments = [(list(a), list(b), list(c)) for a, b, c in segments]
    ess, k = _sizes_of(scheme_or_ctx, ctx)
    if ess <= 0 or k <= 0:
        _raise(None, N.EC_ERR_INVALID_ARG)
    plens = []
    for _, pieces, _ in segments:
        plen = pieces[0].numel() if pieces else 0
        if any(p.numel() != plen for p in pieces):
            _raise(ctx, N.EC_ERR_SHARE_SIZE)
        if plen % ess:
            _raise(ctx, N.EC_ERR_INVALID_ARG)
        plens.append(plen)

    def call(segs, rows, stripes, flags, status):
        return repair_call_sized(ctx, segs, rows, stripes, flags, status, stream)

    return _repair(ctx, call, segments, plens, ess, k, check, hash_pieces, hash_algo, stream)


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
