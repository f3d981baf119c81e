"""A batch of concurrent downloads of different sizes decoded in one call
(include/uplink_ec.h ec_rebuild_segments_sized / ec_decode_segments_sized).

What it stands in for: ecclient.Client.GetWithOptions (private/ecclient/
client.go:273-308) sizes every download from its own `size` -- calcPadded to
whole stripes, pieceSize = paddedSize / k -- and hands the pieces to one
StripeReader each; the ranger it returns is unpadded to `size`.  Many such
downloads are in flight at once (store.go:240-253), of as many sizes as there
are objects.  Here they are one stream-ordered pass on the GPU.

  segment_geometry   (padded_size, piece_size, nstripes) of a download
  decode_downloads   the plaintext-sized outputs of a batch of downloads
"""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

from . import _native as N
from .ecclient import calc_padded
from .eestream import SegmentCodec, _raise


def segment_geometry(size: int, es) -> Tuple[int, int, int]:
    """GetWithOptions' sizes (client.go:302-303) of a download of `size` bytes
    under erasure scheme `es`: (padded_size, piece_size, nstripes)."""
    if size < 0:
        raise ValueError("size is negative")
    stripe = es.stripe_size()
    padded = calc_padded(size, stripe)
    return padded, padded // es.required_count(), padded // stripe


def _error_of(ctx, code: int):
    try:
        _raise(ctx, code)
    except Exception as e:  # noqa: BLE001 - the eestream exception of the code
        return e
    return None


def decode_downloads(scheme, downloads: Sequence[Tuple[int, Dict[int, object]]], *, error_detection: bool = False,
                     collect_errors: bool = False, stream=None):
    """downloads: per download (size, {piece number: uint8 device tensor}), the
    pieces that arrived, each piece_size bytes (segment_geometry).  Returns per
    download a device tensor of exactly `size` bytes: the padded output without
    its last padded_size - size bytes, as ecclient.unpad.  size == 0 yields an
    empty tensor.

    error_detection: Decode (Correct + Rebuild, stripe.go:407-408) instead of
    Rebuild; a segment with errors has its piece tensors corrected in place and
    the call returns when done.  A piece whose length is not the download's
    piece_size raises as EC_ERR_SHARE_SIZE does.  With collect_errors the
    return value is (outputs, errors): a segment that failed has its eestream
    exception in `errors` (None for the others) instead of raising, and its
    output is not to be used."""
    import torch

    codec = SegmentCodec(scheme)
    ctx = scheme.ctx
    sets, nstripes, geo = [], [], []
    dev = None
    for size, pieces in downloads:
        padded, piece_size, ns = segment_geometry(int(size), scheme)
        nums = list(pieces.keys())
        for x in nums:
            if pieces[x].numel() != piece_size:
                _raise(ctx, N.EC_ERR_SHARE_SIZE)
            if dev is None:
                dev = pieces[x].device
        sets.append((nums, [pieces[x] for x in nums]))
        nstripes.append(ns)
        geo.append((int(size), padded))
    if dev is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    ts = stream if hasattr(stream, "cuda_stream") else None
    with torch.cuda.stream(ts) if ts is not None else _Null():
        # one allocation per output: each is 16-byte aligned, so every segment stays in the pass
        outs = [torch.empty(padded, dtype=torch.uint8, device=dev) for _, padded in geo]
        ptrs = [o if o.numel() else None for o in outs]
        errors: List[object] = [None] * len(outs)
        if error_detection:
            codes = codec.decode_segments_sized(sets, nstripes, ptrs, stream=stream, collect=collect_errors)
            errors = [_error_of(ctx, c) for c in codes]
        else:
            codec.rebuild_segments_sized(sets, nstripes, ptrs, stream=stream)
    res = [o[:size] for o, (size, _) in zip(outs, geo)]
    return (res, errors) if collect_errors else res


class _Null:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False
