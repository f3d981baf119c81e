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
  open_downloads     the decrypted plaintexts of a batch of decoded downloads
                     (ec_gcm_open_segments_sized)
"""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

from . import _native as N
from .ecclient import calc_padded
from .eestream import SegmentCodec, _raise
from .encryption import DEFAULT_BLOCK_SIZE, TAG_SIZE, DecryptionFailed, open_segments_sized


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


def open_downloads(scheme, sealed: Sequence[Tuple[int, object]], dev_keys, dev_nonces, *,
                   block_size: int = DEFAULT_BLOCK_SIZE, check: bool = False, stream=None):
    """decryptRanger (streams/store.go:347-382) over a batch: sealed is per
    download (plain_size, enc), `enc` the uint8 device tensor of exactly the
    enc_len bytes (uploads.cipher_geometry) of its encrypted segment, as
    decode_downloads returns it; another length raises ValueError.  Download g
    is opened under prepared key g of dev_keys and nonce
    dev_nonces[12*g:12*g+12].  Returns (plains, status): plains[g] is a device
    tensor of exactly plain_size bytes (the padding cut off, as store.go:381)
    and status the [nseg] int32 device tensor, -1 or the first block of
    download g whose tag did not verify (its plaintext is not to be used).
    Asynchronous on `stream`; with check=True it waits and raises
    DecryptionFailed(block) for the first failing download."""
    import torch

    from .uploads import cipher_geometry

    geo = []
    dev = None
    for size, enc in sealed:
        nblocks, plain_cap, enc_len = cipher_geometry(int(size), block_size)
        if enc.dtype != torch.uint8 or not enc.is_contiguous():
            raise ValueError("a download's encrypted segment is a contiguous uint8 tensor")
        if enc.numel() != enc_len:
            raise ValueError(f"a download of {int(size)} bytes has {enc_len} encrypted bytes, got {enc.numel()}")
        if dev is None:
            dev = enc.device
        geo.append((int(size), nblocks, plain_cap, enc))
    if dev is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    ts = stream if hasattr(stream, "cuda_stream") else None
    with torch.cuda.stream(ts) if ts is not None else _Null():
        outs = [torch.empty(g[2], dtype=torch.uint8, device=dev) for g in geo]
        status = torch.empty(len(geo), dtype=torch.int32, device=dev)
        if geo:
            open_segments_sized(scheme, [g[3] for g in geo], [g[1] for g in geo], block_size - TAG_SIZE, dev_keys,
                                dev_nonces, outs, status, stream=stream)
        if check:
            if stream is not None and ts is None:  # a raw stream handle: not the stream the copy below runs on
                torch.cuda.synchronize()
            for block in status.cpu().tolist():  # (a copy on the current stream: it waits for the open)
                if block >= 0:
                    raise DecryptionFailed(block)
    return [o[:g[0]] for o, g in zip(outs, geo)], status


class _Null:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False
