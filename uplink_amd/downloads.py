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

Ranged downloads.  uplink's Download takes an offset and a length, and the
range narrows at every layer (store.go:174-253, 347-382; eestream/
decode.go:199-227), so a 1 MiB read costs about 1 MiB of pieces:

  object_ranges      the (segment, offset, length) triples an object range falls on
  range_geometry     the blocks, stripes and piece bytes a segment range covers
  decode_ranges      the covered cipher blocks of a batch of ranges, from piece ranges
  open_ranges        their plaintext ranges (ec_gcm_open_ranges_sized)
  download_ranges    the two in stream order

Inline segments.  An object of up to 4 KiB is never erasure coded: its whole
ciphertext is one GCM message under its content key, itself sealed under the
derived key (streams/store.go:349, 360-375):

  open_content_keys      DecryptKey for a batch (ec_gcm_open_messages)
  open_inline_downloads  DecryptKey, then Decrypt under the keys it produced,
                         which never leave the device
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Sequence, Tuple

from . import _batch as B
from . import _native as N
from .ecclient import calc_padded
from .eestream import SegmentCodec, _raise
from .encryption import (DEFAULT_BLOCK_SIZE, TAG_SIZE, DecryptionFailed, KeyDecryptionFailed, device_rows,
                         open_messages, open_ranges_sized, open_segments_sized)
from .streams import calc_encompassing_blocks


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


def _decode(scheme, sets, nstripes, out_sizes, error_detection, collect_errors, stream):
    """The decode behind decode_downloads and decode_ranges: one
    rebuild_segments_sized (with error_detection, decode_segments_sized) call
    over the share sets, a (nums, piece tensors) and a stripe count per
    segment.  Returns (outputs, errors): segment g's out_sizes[g] decoded bytes
    and its eestream exception or None."""
    import torch

    codec = SegmentCodec(scheme)
    dev = next((p.device for _, pieces in sets for p in pieces), None)
    if dev is None:
        dev = B.default_device()
    with B.stream_scope(stream):
        # one allocation per output: each is 16-byte aligned, so every segment stays in the pass
        outs = [torch.empty(n, dtype=torch.uint8, device=dev) for n in out_sizes]
        ptrs = [o if o.numel() else None for o in outs]
        errors: List[object] = [None] * len(outs)
        if error_detection:
            codes = codec.decode_segments_sized(sets, nstripes, ptrs, stream=stream, collect=collect_errors)
            errors = [_error_of(scheme.ctx, c) for c in codes]
        else:
            codec.rebuild_segments_sized(sets, nstripes, ptrs, stream=stream)
    return outs, errors


def _share_set(ctx, pieces: Dict[int, object], piece_size: int):
    """(nums, piece tensors) of the pieces that arrived, each piece_size bytes"""
    nums = list(pieces.keys())
    if any(pieces[x].numel() != piece_size for x in nums):
        _raise(ctx, N.EC_ERR_SHARE_SIZE)
    return nums, [pieces[x] for x in nums]


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
    sets, nstripes, geo = [], [], []
    for size, pieces in downloads:
        padded, piece_size, ns = segment_geometry(int(size), scheme)
        sets.append(_share_set(scheme.ctx, pieces, piece_size))
        nstripes.append(ns)
        geo.append((int(size), padded))
    outs, errors = _decode(scheme, sets, nstripes, [padded for _, padded in geo], error_detection, collect_errors,
                           stream)
    res = [o[:size] for o, (size, _) in zip(outs, geo)]
    return (res, errors) if collect_errors else res


def _raise_first_failure(status, stream):
    """check=True of the opens: waits for `stream` and raises
    DecryptionFailed(block) for the first download whose status names a block"""
    for block in B.read_back(status, stream):
        if block >= 0:
            raise DecryptionFailed(block)


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
    for size, enc in sealed:
        nblocks, plain_cap, enc_len = cipher_geometry(int(size), block_size)
        if enc.dtype != torch.uint8 or not enc.is_contiguous():
            raise ValueError("a download's encrypted segment is a contiguous uint8 tensor")
        if enc.numel() != enc_len:
            raise ValueError(f"a download of {int(size)} bytes has {enc_len} encrypted bytes, got {enc.numel()}")
        geo.append((int(size), nblocks, plain_cap, enc))
    dev = geo[0][3].device if geo else B.default_device()
    with B.stream_scope(stream):
        outs = [torch.empty(g[2], dtype=torch.uint8, device=dev) for g in geo]
        status = torch.empty(len(geo), dtype=torch.int32, device=dev)
        if geo:
            open_segments_sized(scheme, [g[3] for g in geo], [g[1] for g in geo], block_size - TAG_SIZE, dev_keys,
                                dev_nonces, outs, status, stream=stream)
        if check:
            _raise_first_failure(status, stream)
    return [o[:g[0]] for o, g in zip(outs, geo)], status


class RangeGeometry(NamedTuple):
    """What a plaintext range of one download costs at every layer
    (range_geometry; uplink_amd/csrc/range_geom.hpp)."""
    plain_size: int
    offset: int
    length: int
    first_block: int    # fb: the covered cipher blocks are the segment's blocks fb .. fb+nblocks-1
    nblocks: int
    head: int           # the range starts head bytes into block fb
    enc_offset: int     # fb * block_size
    enc_length: int     # nblocks * block_size
    first_stripe: int   # fs: the covering stripes are fs .. fs+nstripes-1
    nstripes: int
    skip: int           # the covered blocks start skip bytes into the decoded stripes
    piece_offset: int   # every piece contributes bytes [piece_offset, piece_offset + piece_length)
    piece_length: int


def range_geometry(plain_size: int, offset: int, length: int, es, block_size: int = DEFAULT_BLOCK_SIZE) -> RangeGeometry:
    """The range [offset, offset+length) of a download of plain_size plaintext
    bytes, as the reference narrows it: decryptRanger's Range (streams/
    store.go:347-382, encryption.Transform) asks for the cipher blocks
    CalcEncompassingBlocks(offset, length, block_size - 16) gives, and
    decodedRanger.Range (eestream/decode.go:199-227) for the stripes that cover
    those blocks' encrypted bytes.  A length of 0 covers no block and no stripe.
    ValueError: a negative value, a range outside [0, plain_size], a block size
    the cipher does not take, more blocks than a status word counts (first
    block + blocks above 0x7FFFFFFF).

    Not here: decryptRanger's whole-segment encryption.Decrypt branch
    (store.go:360-375, an encrypted size that is no multiple of the block).
    Those are inline segments; they never reach the erasure path."""
    plain_size, offset, length, block_size = int(plain_size), int(offset), int(length), int(block_size)
    if plain_size < 0 or offset < 0 or length < 0:
        raise ValueError("a size, an offset or a length is negative")
    if offset + length > plain_size:
        raise ValueError(f"the range ({offset}, {length}) is outside a download of {plain_size} bytes")
    ib = block_size - TAG_SIZE
    if ib <= 0 or ib % 16 or ib > 1 << 24:
        raise ValueError("block_size - 16 is a positive multiple of 16, at most 1<<24")
    k, ess = es.required_count(), es.erasure_share_size()
    stripe = k * ess
    if k <= 0 or ess <= 0:
        raise ValueError("the erasure scheme has no stripe")
    fb, nb = calc_encompassing_blocks(offset, length, ib)
    if fb + nb > 0x7FFFFFFF:
        raise ValueError("first block + blocks is above 0x7FFFFFFF")
    if max(plain_size, (fb + nb) * block_size + stripe) >= 1 << 64:
        raise ValueError("a size does not fit 64 bits")
    enc_off, enc_len = fb * block_size, nb * block_size
    fs, ns = calc_encompassing_blocks(enc_off, enc_len, stripe)
    return RangeGeometry(plain_size, offset, length, fb, nb, offset - fb * ib, enc_off, enc_len, fs, ns,
                         enc_off - fs * stripe, fs * ess, ns * ess)


def object_ranges(segment_plain_sizes: Sequence[int], offset: int, length: int) -> List[Tuple[int, int, int]]:
    """The (segment index, offset within it, length) triples the range
    [offset, offset+length) of an object falls on, its segments being
    segment_plain_sizes in order: Store.Get concatenates one ranger per segment
    (streams/store.go:174-253).  Segments the range does not touch are absent, a
    zero-length range gives an empty list, a range beyond the object raises
    ValueError."""
    offset, length = int(offset), int(length)
    sizes = [int(s) for s in segment_plain_sizes]
    if offset < 0 or length < 0 or any(s < 0 for s in sizes):
        raise ValueError("a size, an offset or a length is negative")
    if offset + length > sum(sizes):
        raise ValueError(f"the range ({offset}, {length}) is outside an object of {sum(sizes)} bytes")
    res, start, end = [], 0, offset + length
    for i, s in enumerate(sizes):
        lo, hi = max(offset, start), min(end, start + s)
        if lo < hi:
            res.append((i, lo - start, hi - lo))
        start += s
    return res


def decode_ranges(scheme, ranges: Sequence[Tuple[RangeGeometry, Dict[int, object]]], *, error_detection: bool = False,
                  collect_errors: bool = False, stream=None):
    """decodedRanger.Range (eestream/decode.go:199-227) over a batch: ranges is
    per download (geometry, {piece number: uint8 device tensor}), the piece
    *ranges* as fetched -- bytes [piece_offset, piece_offset + piece_length) of
    each piece that arrived, not whole pieces.  One rebuild_segments_sized (or,
    with error_detection, decode_segments_sized) call over the nstripes stripes
    of each.  Returns per download the enc_length-byte view at `skip` into its
    decoded stripes: the covered cipher blocks, as open_ranges takes them.  A
    piece of another length raises as EC_ERR_SHARE_SIZE does; error_detection
    and collect_errors are decode_downloads'."""
    stripe = scheme.stripe_size()
    geos = [g for g, _ in ranges]
    sets = [_share_set(scheme.ctx, pieces, g.piece_length) for g, pieces in ranges]
    outs, errors = _decode(scheme, sets, [g.nstripes for g in geos], [g.nstripes * stripe for g in geos],
                           error_detection, collect_errors, stream)
    res = [o[g.skip:g.skip + g.enc_length] for o, g in zip(outs, geos)]
    return (res, errors) if collect_errors else res


def open_ranges(scheme, sealed: Sequence[Tuple[RangeGeometry, object]], dev_keys, dev_nonces, *,
                block_size: int = DEFAULT_BLOCK_SIZE, check: bool = False, stream=None):
    """decryptRanger's Range (streams/store.go:347-382) over a batch
    (ec_gcm_open_ranges_sized): sealed is per download (geometry, enc), `enc`
    the uint8 device tensor of exactly the enc_length bytes of its covered
    blocks, at any alignment, as decode_ranges returns it; another length raises
    ValueError.  Download g is opened under prepared key g of dev_keys and
    nonce dev_nonces[12*g:12*g+12] + its absolute block numbers: the key and
    nonce arrays of a whole open.  Returns (plains, status): plains[g] is a
    device tensor of exactly `length` bytes and status the [nseg] int32 device
    tensor, -1 or the smallest absolute number of a covered block of download g
    whose tag did not verify -- every covered block is authenticated whole.
    check=True behaves as in open_downloads."""
    import torch

    ib = int(block_size) - TAG_SIZE
    for geo, enc in sealed:
        if enc.dtype != torch.uint8 or not enc.is_contiguous():
            raise ValueError("a download's covered blocks are a contiguous uint8 tensor")
        if enc.numel() != geo.enc_length or geo.enc_length != geo.nblocks * int(block_size):
            raise ValueError(f"a range of {geo.nblocks} blocks has {geo.nblocks * int(block_size)} encrypted bytes, "
                             f"got {enc.numel()}")
    geos = [g for g, _ in sealed]
    dev = sealed[0][1].device if geos else B.default_device()
    with B.stream_scope(stream):
        outs = [torch.empty(g.length, dtype=torch.uint8, device=dev) for g in geos]
        status = torch.empty(len(geos), dtype=torch.int32, device=dev)
        if geos:
            open_ranges_sized(scheme, [e if g.nblocks else None for g, e in sealed], [g.first_block for g in geos],
                              [g.nblocks for g in geos], [g.head for g in geos], [g.length for g in geos], ib, dev_keys,
                              dev_nonces, [o if o.numel() else None for o in outs], status, stream=stream)
        if check:
            _raise_first_failure(status, stream)
    return outs, status


def download_ranges(scheme, ranges: Sequence[Tuple[RangeGeometry, Dict[int, object]]], dev_keys, dev_nonces, *,
                    block_size: int = DEFAULT_BLOCK_SIZE, error_detection: bool = False, check: bool = False,
                    stream=None):
    """decode_ranges then open_ranges in stream order: the piece ranges of a
    batch of downloads in, (plains, status) out -- plains[g] the bytes
    [offset, offset+length) of download g's plaintext."""
    encs = decode_ranges(scheme, ranges, error_detection=error_detection, stream=stream)
    return open_ranges(scheme, [(g, e) for (g, _), e in zip(ranges, encs)], dev_keys, dev_nonces,
                       block_size=block_size, check=check, stream=stream)


def open_content_keys(scheme, encrypted_keys, derived_keys, key_nonces, *, stream=None):
    """encryption.DecryptKey (streams/store.go:349) for a batch: encrypted_keys
    is [N, 48], derived_keys [N, 32], key_nonces [N, 12] -- device tensors, or N
    byte strings each (nonces cut to their first 12 bytes).  Returns (keys,
    status): keys the [N, 32] device tensor of content keys and status the [N]
    int32 device tensor, 0, or 1 where the key did not verify (its row is then
    zeros).  Asynchronous on `stream`."""
    import torch

    with B.stream_scope(stream):
        ek = device_rows(encrypted_keys, 48)
        dk, kn = device_rows(derived_keys, 32, ek.device), device_rows(key_nonces, 12, ek.device)
        n = len(ek)
        if not (len(dk) == len(kn) == n):
            raise ValueError("one derived key and one key nonce per encrypted key")
        keys = torch.empty((n, 32), dtype=torch.uint8, device=ek.device)
        status = torch.empty(n, dtype=torch.int32, device=ek.device)
        if n:
            open_messages(scheme, [ek.data_ptr() + 48 * g for g in range(n)], [32] * n, dk, kn,
                          [keys.data_ptr() + 32 * g for g in range(n)], status, stream=stream)
    return keys, status


def open_inline_downloads(scheme, ciphers: Sequence[object], encrypted_keys, derived_keys, key_nonces, start_nonces, *,
                          stream=None):
    """decryptRanger for inline segments (streams/store.go:349, then the
    whole-segment branch :360-375), for a batch: download g's content key is
    opened from encrypted_keys[g] under derived_keys[g] and key_nonces[g], and
    its data (ciphers[g], a contiguous uint8 device tensor of plaintext size + 16
    bytes) under that content key and start_nonces[g].  Two ec_gcm_open_messages
    calls in stream order; the content keys the first produces are the key array
    of the second and never leave the device.  Returns per download its
    plaintext as a device tensor, or an exception instance instead:
    KeyDecryptionFailed(0) when its content key did not verify, DecryptionFailed(0)
    when the key did and the data did not (or is shorter than a tag).  An empty
    cipher text gives an empty plaintext (Decrypt does not open an empty slice).
    Waits for the two calls (the statuses are read back)."""
    import torch

    ciphers = list(ciphers)
    n = len(ciphers)
    for c in ciphers:
        if c.dtype != torch.uint8 or not c.is_contiguous():
            raise ValueError("a download's cipher text is a contiguous uint8 tensor")
    keys, kstatus = open_content_keys(scheme, encrypted_keys, derived_keys, key_nonces, stream=stream)
    dev = keys.device
    with B.stream_scope(stream):
        sn = device_rows(start_nonces, 12, dev)
        if not (len(keys) == len(sn) == n):
            raise ValueError("one encrypted key, derived key, key nonce and starting nonce per download")
        data = [g for g, c in enumerate(ciphers) if c.numel() >= TAG_SIZE]
        plains = [torch.empty(max(c.numel() - TAG_SIZE, 0), dtype=torch.uint8, device=dev) for c in ciphers]
        dstatus = torch.zeros(max(len(data), 1), dtype=torch.int32, device=dev)
        if data:
            if len(data) == n:
                k32, n12 = keys, sn
            else:
                idx = torch.tensor(data, dtype=torch.long, device=dev)
                k32, n12 = keys[idx], sn[idx]
            open_messages(scheme, [ciphers[g] for g in data], [ciphers[g].numel() - TAG_SIZE for g in data], k32, n12,
                          [plains[g] if plains[g].numel() else None for g in data], dstatus, stream=stream)
        kst, dst = B.read_back(kstatus, stream), dict(zip(data, B.read_back(dstatus, stream)))
    out: List[object] = []
    for g, c in enumerate(ciphers):
        if kst[g]:
            out.append(KeyDecryptionFailed(0))
        elif 0 < c.numel() < TAG_SIZE or dst.get(g, 0):
            out.append(DecryptionFailed(0))
        else:
            out.append(plains[g])
    return out
