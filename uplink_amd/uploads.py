"""A batch of concurrent uploads of different sizes encoded in one call
(include/uplink_ec.h ec_encode_segments_sized): the counterpart of downloads.py.

What it stands in for: the upload of one segment (private/storage/streams/
single.go:233-238) wraps the segment's reader in encryption.PadReader for the
erasure scheme's stripe size and hands it to the encoder, which reads the n
pieces of that one segment (segmentupload/encode.go:39-75).  Many such uploads
are in flight at once, of as many sizes as there are objects.  Here they are one
stream-ordered pass on the GPU.

  upload_geometry   (padded_size, piece_size, nstripes) of an upload
  encode_uploads    the pieces of a batch of uploads and, with hash_pieces, the
                    hash each piece is sent with (ec_hash_segments_sized; SHA-256 by
                    hash_algo: ec_sha256_segments_sized)
  cipher_geometry   (nblocks, plain_cap, enc_len) of an upload through the cipher
  seal_uploads      the encrypted segments of a batch of uploads, each in the
                    buffer encode_uploads takes (ec_gcm_seal_segments_sized)
"""
from __future__ import annotations

from typing import Sequence, Tuple

from .eestream import SegmentCodec
from .encryption import DEFAULT_BLOCK_SIZE, TAG_SIZE, seal_segments_sized


def upload_geometry(size: int, es) -> Tuple[int, int, int]:
    """PadReader's sizes of a segment of `size` bytes under erasure scheme `es`
    (encryption.PadReader: at least 4 bytes of padding, up to whole stripes):
    (padded_size, piece_size, nstripes)."""
    if size < 0:
        raise ValueError("size is negative")
    stripe = es.stripe_size()
    padded = size + 4 + (stripe - (size + 4) % stripe) % stripe
    return padded, padded // es.required_count(), padded // stripe


def encode_uploads(scheme, uploads: Sequence[Tuple[int, object]], *, parity_only: bool = False,
                   hash_pieces: bool = False, hash_algo=None, stream=None):
    """uploads: per upload (size, buffer); `buffer` is a uint8 device tensor of
    at least padded_size bytes (upload_geometry) whose first `size` bytes are
    the data.  Its tail is overwritten with PadReader's padding.  Returns per
    upload a [n, piece_size] device tensor of its pieces ([n-k, piece_size] with
    parity_only).  A buffer that is too short raises before anything is queued.
    With hash_pieces it returns (pieces, hashes): hashes[g] is the [n, 32]
    device tensor of the hashes upload g's pieces are sent with
    (piecestore/upload.go:270) -- BLAKE3, or the algorithm hash_algo names
    (piecehash.PieceHashAlgorithm; WithPieceHashAlgo) --, all n rows also with parity_only (the data
    pieces are then hashed in place from the padded buffer); the rows are views
    of one buffer, filled by one ec_hash_segments_sized (ec_sha256_segments_sized)
    call queued behind the encode.  Asynchronous on `stream`."""
    import torch

    codec = SegmentCodec(scheme)
    rows = scheme.total_count() - (scheme.required_count() if parity_only else 0)
    geo = []
    for size, buf in uploads:
        padded, piece_size, ns = upload_geometry(int(size), scheme)
        if buf.dtype != torch.uint8 or not buf.is_contiguous():
            raise ValueError("an upload's buffer is a contiguous uint8 tensor")
        if buf.numel() < padded:
            raise ValueError(f"an upload of {int(size)} bytes needs a buffer of {padded} bytes, got {buf.numel()}")
        geo.append((int(size), piece_size, ns, buf))
    ts = stream if hasattr(stream, "cuda_stream") else None
    with torch.cuda.stream(ts) if ts is not None else _Null():
        # one allocation per upload: each is 16-byte aligned, so every segment stays in the pass
        outs = [torch.empty((rows, piece_size), dtype=torch.uint8, device=buf.device) for _, piece_size, _, buf in geo]
        codec.encode_segments_sized([g[3] for g in geo], [g[2] for g in geo], outs, data_len=[g[0] for g in geo],
                                    parity_only=parity_only, stream=stream)
        if not hash_pieces:
            return outs
        dev = geo[0][3].device if geo else "cuda"
        hashes = torch.empty((len(geo), scheme.total_count(), 32), dtype=torch.uint8, device=dev)
        codec.hash_segments_sized([g[3] for g in geo], [g[2] for g in geo], outs, hashes, parity_only=parity_only,
                                  stream=stream, algo=hash_algo)
    return outs, [hashes[g] for g in range(len(geo))]


def cipher_geometry(size: int, block_size: int = DEFAULT_BLOCK_SIZE) -> Tuple[int, int, int]:
    """TransformWriterPadded's sizes (splitter/splitter.go:156,170) of a segment
    of `size` plaintext bytes sealed in encrypted blocks of block_size bytes:
    (nblocks, plain_cap, enc_len) -- its GCM blocks, the bytes its padded
    plaintext takes and the bytes of its ciphertext (pipeline.SegmentGeometry's
    nblocks, plain_cap and enc_len)."""
    if size < 0:
        raise ValueError("size is negative")
    in_block = block_size - TAG_SIZE
    if in_block <= 0:
        raise ValueError(f"encrypted block size {block_size} too small")
    plain_cap = size + 4 + (in_block - (size + 4) % in_block) % in_block
    nblocks = plain_cap // in_block
    return nblocks, plain_cap, nblocks * block_size


def seal_uploads(scheme, uploads: Sequence[Tuple[int, object]], dev_keys, dev_nonces, *,
                 block_size: int = DEFAULT_BLOCK_SIZE, stream=None):
    """uploads: per upload (size, buffer); `buffer` is a contiguous uint8 device
    tensor of at least plain_cap bytes (cipher_geometry) whose first `size`
    bytes are the plaintext.  Its tail is overwritten with PadReader's padding
    to the cipher's block.  Upload g is sealed under prepared key g of dev_keys
    (encryption.prepare_keys) and nonce dev_nonces[12*g:12*g+12].  Returns per
    upload (enc_len, enc_buffer): enc_buffer holds the enc_len ciphertext bytes
    and has the upload_geometry(enc_len, scheme)[0] bytes encode_uploads asks
    for, so the list goes straight into encode_uploads -- the seal lands in the
    RS encoder's input and no byte moves between the stages, as pipeline.py
    does for one size.  A buffer that is too short raises before anything is
    queued.  Asynchronous on `stream`."""
    import torch

    geo = []
    for size, buf in uploads:
        nblocks, plain_cap, enc_len = cipher_geometry(int(size), block_size)
        if buf.dtype != torch.uint8 or not buf.is_contiguous():
            raise ValueError("an upload's buffer is a contiguous uint8 tensor")
        if buf.numel() < plain_cap:
            raise ValueError(f"an upload of {int(size)} bytes needs a buffer of {plain_cap} bytes, got {buf.numel()}")
        geo.append((int(size), nblocks, enc_len, buf))
    ts = stream if hasattr(stream, "cuda_stream") else None
    with torch.cuda.stream(ts) if ts is not None else _Null():
        # one allocation per upload: each is 16-byte aligned
        encs = [torch.empty(upload_geometry(enc_len, scheme)[0], dtype=torch.uint8, device=buf.device)
                for _, _, enc_len, buf in geo]
        seal_segments_sized(scheme, [g[3] for g in geo], [g[1] for g in geo], block_size - TAG_SIZE, dev_keys,
                            dev_nonces, encs, data_len=[g[0] for g in geo], stream=stream)
    return [(g[2], e) for g, e in zip(geo, encs)]


class _Null:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False
