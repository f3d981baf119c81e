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
  seal_inline_uploads  the encrypted inline data and encrypted content keys of a
                    batch of uploads too small to be erasure coded
                    (ec_gcm_seal_messages)
"""
from __future__ import annotations

from typing import Sequence, Tuple

from . import _batch as B
from .eestream import SegmentCodec
from .encryption import DEFAULT_BLOCK_SIZE, TAG_SIZE, device_rows, seal_messages, seal_segments_sized


def upload_geometry(size: int, es) -> Tuple[int, int, int]:
    """PadReader's sizes of a segment of `size` bytes under erasure scheme `es`
    (encryption.PadReader: at least 4 bytes of padding, up to whole stripes):
    (padded_size, piece_size, nstripes)."""
    if size < 0:
        raise ValueError("size is negative")
    stripe = es.stripe_size()
    padded = size + 4 + (stripe - (size + 4) % stripe) % stripe
    return padded, padded // es.required_count(), padded // stripe


def _check_buffer(size: int, buf, need: int):
    """an upload's buffer: a contiguous uint8 tensor of at least `need` bytes"""
    import torch
    if buf.dtype != torch.uint8 or not buf.is_contiguous():
        raise ValueError("an upload's buffer is a contiguous uint8 tensor")
    if buf.numel() < need:
        raise ValueError(f"an upload of {size} bytes needs a buffer of {need} bytes, got {buf.numel()}")


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
        _check_buffer(int(size), buf, padded)
        geo.append((int(size), piece_size, ns, buf))
    with B.stream_scope(stream):
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
        _check_buffer(int(size), buf, plain_cap)
        geo.append((int(size), nblocks, enc_len, buf))
    with B.stream_scope(stream):
        # one allocation per upload: each is 16-byte aligned
        encs = [torch.empty(upload_geometry(enc_len, scheme)[0], dtype=torch.uint8, device=buf.device)
                for _, _, enc_len, buf in geo]
        seal_segments_sized(scheme, [g[3] for g in geo], [g[1] for g in geo], block_size - TAG_SIZE, dev_keys,
                            dev_nonces, encs, data_len=[g[0] for g in geo], stream=stream)
    return [(g[2], e) for g, e in zip(geo, encs)]


def seal_inline_uploads(scheme, uploads: Sequence[object], content_keys, nonces, derived_keys, key_nonces, *,
                        stream=None):
    """What the splitter does for an object of up to maxInlineSize bytes
    (splitter/splitter.go:160,189), for a batch: upload g's plaintext
    (uploads[g], a contiguous uint8 device tensor) is sealed whole under its
    content key and nonce -- encryption.Encrypt(inline, cipher, &contentKey,
    &nonce) --, and its content key under its derived key and key nonce --
    encryption.EncryptKey(&contentKey, cipher, key, &keyNonce).  One
    ec_gcm_seal_messages call over the 2N messages.  content_keys and
    derived_keys are [N, 32], nonces and key_nonces [N, 12]: device tensors, or
    N byte strings each (nonces cut to their first 12 bytes).  Returns
    (encrypted, encrypted_keys): encrypted[g] is the device tensor of upload g's
    size + 16 bytes (empty for an empty upload: Encrypt does not seal an empty
    slice) and encrypted_keys the [N, 48] device tensor.  Asynchronous on
    `stream`."""
    import torch

    uploads = list(uploads)
    n = len(uploads)
    for buf in uploads:
        if buf.dtype != torch.uint8 or not buf.is_contiguous():
            raise ValueError("an upload's plaintext is a contiguous uint8 tensor")
    dev = uploads[0].device if uploads else B.default_device()
    with B.stream_scope(stream):
        ck, dk = device_rows(content_keys, 32, dev), device_rows(derived_keys, 32, dev)
        nn, kn = device_rows(nonces, 12, dev), device_rows(key_nonces, 12, dev)
        if not (len(ck) == len(dk) == len(nn) == len(kn) == n):
            raise ValueError("one content key, nonce, derived key and key nonce per upload")
        encs = [torch.empty(b.numel() + TAG_SIZE if b.numel() else 0, dtype=torch.uint8, device=dev) for b in uploads]
        enc_keys = torch.empty((n, 48), dtype=torch.uint8, device=dev)
        if n == 0:
            return encs, enc_keys
        data = [g for g, b in enumerate(uploads) if b.numel()]  # (an empty upload is not a message)
        if len(data) == n:
            keys32, nonces12 = torch.cat([ck, dk]), torch.cat([nn, kn])
        else:
            idx = torch.tensor(data, dtype=torch.long, device=dev)
            keys32, nonces12 = torch.cat([ck[idx], dk]), torch.cat([nn[idx], kn])
        plains = [uploads[g] for g in data] + [ck.data_ptr() + 32 * g for g in range(n)]
        outs = [encs[g] for g in data] + [enc_keys.data_ptr() + 48 * g for g in range(n)]
        lens = [uploads[g].numel() for g in data] + [32] * n
        seal_messages(scheme, plains, lens, keys32, nonces12, outs, stream=stream)
        # keys32 and nonces12 are read by the queued kernels: freed on this stream they are reused only
        # behind them; a raw stream handle is not the stream they were made on, so wait for it
        B.wait_if_raw(stream)
    return encs, enc_keys
