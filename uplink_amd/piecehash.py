"""Piece hashing of the upload, on the engine.

Mirrors:

  PieceHashAlgorithm / GetPieceHashAlgo   private/piecestore/hash.go:12-26
                                          (BLAKE3 unless overridden by WithPieceHashAlgo)
  pb.NewHashFromAlgorithm(algo) fed by    private/piecestore/upload.go:133,155
  io.TeeReader, Hash: client.hash.Sum(nil) private/piecestore/upload.go:270

The reference hashes each piece while it streams to the storage node, one
byte slice at a time.  Here the hash of every piece of a segment is computed
by the GPU next to the encode, from the copies the encoder already has in
HBM (ec_hash_segments / ec_encode_segments_host_hashed), and the uploader
sends the precomputed 32 bytes.  Pieces that each have their own length --
the uploads in flight at once are of as many sizes as objects -- are hashed
in one pass by blake3_pieces_list / hash_segments_sized
(ec_blake3_pieces_list / ec_hash_segments_sized).

Both values of the enum are computed here.  BLAKE3 is the default and a tree:
one piece alone fills the GPU.  SHA-256 (the protobuf zero value, the legacy
option) is one serial chain per piece, so the engine runs it one lane per
piece (ec_sha256_*): a single piece is slow, a batch of segments is thousands
of chains, and that is the shape these calls take it in.  Every entry point
with an `algo` argument takes either; hash_pieces_list / hash_host /
hash_device are the algorithm-neutral names of blake3_pieces_list /
blake3_host / blake3_device.  The streamed host-memory upload
(segment.SegmentPieceReader(hash_pieces=True), ec_upload_begin with
EC_FLAG_HASH_PIECES, ec_encode_segments_host_hashed) hashes with BLAKE3 only.
"""
from __future__ import annotations

import enum

import numpy as np

from . import _batch as B
from . import _native as N
from .eestream import _raise


class PieceHashAlgorithm(enum.IntEnum):
    """pb.PieceHashAlgorithm (storj.io/common/pb)."""
    SHA256 = 0
    BLAKE3 = 1


DEFAULT_ALGORITHM = PieceHashAlgorithm.BLAKE3  # hash.go:25


def _check(algo) -> PieceHashAlgorithm:
    """the algorithm as the enum (ValueError for a value pb.PieceHashAlgorithm does not have)"""
    return PieceHashAlgorithm(algo)


def _sha(algo) -> bool:
    return _check(algo) == PieceHashAlgorithm.SHA256


def hash_host(pieces, algo=DEFAULT_ALGORITHM) -> np.ndarray:
    """[npieces][32] hashes of the rows of a host array [npieces][len]
    (or one 1-D buffer), computed on the GPU (ec_blake3_host / ec_sha256_host)."""
    L = N.load()
    call = L.ec_sha256_host if _sha(algo) else L.ec_blake3_host
    a = np.ascontiguousarray(pieces, dtype=np.uint8)
    if a.ndim == 1:
        a = a.reshape(1, -1)
    npieces, ln = a.shape
    out = np.empty((npieces, 32), dtype=np.uint8)
    rc = call(a.ctypes.data if a.size else None, npieces, ln, ln, out.ctypes.data)
    _raise(None, rc)
    return out


def blake3_host(pieces, algo=DEFAULT_ALGORITHM) -> np.ndarray:
    """hash_host under its first name: BLAKE3 unless `algo` says otherwise."""
    return hash_host(pieces, algo=algo)


def hash_device(base, npieces: int, piece_len: int, piece_stride: int, hashes, run: int = 0,
                run_stride: int = 0, stream=None, algo=DEFAULT_ALGORITHM):
    """ec_blake3_pieces / ec_sha256_pieces on device buffers (torch CUDA tensors
    or addresses): byte t of piece j at base + j*piece_stride +
    (t//run)*run_stride + t%run (run = 0: contiguous).  hashes: npieces*32
    device bytes."""
    L = N.load()
    call = L.ec_sha256_pieces if _sha(algo) else L.ec_blake3_pieces
    rc = call(B.addr(base), npieces, piece_stride, piece_len, run, run_stride, B.addr(hashes), B.stream_handle(stream))
    _raise(None, rc)


def blake3_device(base, npieces: int, piece_len: int, piece_stride: int, hashes, run: int = 0,
                  run_stride: int = 0, stream=None, algo=DEFAULT_ALGORITHM):
    """hash_device under its first name: BLAKE3 unless `algo` says otherwise."""
    hash_device(base, npieces, piece_len, piece_stride, hashes, run=run, run_stride=run_stride, stream=stream,
                algo=algo)


def hash_segments(scheme, segs, parity, nseg: int, nstripes: int, hashes, stream=None, algo=DEFAULT_ALGORITHM):
    """ec_hash_segments: the hashes of all n pieces of nseg device-resident
    segments; data pieces are read in place from the stripe-major segments,
    parity pieces from the EC_FLAG_PARITY_ONLY output.  hashes [nseg][n][32].
    SHA-256 goes through ec_sha256_segments_sized, with each segment's
    pointers computed from this uniform layout."""
    if _sha(algo):
        k, n, ess = scheme.required_count(), scheme.total_count(), scheme.erasure_share_size()
        s0 = B.addr(segs)
        p0 = B.addr(parity) if parity is not None else None
        if not s0 or (n > k and not p0):
            _raise(scheme.ctx, N.EC_ERR_INVALID_ARG)
        seg_bytes, par_bytes = nstripes * k * ess, nstripes * (n - k) * ess
        hash_segments_sized(scheme, [s0 + g * seg_bytes for g in range(nseg)], [nstripes] * nseg,
                            [p0 + g * par_bytes if p0 else None for g in range(nseg)], hashes, parity_only=True,
                            stream=stream, algo=algo)
        return
    rc = N.load().ec_hash_segments(scheme.ctx, B.addr(segs), B.addr(parity) if parity is not None else None, nseg,
                                   nstripes, B.addr(hashes), B.stream_handle(stream))
    _raise(scheme.ctx, rc)


def hash_pieces_list(scheme_or_ctx, tensors, hashes=None, stream=None, algo=DEFAULT_ALGORITHM):
    """ec_blake3_pieces_list / ec_sha256_pieces_list: the hashes of a list of
    contiguous uint8 device tensors of any lengths (an empty one hashes the
    empty input), in one stream-ordered pass.  Returns the [npieces, 32] device
    tensor of their hashes, row i for tensors[i] (`hashes` when given).
    Asynchronous on `stream`; the tensors must stay alive until the stream has
    run the call."""
    sha = _sha(algo)
    import torch

    tensors = list(tensors)
    for t in tensors:
        if t.dtype != torch.uint8 or not t.is_contiguous():
            raise ValueError("a piece is a contiguous uint8 tensor")
    npieces = len(tensors)
    if hashes is None:
        dev = tensors[0].device if tensors else "cuda"
        with B.stream_scope(stream):
            hashes = torch.empty((npieces, 32), dtype=torch.uint8, device=dev)
    elif hashes.numel() != npieces * 32 or hashes.dtype != torch.uint8 or not hashes.is_contiguous():
        raise ValueError("hashes is a contiguous uint8 tensor of npieces*32 bytes")
    ctx = B.ctx_of(scheme_or_ctx)
    L = N.load()
    call = L.ec_sha256_pieces_list if sha else L.ec_blake3_pieces_list
    rc = call(ctx, npieces, B.ptr_array([t if t.numel() else None for t in tensors]),
              B.size_array([t.numel() for t in tensors]), hashes.data_ptr() if npieces else None,
              B.stream_handle(stream))
    _raise(ctx, rc)
    return hashes


def blake3_pieces_list(scheme_or_ctx, tensors, hashes=None, stream=None, algo=DEFAULT_ALGORITHM):
    """hash_pieces_list under its first name: BLAKE3 unless `algo` says otherwise."""
    return hash_pieces_list(scheme_or_ctx, tensors, hashes=hashes, stream=stream, algo=algo)


def hash_segments_sized(scheme_or_ctx, segs, nstripes, pieces, hashes, parity_only: bool = False, stream=None,
                        algo=DEFAULT_ALGORITHM):
    """ec_hash_segments_sized / ec_sha256_segments_sized: all n piece hashes of a batch encoded by
    ec_encode_segments_sized, from the same segs / nstripes / pieces /
    parity_only.  hashes [nseg][n][32] on the device.  With parity_only the data
    pieces are read in place from the stripe-major segments; without it segs may
    be None.  nstripes[g] == 0 skips segment g (its buffers may be None, its hash
    rows stay as they are).  Asynchronous on `stream`."""
    sha = _sha(algo)
    nstripes, pieces = list(nstripes), list(pieces)
    nseg = len(nstripes)
    segs = None if segs is None else list(segs)
    if len(pieces) != nseg or (segs is not None and len(segs) != nseg):
        raise ValueError("one segment, one stripe count and one piece buffer per segment")
    c_nst = B.size_array(nstripes, nseg, "stripe count")
    if parity_only and segs is None:
        raise ValueError("parity_only reads the data pieces from the segments")
    ctx = B.ctx_of(scheme_or_ctx)
    L = N.load()
    call = L.ec_sha256_segments_sized if sha else L.ec_hash_segments_sized
    rc = call(ctx, nseg, None if segs is None else B.ptr_array(segs), c_nst, B.ptr_array(pieces),
              N.EC_FLAG_PARITY_ONLY if parity_only else 0, B.addr(hashes), B.stream_handle(stream))
    _raise(ctx, rc)
