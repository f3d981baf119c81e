"""Segment encryption on the engine: the AES-256-GCM
transform of storj.io/common/encryption as the stream layer uses it.

Mirrors:

  increment / nonce_for_position   encryption.Increment; splitter/common.go:27-32,
                                   streams/store.go:264-270 (deriveContentNonce)
  AESGCMEncrypter                  encryption.NewEncrypter(EncAESGCM, key, nonce, BlockSize)
                                   splitter/splitter.go:156; InBlockSize = BlockSize-16
  encrypt_segment                  encryption.TransformWriterPadded(buf, enc)  splitter.go:170
  AESGCMDecrypter/decrypt_segment  decryptRanger: NewDecrypter, Transform, Unpad
                                   streams/store.go:347-382

Every block is sealed or opened by the GPU (ec_gcm_*); a block whose tag
does not verify raises DecryptionFailed ("cipher: message authentication
failed", Go's crypto/cipher error) naming the block.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native as N
from .eestream import _raise, pad, unpad

TAG_SIZE = 16
DEFAULT_BLOCK_SIZE = 29 * 256  # project.go:84


class DecryptionFailed(Exception):
    def __init__(self, block: int):
        super().__init__(f"cipher: message authentication failed (block {block})")
        self.block = block


def increment(nonce: bytes, amount: int) -> bytes:
    """encryption.Increment: little-endian add with carry (wraps silently)."""
    if amount < 0:
        raise ValueError("amount was negative")
    b = bytearray(nonce)
    for i in range(len(b)):
        if not amount:
            break
        s = b[i] + (amount & 0xFF)
        b[i] = s & 0xFF
        amount = (amount >> 8) + (s >> 8)
    return bytes(b)


def nonce_for_position(part_number: int, index: int) -> bytes:
    """24-byte storj.Nonce for a segment position (splitter/common.go:27-32)."""
    return increment(bytes(24), (part_number << 32) | (index + 1))


def _key(key) -> bytes:
    key = bytes(key)
    if len(key) != 32:
        raise ValueError("AES-256-GCM needs a 32-byte key")
    return key


class AESGCMEncrypter:
    """NewEncrypter(EncAESGCM, key, nonce, encrypted_block_size)."""

    def __init__(self, key, starting_nonce, encrypted_block_size: int = DEFAULT_BLOCK_SIZE):
        if encrypted_block_size <= TAG_SIZE:
            raise ValueError(f"encrypted block size {encrypted_block_size} too small")
        self.key = _key(key)
        self.nonce = bytes(starting_nonce)[:12]  # AESGCMNonce = first 12 bytes of storj.Nonce
        self.block_size = encrypted_block_size

    def in_block_size(self) -> int:
        return self.block_size - TAG_SIZE

    def out_block_size(self) -> int:
        return self.block_size

    def transform(self, padded) -> bytes:
        """Seal every InBlockSize block of `padded` (block b under nonce + b)."""
        a = np.ascontiguousarray(np.frombuffer(bytes(padded), dtype=np.uint8))
        ib = self.in_block_size()
        if a.size % ib:
            raise ValueError(f"input is not a multiple of the block size {ib}")
        nb = a.size // ib
        out = np.empty(nb * self.block_size, dtype=np.uint8)
        rc = N.load().ec_gcm_seal_host(self.key, self.nonce, a.ctypes.data if a.size else None, nb, ib,
                                       out.ctypes.data if out.size else None)
        _raise(None, rc)
        return out.tobytes()


class AESGCMDecrypter(AESGCMEncrypter):
    """NewDecrypter(EncAESGCM, key, nonce, encrypted_block_size)."""

    def in_block_size(self) -> int:
        return self.block_size

    def out_block_size(self) -> int:
        return self.block_size - TAG_SIZE

    def transform(self, cipher) -> bytes:
        a = np.ascontiguousarray(np.frombuffer(bytes(cipher), dtype=np.uint8))
        if a.size % self.block_size:
            raise ValueError(f"input is not a multiple of the block size {self.block_size}")
        nb = a.size // self.block_size
        ib = self.block_size - TAG_SIZE
        out = np.empty(nb * ib, dtype=np.uint8)
        bad = ctypes.c_longlong(-1)
        rc = N.load().ec_gcm_open_host(self.key, self.nonce, a.ctypes.data if a.size else None, nb, ib,
                                       out.ctypes.data if out.size else None, ctypes.byref(bad))
        if rc == N.EC_ERR_AUTH:
            raise DecryptionFailed(bad.value)
        _raise(None, rc)
        return out.tobytes()


def encrypt_segment(plain, key, nonce, block_size: int = DEFAULT_BLOCK_SIZE) -> bytes:
    """TransformWriterPadded(buf, NewEncrypter(...)): PadReader padding to
    InBlockSize, then one GCM seal per block."""
    enc = AESGCMEncrypter(key, nonce, block_size)
    return enc.transform(pad(bytes(plain), enc.in_block_size()))


def decrypt_segment(cipher, key, nonce, plain_size: int | None = None, block_size: int = DEFAULT_BLOCK_SIZE) -> bytes:
    """decryptRanger's Transform + Unpad: plain_size when known (store.go:381),
    else the padding trailer."""
    padded = AESGCMDecrypter(key, nonce, block_size).transform(cipher)
    return padded[:plain_size] if plain_size is not None else unpad(padded)


def prepare_keys(keys, dev_buf=None, stream=None):
    """ec_gcm_prepare_keys into a device buffer (torch uint8 tensor allocated
    when dev_buf is None); returns it."""
    import torch
    from .eestream import SegmentCodec
    keys = [_key(k) for k in keys]
    nbytes = len(keys) * N.load().ec_gcm_key_bytes()
    if dev_buf is None:
        dev_buf = torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda")
    host = np.frombuffer(b"".join(keys), dtype=np.uint8)
    rc = N.load().ec_gcm_prepare_keys(host.ctypes.data, len(keys), SegmentCodec._addr(dev_buf),
                                      SegmentCodec._stream(stream))
    _raise(None, rc)
    return dev_buf


def seal_segments(plain, nseg: int, nblocks: int, in_block: int, dev_keys, dev_nonces, out, stream=None):
    """ec_gcm_seal_segments on device buffers: [nseg][nblocks*in_block] ->
    [nseg][nblocks*(in_block+16)]."""
    from .eestream import SegmentCodec as C
    rc = N.load().ec_gcm_seal_segments(C._addr(plain), nseg, nblocks, in_block, C._addr(dev_keys),
                                       C._addr(dev_nonces), C._addr(out), C._stream(stream))
    _raise(None, rc)


def _sized_lists(what, bufs, nblocks, outs):
    nblocks = [int(x) for x in nblocks]
    bufs, outs = list(bufs), list(outs)
    if len(bufs) != len(nblocks) or len(outs) != len(nblocks):
        raise ValueError(f"one {what}, one block count and one output per segment")
    if any(x < 0 for x in nblocks):
        raise ValueError("a block count is negative")
    from .eestream import SegmentCodec as C
    n = max(len(nblocks), 1)
    c_in = (ctypes.c_void_p * n)(*[0 if x is None else C._addr(x) for x in bufs])
    c_out = (ctypes.c_void_p * n)(*[0 if x is None else C._addr(x) for x in outs])
    return len(nblocks), c_in, (ctypes.c_size_t * n)(*nblocks), c_out


def seal_segments_sized(scheme, plains, nblocks, in_block: int, dev_keys, dev_nonces, outs, data_len=None,
                        stream=None):
    """seal_segments with a block count, key and nonce per segment
    (ec_gcm_seal_segments_sized): plains[g] is nblocks[g]*in_block bytes,
    outs[g] nblocks[g]*(in_block+16); entries are tensors, addresses or None
    (a segment of 0 blocks).  With data_len, segment g holds data_len[g] bytes
    and PadReader's padding to in_block is written behind them before the seal.
    `scheme` supplies the device and the staging.  Asynchronous on `stream`."""
    from .eestream import SegmentCodec as C
    nseg, c_in, c_nb, c_out = _sized_lists("plaintext", plains, nblocks, outs)
    c_len = None
    if data_len is not None:
        data_len = [int(x) for x in data_len]
        if len(data_len) != nseg or any(x < 0 for x in data_len):
            raise ValueError("one non-negative data length per segment")
        c_len = (ctypes.c_size_t * max(nseg, 1))(*data_len)
    rc = N.load().ec_gcm_seal_segments_sized(scheme.ctx, nseg, c_in, c_nb, c_len, int(in_block), C._addr(dev_keys),
                                             C._addr(dev_nonces), c_out, C._stream(stream))
    _raise(scheme.ctx, rc)


def open_segments_sized(scheme, ciphers, nblocks, in_block: int, dev_keys, dev_nonces, outs, dev_status,
                        stream=None):
    """ec_gcm_open_segments_sized: ciphers[g] is nblocks[g]*(in_block+16) bytes,
    outs[g] nblocks[g]*in_block; dev_status is [nseg] int32 on the device and
    dev_status[g] ends as -1 or the first failing block of segment g."""
    from .eestream import SegmentCodec as C
    nseg, c_in, c_nb, c_out = _sized_lists("ciphertext", ciphers, nblocks, outs)
    rc = N.load().ec_gcm_open_segments_sized(scheme.ctx, nseg, c_in, c_nb, int(in_block), C._addr(dev_keys),
                                             C._addr(dev_nonces), c_out, C._addr(dev_status), C._stream(stream))
    _raise(scheme.ctx, rc)


def open_ranges_sized(scheme, ciphers, first_block, nblocks, head, length, in_block: int, dev_keys, dev_nonces, outs,
                      dev_status, stream=None):
    """ec_gcm_open_ranges_sized: ciphers[g] is the nblocks[g]*(in_block+16)
    bytes of the covered blocks first_block[g].. of segment g, outs[g] the
    length[g] plaintext bytes that start head[g] bytes into the first of them;
    any alignment.  dev_status[g] ends as -1 or the smallest absolute number of
    a covered block that failed."""
    from .eestream import SegmentCodec as C
    nseg, c_in, c_nb, c_out = _sized_lists("ciphertext", ciphers, nblocks, outs)
    per = []
    for name, v in (("first block", first_block), ("head", head), ("length", length)):
        v = [int(x) for x in v]
        if len(v) != nseg or any(x < 0 for x in v):
            raise ValueError(f"one non-negative {name} per segment")
        per.append((ctypes.c_size_t * max(nseg, 1))(*v))
    rc = N.load().ec_gcm_open_ranges_sized(scheme.ctx, nseg, c_in, per[0], c_nb, per[1], per[2], int(in_block),
                                           C._addr(dev_keys), C._addr(dev_nonces), c_out, C._addr(dev_status),
                                           C._stream(stream))
    _raise(scheme.ctx, rc)


def open_segments(cipher, nseg: int, nblocks: int, in_block: int, dev_keys, dev_nonces, out, dev_status,
                  stream=None):
    """ec_gcm_open_segments; dev_status[g] = -1 or the first failing block."""
    from .eestream import SegmentCodec as C
    rc = N.load().ec_gcm_open_segments(C._addr(cipher), nseg, nblocks, in_block, C._addr(dev_keys),
                                       C._addr(dev_nonces), C._addr(out), C._addr(dev_status), C._stream(stream))
    _raise(None, rc)
