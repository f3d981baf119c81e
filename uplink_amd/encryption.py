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

  encrypt / decrypt                encryption.Encrypt / Decrypt for EncAESGCM: one whole
                                   message, aesgcm.Seal(nil, nonce[:12], data, nil) -- the
                                   inline segment (splitter.go:189, store.go:360-375),
                                   stream info and ETags (uploader.go:421,438)
  encrypt_key / decrypt_key        encryption.EncryptKey / DecryptKey: a 32-byte key
                                   sealed to 48 bytes (splitter.go:160, store.go:349)
  seal_messages / open_messages    lists of such messages, a raw key each, in one call
                                   (ec_gcm_seal_messages / ec_gcm_open_messages)

Every block is sealed or opened by the GPU (ec_gcm_*); a block whose tag
does not verify raises DecryptionFailed ("cipher: message authentication
failed", Go's crypto/cipher error) naming the block.
"""
from __future__ import annotations

import ctypes
import threading

import numpy as np

from . import _batch as B
from . import _native as N
from .eestream import _raise, pad, unpad

TAG_SIZE = 16
DEFAULT_BLOCK_SIZE = 29 * 256  # project.go:84


class DecryptionFailed(Exception):
    def __init__(self, block: int):
        super().__init__(f"cipher: message authentication failed (block {block})")
        self.block = block


class KeyDecryptionFailed(DecryptionFailed):
    """DecryptKey failed: the encrypted content key did not verify under the
    derived key (downloads.open_inline_downloads tells it from a failure of the
    data under a good content key, which is a plain DecryptionFailed)."""


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
    keys = [_key(k) for k in keys]
    nbytes = len(keys) * N.load().ec_gcm_key_bytes()
    if dev_buf is None:
        dev_buf = torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda")
    host = np.frombuffer(b"".join(keys), dtype=np.uint8)
    rc = N.load().ec_gcm_prepare_keys(host.ctypes.data, len(keys), B.addr(dev_buf), B.stream_handle(stream))
    _raise(None, rc)
    return dev_buf


def seal_segments(plain, nseg: int, nblocks: int, in_block: int, dev_keys, dev_nonces, out, stream=None):
    """ec_gcm_seal_segments on device buffers: [nseg][nblocks*in_block] ->
    [nseg][nblocks*(in_block+16)]."""
    rc = N.load().ec_gcm_seal_segments(B.addr(plain), nseg, nblocks, in_block, B.addr(dev_keys), B.addr(dev_nonces),
                                       B.addr(out), B.stream_handle(stream))
    _raise(None, rc)


def _in_out_lists(what, bufs, count, sizes, outs, per):
    """(n, inputs[], sizes[], outputs[]) of a call that takes one input, one
    size (a `count`: "block count", "length") and one output per segment or message"""
    bufs, sizes, outs = list(bufs), list(sizes), list(outs)
    n = len(sizes)
    if len(bufs) != n or len(outs) != n:
        raise ValueError(f"one {what}, one {count} and one output per {per}")
    return n, B.ptr_array(bufs), B.size_array(sizes, n, count), B.ptr_array(outs)


def seal_segments_sized(scheme, plains, nblocks, in_block: int, dev_keys, dev_nonces, outs, data_len=None,
                        stream=None):
    """seal_segments with a block count, key and nonce per segment
    (ec_gcm_seal_segments_sized): plains[g] is nblocks[g]*in_block bytes,
    outs[g] nblocks[g]*(in_block+16); entries are tensors, addresses or None
    (a segment of 0 blocks).  With data_len, segment g holds data_len[g] bytes
    and PadReader's padding to in_block is written behind them before the seal.
    `scheme` supplies the device and the staging.  Asynchronous on `stream`."""
    nseg, c_in, c_nb, c_out = _in_out_lists("plaintext", plains, "block count", nblocks, outs, "segment")
    c_len = None if data_len is None else B.size_array(data_len, nseg, "data length", one_error=True)
    rc = N.load().ec_gcm_seal_segments_sized(scheme.ctx, nseg, c_in, c_nb, c_len, int(in_block), B.addr(dev_keys),
                                             B.addr(dev_nonces), c_out, B.stream_handle(stream))
    _raise(scheme.ctx, rc)


def open_segments_sized(scheme, ciphers, nblocks, in_block: int, dev_keys, dev_nonces, outs, dev_status,
                        stream=None):
    """ec_gcm_open_segments_sized: ciphers[g] is nblocks[g]*(in_block+16) bytes,
    outs[g] nblocks[g]*in_block; dev_status is [nseg] int32 on the device and
    dev_status[g] ends as -1 or the first failing block of segment g."""
    nseg, c_in, c_nb, c_out = _in_out_lists("ciphertext", ciphers, "block count", nblocks, outs, "segment")
    rc = N.load().ec_gcm_open_segments_sized(scheme.ctx, nseg, c_in, c_nb, int(in_block), B.addr(dev_keys),
                                             B.addr(dev_nonces), c_out, B.addr(dev_status), B.stream_handle(stream))
    _raise(scheme.ctx, rc)


def open_ranges_sized(scheme, ciphers, first_block, nblocks, head, length, in_block: int, dev_keys, dev_nonces, outs,
                      dev_status, stream=None):
    """ec_gcm_open_ranges_sized: ciphers[g] is the nblocks[g]*(in_block+16)
    bytes of the covered blocks first_block[g].. of segment g, outs[g] the
    length[g] plaintext bytes that start head[g] bytes into the first of them;
    any alignment.  dev_status[g] ends as -1 or the smallest absolute number of
    a covered block that failed."""
    nseg, c_in, c_nb, c_out = _in_out_lists("ciphertext", ciphers, "block count", nblocks, outs, "segment")
    c_first, c_head, c_length = [B.size_array(v, nseg, noun, one_error=True)
                                 for noun, v in (("first block", first_block), ("head", head), ("length", length))]
    rc = N.load().ec_gcm_open_ranges_sized(scheme.ctx, nseg, c_in, c_first, c_nb, c_head, c_length, int(in_block),
                                           B.addr(dev_keys), B.addr(dev_nonces), c_out, B.addr(dev_status),
                                           B.stream_handle(stream))
    _raise(scheme.ctx, rc)


def open_segments(cipher, nseg: int, nblocks: int, in_block: int, dev_keys, dev_nonces, out, dev_status,
                  stream=None):
    """ec_gcm_open_segments; dev_status[g] = -1 or the first failing block."""
    rc = N.load().ec_gcm_open_segments(B.addr(cipher), nseg, nblocks, in_block, B.addr(dev_keys), B.addr(dev_nonces),
                                       B.addr(out), B.addr(dev_status), B.stream_handle(stream))
    _raise(None, rc)


# ---- one-shot messages, a raw key each (ec_gcm_seal_messages / ec_gcm_open_messages) ----

def seal_messages(scheme, plains, lens, dev_keys32, dev_nonces, outs, stream=None):
    """ec_gcm_seal_messages: message i is lens[i] plaintext bytes at plains[i]
    sealed under the 32 raw key bytes dev_keys32[32*i:] and the nonce
    dev_nonces[12*i:] (device memory, any alignment) to lens[i]+16 bytes,
    ciphertext || tag, at outs[i].  Entries are tensors, addresses or None (the
    plaintext of an empty message); any alignment.  No prepared keys: the GPU
    derives everything from the key bytes.  `scheme` supplies the device and
    the staging.  Asynchronous on `stream`."""
    nmsg, c_in, c_len, c_out = _in_out_lists("plaintext", plains, "length", lens, outs, "message")
    rc = N.load().ec_gcm_seal_messages(scheme.ctx, nmsg, c_in, c_len, B.addr(dev_keys32), B.addr(dev_nonces), c_out,
                                       B.stream_handle(stream))
    _raise(scheme.ctx, rc)


def open_messages(scheme, ciphers, lens, dev_keys32, dev_nonces, outs, dev_status, stream=None):
    """ec_gcm_open_messages: ciphers[i] is lens[i]+16 bytes, outs[i] lens[i]
    (lens are plaintext lengths); dev_status is [nmsg] int32 on the device and
    dev_status[i] ends as 0, or as 1 when the tag did not verify -- outs[i] is
    then lens[i] zero bytes."""
    nmsg, c_in, c_len, c_out = _in_out_lists("ciphertext", ciphers, "length", lens, outs, "message")
    rc = N.load().ec_gcm_open_messages(scheme.ctx, nmsg, c_in, c_len, B.addr(dev_keys32), B.addr(dev_nonces), c_out,
                                       B.addr(dev_status), B.stream_handle(stream))
    _raise(scheme.ctx, rc)


class _MessageScheme:
    """the context the bytes-in, bytes-out mirrors below run on (the message
    calls take only the device and a staging pool from it); made on first use"""
    _lock = threading.Lock()
    _one = None

    def __init__(self):
        self.ctx = ctypes.c_void_p()
        _raise(None, N.load().ec_create(2, 4, 16, ctypes.byref(self.ctx)))

    @classmethod
    def get(cls):
        with cls._lock:
            if cls._one is None:
                cls._one = cls()
            return cls._one


def _one_message(data: bytes, key, nonce, open_: bool):
    """one message through the GPU: the sealed bytes, or (plaintext, status)"""
    import torch
    key, nonce = _key(key), bytes(nonce)[:12]
    if len(nonce) != 12:
        raise ValueError("AES-256-GCM needs a nonce of at least 12 bytes")
    n = len(data) - TAG_SIZE if open_ else len(data)
    host = np.frombuffer(key + nonce + bytes(data), dtype=np.uint8).copy()
    dev = torch.from_numpy(host).cuda()
    out = torch.empty(max(n + (0 if open_ else TAG_SIZE), 1), dtype=torch.uint8, device=dev.device)
    sch = _MessageScheme.get()
    if not open_:
        seal_messages(sch, [dev[44:] if n else None], [n], dev, dev[32:], [out])
        return out.cpu().numpy()[:n + TAG_SIZE].tobytes()
    status = torch.empty(1, dtype=torch.int32, device=dev.device)
    open_messages(sch, [dev[44:]], [n], dev, dev[32:], [out if n else None], status)
    return out.cpu().numpy()[:n].tobytes(), int(status.cpu()[0])


def encrypt(data, key, nonce) -> bytes:
    """encryption.Encrypt(data, EncAESGCM, key, nonce): the whole of `data` as
    one GCM message under the first 12 bytes of `nonce`, ciphertext || tag, on
    the GPU.  Empty data gives empty bytes without calling the cipher: that is
    storj.io/common's rule ("don't encrypt empty slice"), stated here from
    memory -- the module is a dependency of the reference, not part of it.
    (ec_gcm_seal_messages itself treats length 0 as a message, as the GCM
    specification's test case 13 does.)"""
    data = bytes(data)
    if not data:
        return b""
    return _one_message(data, key, nonce, False)


def decrypt(cipher, key, nonce) -> bytes:
    """encryption.Decrypt(cipher, EncAESGCM, key, nonce).  Raises
    DecryptionFailed(0) when the tag does not verify, and for a cipher text
    shorter than the 16-byte tag; empty input gives empty bytes (the rule of
    encrypt, from memory as there)."""
    cipher = bytes(cipher)
    if not cipher:
        return b""
    if len(cipher) < TAG_SIZE:
        raise DecryptionFailed(0)
    plain, status = _one_message(cipher, key, nonce, True)
    if status != 0:
        raise DecryptionFailed(0)
    return plain


def encrypt_key(key_to_encrypt, key, nonce) -> bytes:
    """encryption.EncryptKey(keyToEncrypt, EncAESGCM, key, nonce): the 32-byte
    key sealed to 48 bytes (splitter.go:160)."""
    return encrypt(_key(key_to_encrypt), key, nonce)


def decrypt_key(encrypted, key, nonce) -> bytes:
    """encryption.DecryptKey(encrypted, EncAESGCM, key, nonce) (store.go:349):
    the 32-byte key, DecryptionFailed(0) when it does not verify."""
    plain = decrypt(encrypted, key, nonce)
    if len(plain) != 32:
        raise ValueError("an encrypted key is 48 bytes")
    return plain


def device_rows(rows, width: int, device=None):
    """[N, width] uint8 on the device from a device tensor of that shape or from
    N byte strings, each cut to its first `width` bytes (a storj.Nonce is 24
    bytes, AES-GCM takes 12)"""
    import torch
    if isinstance(rows, torch.Tensor):
        if rows.dtype != torch.uint8 or rows.dim() != 2 or rows.shape[1] != width or not rows.is_contiguous():
            raise ValueError(f"expected a contiguous [N, {width}] uint8 tensor")
        return rows
    rows = [bytes(r)[:width] for r in rows]
    if any(len(r) != width for r in rows):
        raise ValueError(f"expected {width} bytes per entry")
    host = np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), width).copy()
    t = torch.from_numpy(host)
    return t.to(device if device is not None else B.default_device())
