"""What the Python batch layer hands to the native library, pinned argument by
argument (uplink_amd/eestream.py SegmentCodec, encryption.py, piecehash.py,
repair.py, downloads.py).  _native.load is replaced by a recorder whose
attributes store their arguments and return EC_OK, so every ctypes array a
wrapper builds can be unpacked and compared with literals: the export's name,
the scalars, each array's entries (None as 0) and length (one slot for an
empty list), and which arguments are None.  The ValueError of every wrong
length and negative value is pinned by its text.  No device needed: addresses
are plain integers or a tiny object with data_ptr(), and the drivers run on
CPU tensors, where the recorder can even fill in a status word."""
import ctypes

import pytest

from uplink_amd import _native, downloads, eestream, encryption, piecehash, repair

CTX = 0x1234


class Recorder:
    """Stands in for the loaded library: lib.<export>(*args) is stored in
    .calls and returns EC_OK.  `returns` gives other return values by name
    (those calls are queries and are not stored, nor is ec_format_error);
    `hooks` are called with the arguments first (to write a status word)."""

    def __init__(self, returns=None, hooks=None):
        self.calls, self.returns, self.hooks = [], dict(returns or {}), dict(hooks or {})

    def __getattr__(self, name):
        def call(*args):
            if name in self.returns:
                return self.returns[name]
            if name != "ec_format_error":
                self.calls.append((name, args))
            if name in self.hooks:
                self.hooks[name](*args)
            return _native.EC_OK
        return call

    def unpacked(self):
        """[(name, [argument, ...])] with every ctypes array as a list of ints"""
        return [(name, [_ints(a) for a in args]) for name, args in self.calls]

    def only(self):
        calls = self.unpacked()
        assert len(calls) == 1, calls
        return calls[0]


def _ints(a):
    return [int(x or 0) for x in a] if isinstance(a, ctypes.Array) else a


class T:
    """the least of a tensor: something with data_ptr()"""

    def __init__(self, address):
        self.address = address

    def data_ptr(self):
        return self.address


class TorchStream:
    cuda_stream = 88


class Scheme:
    """Duck-typed ErasureScheme carrying the recorder where SegmentCodec reads it."""

    def __init__(self, lib, k=2, ess=64):
        self._lib, self.ctx, self.k, self.ess = lib, CTX, k, ess

    def erasure_share_size(self):
        return self.ess

    def required_count(self):
        return self.k

    def stripe_size(self):
        return self.k * self.ess


@pytest.fixture
def rec(monkeypatch):
    r = Recorder(returns={"ec_share_size": 64, "ec_required": 2})
    monkeypatch.setattr(_native, "load", lambda *a, **kw: r)
    return r


def raises(text):
    return pytest.raises(ValueError, match="^" + text + "$")


# ------------------------------------------------------------------ eestream.SegmentCodec
def test_encode_segments_sized(rec):
    codec = eestream.SegmentCodec(Scheme(rec))
    codec.encode_segments_sized([T(0x1000), 0x2000, None], [2, 3, 0], [0x9000, T(0xA000), None],
                                data_len=[100, 200, 0], parity_only=True, stream=77)
    assert rec.only() == ("ec_encode_segments_sized", [CTX, 3, [0x1000, 0x2000, 0], [2, 3, 0], [100, 200, 0],
                                                       [0x9000, 0xA000, 0], _native.EC_FLAG_PARITY_ONLY, 77])
    rec.calls.clear()
    codec.encode_segments_sized([0x1000, 0x2000], [2, 3], [0x9000, 0xA000], stream=TorchStream())
    assert rec.only() == ("ec_encode_segments_sized", [CTX, 2, [0x1000, 0x2000], [2, 3], None, [0x9000, 0xA000], 0, 88])
    rec.calls.clear()
    codec.encode_segments_sized([], [], [], data_len=[], stream=77)
    assert rec.only() == ("ec_encode_segments_sized", [CTX, 0, [0], [0], [0], [0], 0, 77])
    rec.calls.clear()
    one = "one segment, one stripe count and one piece buffer per segment"
    with raises(one):
        codec.encode_segments_sized([1], [1, 2], [1, 2], stream=77)
    with raises(one):
        codec.encode_segments_sized([1, 2], [1, 2], [1], stream=77)
    with raises(one):  # (the lengths win over a negative count)
        codec.encode_segments_sized([1], [1, -2], [1, 2], stream=77)
    with raises("a stripe count is negative"):
        codec.encode_segments_sized([1, 2], [1, -2], [1, 2], data_len=[1], stream=77)
    with raises("one non-negative data length per segment"):
        codec.encode_segments_sized([1, 2], [1, 2], [1, 2], data_len=[1], stream=77)
    with raises("one non-negative data length per segment"):
        codec.encode_segments_sized([1, 2], [1, 2], [1, 2], data_len=[1, -1], stream=77)
    assert rec.calls == []


@pytest.mark.parametrize("method, export", [("rebuild_segments", "ec_rebuild_segments_batched"),
                                            ("decode_segments", "ec_decode_segments_batched")])
def test_one_share_set_for_the_batch(rec, method, export):
    call = getattr(eestream.SegmentCodec(Scheme(rec)), method)
    call(iter([3, 1, 4]), iter([0x100, T(0x200), 0x300]), 5, T(0x5000), nseg=2, piece_seg_stride=64,
         out_seg_stride=128, stream=TorchStream())
    assert rec.only() == (export, [CTX, 3, [3, 1, 4], [0x100, 0x200, 0x300], 5, 2, 64, 128, 0x5000, 88])
    rec.calls.clear()
    call([], [], 5, 0x5000, stream=77)
    assert rec.only() == (export, [CTX, 0, [0], [0], 5, 1, 0, 0, 0x5000, 77])
    rec.calls.clear()
    with raises("nums and piece pointers differ in length"):
        call([1, 2], [0x100], 5, 0x5000, stream=77)
    assert rec.calls == []


SETS = [([0, 2], [0x10, T(0x20)]), ([5], [0x30]), ([], [])]


@pytest.mark.parametrize("method, export", [("rebuild_segments_sets", "ec_rebuild_segments_sets"),
                                            ("decode_segments_sets", "ec_decode_segments_sets")])
def test_share_sets(rec, method, export):
    call = getattr(eestream.SegmentCodec(Scheme(rec)), method)
    sets = [(iter(a), iter(b)) for a, b in SETS]
    call(sets, 7, [0x1000, T(0x2000), 0x3000], stream=66)
    assert rec.only() == (export, [CTX, 3, [2, 1, 0], [0, 2, 5], [0x10, 0x20, 0x30], 7, [0x1000, 0x2000, 0x3000], 66])
    rec.calls.clear()
    call([], 7, [], stream=66)
    assert rec.only() == (export, [CTX, 0, [0], [0], [0], 7, [0], 66])
    rec.calls.clear()
    with raises("one output per segment"):
        call(sets, 7, [0x1000, 0x2000], stream=66)
    with raises("one output per segment"):  # (it wins over a set's own mismatch)
        call([([1, 2], [0x10])], 7, [], stream=66)
    with raises("nums and piece pointers differ in length"):
        call([([1], [0x10]), ([1, 2], [0x10])], 7, [0x1000, 0x2000], stream=66)
    assert rec.calls == []


@pytest.mark.parametrize("method, export", [("rebuild_segments_sized", "ec_rebuild_segments_sized"),
                                            ("decode_segments_sized", "ec_decode_segments_sized")])
def test_share_sets_sized(rec, method, export):
    call = getattr(eestream.SegmentCodec(Scheme(rec)), method)
    sets = [(list(a), list(b)) for a, b in SETS]
    status = [[0, 0, 0]] if method.startswith("decode") else []
    res = call(sets, [7, 2, 0], [0x1000, T(0x2000), None], stream=66)
    assert rec.only() == (export, [CTX, 3, [2, 1, 0], [0, 2, 5], [0x10, 0x20, 0x30], [7, 2, 0], [0x1000, 0x2000, 0]] +
                          status + [66])
    assert res == ([0, 0, 0] if status else None)
    rec.calls.clear()
    res = call([], [], [], stream=66)
    assert rec.only() == (export, [CTX, 0, [0], [0], [0], [0], [0]] + ([[0]] if status else []) + [66])
    assert res == ([] if status else None)
    rec.calls.clear()
    with raises("one stripe count per segment"):  # (it wins over the outputs' count)
        call(sets, [7, 2], [0x1000], stream=66)
    with raises("a stripe count is negative"):
        call(sets, [7, -2, 0], [0x1000], stream=66)
    with raises("one output per segment"):
        call(sets, [7, 2, 0], [0x1000, None], stream=66)
    with raises("nums and piece pointers differ in length"):
        call([([1, 2], [0x10])], [7], [0x1000], stream=66)
    assert rec.calls == []


# ------------------------------------------------------------------ encryption
def test_seal_segments_sized(rec):
    es = Scheme(rec)
    encryption.seal_segments_sized(es, [T(0x1000), 0x2000, None], [2, 3, 0], 7408, T(0x700), 0x800,
                                   [0x9000, T(0xA000), None], data_len=[14000, 22000, 0], stream=77)
    assert rec.only() == ("ec_gcm_seal_segments_sized", [CTX, 3, [0x1000, 0x2000, 0], [2, 3, 0], [14000, 22000, 0], 7408,
                                                         0x700, 0x800, [0x9000, 0xA000, 0], 77])
    rec.calls.clear()
    encryption.seal_segments_sized(es, [], [], 7408, 0x700, 0x800, [], stream=TorchStream())
    assert rec.only() == ("ec_gcm_seal_segments_sized", [CTX, 0, [0], [0], None, 7408, 0x700, 0x800, [0], 88])
    rec.calls.clear()
    with raises("one plaintext, one block count and one output per segment"):
        encryption.seal_segments_sized(es, [1], [1, 2], 16, 1, 1, [1, 2], stream=77)
    with raises("one plaintext, one block count and one output per segment"):
        encryption.seal_segments_sized(es, [1, 2], [1, -2], 16, 1, 1, [1], stream=77)
    with raises("a block count is negative"):
        encryption.seal_segments_sized(es, [1, 2], [1, -2], 16, 1, 1, [1, 2], data_len=[1], stream=77)
    with raises("one non-negative data length per segment"):
        encryption.seal_segments_sized(es, [1, 2], [1, 2], 16, 1, 1, [1, 2], data_len=[1], stream=77)
    with raises("one non-negative data length per segment"):
        encryption.seal_segments_sized(es, [1, 2], [1, 2], 16, 1, 1, [1, 2], data_len=[-1, 1], stream=77)
    assert rec.calls == []


def test_open_segments_sized(rec):
    es = Scheme(rec)
    encryption.open_segments_sized(es, [T(0x1000), None], [2, 0], 7408, 0x700, T(0x800), [T(0x9000), None], T(0x50),
                                   stream=77)
    assert rec.only() == ("ec_gcm_open_segments_sized", [CTX, 2, [0x1000, 0], [2, 0], 7408, 0x700, 0x800, [0x9000, 0],
                                                         0x50, 77])
    rec.calls.clear()
    encryption.open_segments_sized(es, [], [], 7408, 0x700, 0x800, [], 0x50, stream=77)
    assert rec.only() == ("ec_gcm_open_segments_sized", [CTX, 0, [0], [0], 7408, 0x700, 0x800, [0], 0x50, 77])
    rec.calls.clear()
    with raises("one ciphertext, one block count and one output per segment"):
        encryption.open_segments_sized(es, [1, 2], [1, 2], 16, 1, 1, [1], 1, stream=77)
    with raises("a block count is negative"):
        encryption.open_segments_sized(es, [1, 2], [-1, 2], 16, 1, 1, [1, 2], 1, stream=77)
    assert rec.calls == []


def test_open_ranges_sized(rec):
    es = Scheme(rec)
    encryption.open_ranges_sized(es, [T(0x1000), 0x2000, None], [4, 0, 9], [2, 3, 0], [17, 0, 5], [9000, 22000, 0], 7408,
                                 0x700, 0x800, [0x9000, T(0xA000), None], 0x50, stream=77)
    assert rec.only() == ("ec_gcm_open_ranges_sized", [CTX, 3, [0x1000, 0x2000, 0], [4, 0, 9], [2, 3, 0], [17, 0, 5],
                                                       [9000, 22000, 0], 7408, 0x700, 0x800, [0x9000, 0xA000, 0], 0x50,
                                                       77])
    rec.calls.clear()
    encryption.open_ranges_sized(es, [], [], [], [], [], 7408, 0x700, 0x800, [], 0x50, stream=77)
    assert rec.only() == ("ec_gcm_open_ranges_sized", [CTX, 0, [0], [0], [0], [0], [0], 7408, 0x700, 0x800, [0], 0x50,
                                                       77])
    rec.calls.clear()
    with raises("one ciphertext, one block count and one output per segment"):
        encryption.open_ranges_sized(es, [1], [0], [1, 2], [0], [1], 16, 1, 1, [1], 1, stream=77)
    with raises("a block count is negative"):  # (it wins over the arrays that follow)
        encryption.open_ranges_sized(es, [1], [], [-1], [0], [1], 16, 1, 1, [1], 1, stream=77)
    for bad in ([], [-1]):
        with raises("one non-negative first block per segment"):
            encryption.open_ranges_sized(es, [1], bad, [1], bad, bad, 16, 1, 1, [1], 1, stream=77)
        with raises("one non-negative head per segment"):
            encryption.open_ranges_sized(es, [1], [0], [1], bad, bad, 16, 1, 1, [1], 1, stream=77)
        with raises("one non-negative length per segment"):
            encryption.open_ranges_sized(es, [1], [0], [1], [0], bad, 16, 1, 1, [1], 1, stream=77)
    assert rec.calls == []


def test_seal_and_open_messages(rec):
    es = Scheme(rec)
    encryption.seal_messages(es, [T(0x1000), 0x2000, None], [5, 4096, 0], T(0x700), 0x800, [0x9000, T(0xA000), 0xB000],
                             stream=77)
    assert rec.only() == ("ec_gcm_seal_messages", [CTX, 3, [0x1000, 0x2000, 0], [5, 4096, 0], 0x700, 0x800,
                                                   [0x9000, 0xA000, 0xB000], 77])
    rec.calls.clear()
    encryption.open_messages(es, [T(0x1000), 0x2000], [5, 0], 0x700, T(0x800), [0x9000, None], T(0x50),
                             stream=TorchStream())
    assert rec.only() == ("ec_gcm_open_messages", [CTX, 2, [0x1000, 0x2000], [5, 0], 0x700, 0x800, [0x9000, 0], 0x50, 88])
    rec.calls.clear()
    encryption.seal_messages(es, [], [], 0x700, 0x800, [], stream=77)
    encryption.open_messages(es, [], [], 0x700, 0x800, [], 0x50, stream=77)
    assert rec.unpacked() == [("ec_gcm_seal_messages", [CTX, 0, [0], [0], 0x700, 0x800, [0], 77]),
                              ("ec_gcm_open_messages", [CTX, 0, [0], [0], 0x700, 0x800, [0], 0x50, 77])]
    rec.calls.clear()
    with raises("one plaintext, one length and one output per message"):
        encryption.seal_messages(es, [1], [1, 2], 1, 1, [1, 2], stream=77)
    with raises("one plaintext, one length and one output per message"):
        encryption.seal_messages(es, [1, 2], [1, -2], 1, 1, [1], stream=77)
    with raises("a length is negative"):
        encryption.seal_messages(es, [1, 2], [1, -2], 1, 1, [1, 2], stream=77)
    with raises("one ciphertext, one length and one output per message"):
        encryption.open_messages(es, [1, 2], [1], 1, 1, [1, 2], 1, stream=77)
    with raises("a length is negative"):
        encryption.open_messages(es, [1], [-1], 1, 1, [1], 1, stream=77)
    assert rec.calls == []


# ------------------------------------------------------------------ piecehash
@pytest.mark.parametrize("algo, export", [(piecehash.PieceHashAlgorithm.BLAKE3, "ec_hash_segments_sized"),
                                          (piecehash.PieceHashAlgorithm.SHA256, "ec_sha256_segments_sized")])
def test_hash_segments_sized(rec, algo, export):
    es = Scheme(rec)
    piecehash.hash_segments_sized(es, [T(0x1000), 0x2000, None], [2, 3, 0], [0x9000, T(0xA000), None], T(0x60),
                                  parity_only=True, stream=77, algo=algo)
    assert rec.only() == (export, [CTX, 3, [0x1000, 0x2000, 0], [2, 3, 0], [0x9000, 0xA000, 0],
                                   _native.EC_FLAG_PARITY_ONLY, 0x60, 77])
    rec.calls.clear()
    # without segs, and on a raw context
    piecehash.hash_segments_sized(CTX, None, [2, 3], [0x9000, T(0xA000)], 0x60, stream=TorchStream(), algo=int(algo))
    assert rec.only() == (export, [CTX, 2, None, [2, 3], [0x9000, 0xA000], 0, 0x60, 88])
    rec.calls.clear()
    piecehash.hash_segments_sized(es, [], [], [], 0x60, stream=77, algo=algo)
    piecehash.hash_segments_sized(es, None, [], [], 0x60, stream=77, algo=algo)
    assert rec.unpacked() == [(export, [CTX, 0, [0], [0], [0], 0, 0x60, 77]),
                              (export, [CTX, 0, None, [0], [0], 0, 0x60, 77])]
    rec.calls.clear()
    one = "one segment, one stripe count and one piece buffer per segment"
    with raises(one):
        piecehash.hash_segments_sized(es, [1, 2], [1, 2], [1], 1, stream=77, algo=algo)
    with raises(one):
        piecehash.hash_segments_sized(es, [1], [1, -2], [1, 2], 1, stream=77, algo=algo)
    with raises(one):
        piecehash.hash_segments_sized(es, None, [1], [1, 2], 1, stream=77, algo=algo)
    with raises("a stripe count is negative"):  # (it wins over parity_only without segments)
        piecehash.hash_segments_sized(es, None, [1, -2], [1, 2], 1, parity_only=True, stream=77, algo=algo)
    with raises("parity_only reads the data pieces from the segments"):
        piecehash.hash_segments_sized(es, None, [1, 2], [1, 2], 1, parity_only=True, stream=77, algo=algo)
    with pytest.raises(ValueError):
        piecehash.hash_segments_sized(es, [1], [1], [1], 1, stream=77, algo=7)
    assert rec.calls == []


@pytest.mark.parametrize("algo, export", [(piecehash.PieceHashAlgorithm.BLAKE3, "ec_blake3_pieces_list"),
                                          (piecehash.PieceHashAlgorithm.SHA256, "ec_sha256_pieces_list")])
def test_hash_pieces_list(rec, algo, export):
    torch = pytest.importorskip("torch")
    pieces = [torch.zeros(96, dtype=torch.uint8), torch.zeros(0, dtype=torch.uint8), torch.zeros(5, dtype=torch.uint8)]
    hashes = torch.zeros((3, 32), dtype=torch.uint8)
    assert piecehash.hash_pieces_list(Scheme(rec), pieces, hashes=hashes, stream=77, algo=algo) is hashes
    assert rec.only() == (export, [CTX, 3, [pieces[0].data_ptr(), 0, pieces[2].data_ptr()], [96, 0, 5],
                                   hashes.data_ptr(), 77])
    rec.calls.clear()
    # the hashes allocated next to the pieces; none at all for no pieces
    got = piecehash.hash_pieces_list(CTX, pieces[:1], stream=77, algo=algo)
    assert got.shape == (1, 32) and got.dtype == torch.uint8 and got.device == pieces[0].device
    assert rec.only() == (export, [CTX, 1, [pieces[0].data_ptr()], [96], got.data_ptr(), 77])
    rec.calls.clear()
    piecehash.hash_pieces_list(CTX, [], hashes=hashes[:0], stream=77, algo=algo)
    assert rec.only() == (export, [CTX, 0, [0], [0], None, 77])
    rec.calls.clear()
    with raises("a piece is a contiguous uint8 tensor"):
        piecehash.hash_pieces_list(CTX, [torch.zeros(4, dtype=torch.int32)], hashes=hashes, stream=77, algo=algo)
    with raises("hashes is a contiguous uint8 tensor of npieces\\*32 bytes"):
        piecehash.hash_pieces_list(CTX, pieces, hashes=hashes[:2], stream=77, algo=algo)
    assert rec.calls == []


# ------------------------------------------------------------------ repair: the raw calls
SEGMENTS = [([0, 2, 5], [0x10, T(0x20), 0x30], [1, 3]), ([4, 1], [T(0x40), 0x50], [0]), ([7], [0x60], [])]


def _segments():
    return [(iter(a), iter(b), iter(c)) for a, b, c in SEGMENTS]


def test_repair_call(rec):
    rc = repair.repair_call(CTX, _segments(), [0x1000, T(0x2000), 0x3000], 6, _native.EC_FLAG_CHECK_SHARES, T(0x50), 77)
    assert rc == _native.EC_OK
    assert rec.only() == ("ec_repair_segments_sets", [CTX, 3, [3, 2, 1], [0, 2, 5, 4, 1, 7],
                                                      [0x10, 0x20, 0x30, 0x40, 0x50, 0x60], [2, 1, 0], [1, 3, 0],
                                                      [0x1000, 0x2000, 0x3000], 6, _native.EC_FLAG_CHECK_SHARES, 0x50,
                                                      77])
    rec.calls.clear()
    repair.repair_call(CTX, [], [], 6, stream=TorchStream())
    assert rec.only() == ("ec_repair_segments_sets", [CTX, 0, [0], [0], [0], [0], [0], [0], 6, 0, None, 88])
    rec.calls.clear()
    with raises("nums and pieces differ in length"):
        repair.repair_call(CTX, [([1, 2], [16], [3])], [32], 1, stream=77)
    with raises("nums and pieces differ in length"):  # (it wins over the outputs' count)
        repair.repair_call(CTX, [([1, 2], [16], [3])], [], 1, stream=77)
    with raises("one output per target"):
        repair.repair_call(CTX, [([1], [16], [3, 4])], [32], 1, stream=77)
    assert rec.calls == []


def test_repair_call_sized(rec):
    rc = repair.repair_call_sized(CTX, _segments(), [0x1000, T(0x2000), 0x3000], [6, 1, 0], 0, None, TorchStream())
    assert rc == _native.EC_OK
    assert rec.only() == ("ec_repair_segments_sized", [CTX, 3, [3, 2, 1], [0, 2, 5, 4, 1, 7],
                                                       [0x10, 0x20, 0x30, 0x40, 0x50, 0x60], [2, 1, 0], [1, 3, 0],
                                                       [0x1000, 0x2000, 0x3000], [6, 1, 0], 0, None, 88])
    rec.calls.clear()
    repair.repair_call_sized(CTX, [], [], [], _native.EC_FLAG_CHECK_SHARES, 0x50, 77)
    assert rec.only() == ("ec_repair_segments_sized", [CTX, 0, [0], [0], [0], [0], [0], [0], [0],
                                                       _native.EC_FLAG_CHECK_SHARES, 0x50, 77])
    rec.calls.clear()
    with raises("nums and pieces differ in length"):
        repair.repair_call_sized(CTX, [([1, 2], [16], [3])], [32], [1], stream=77)
    with raises("one output per target"):  # (it wins over the stripe counts)
        repair.repair_call_sized(CTX, [([1], [16], [3, 4])], [32], [1, 2], stream=77)
    with raises("one stripe count per segment"):
        repair.repair_call_sized(CTX, [([1], [16], [3])], [32], [1, 2], stream=77)
    with pytest.raises(ValueError):  # (worded unlike the other entry points: only its type is pinned)
        repair.repair_call_sized(CTX, [([1], [16], [3])], [32], [-1], stream=77)
    assert rec.calls == []


# ------------------------------------------------------------------ repair: the drivers, on CPU tensors
# Without a stream argument nothing in them needs torch.cuda: the outputs lie where the pieces
# lie, and a status word in host memory is one the recorder can write.  The stream that reaches
# the library is then the current one where there is a device and None where there is none, so
# it is left out of the comparisons.

def _piece(nbytes, fill=0):
    import torch
    return torch.full((nbytes,), fill, dtype=torch.uint8)


def _no_stream(calls):
    return [(name, args[:-1]) for name, args in calls]


def test_uniform_repair_takes_one_piece_length(rec):
    pytest.importorskip("torch")
    es = Scheme(rec)
    mixed = [([0, 1], [_piece(128), _piece(128)], [2]), ([0, 1], [_piece(64), _piece(64)], [3])]
    with pytest.raises(eestream.InfectiousError) as ei:
        repair.repair_segments(es, mixed)
    assert ei.value.code == _native.EC_ERR_SHARE_SIZE
    with pytest.raises(eestream.InfectiousError) as ei:  # no multiple of the share size
        repair.repair_segments(es, [([0, 1], [_piece(96), _piece(96)], [2])])
    assert ei.value.code == _native.EC_ERR_INVALID_ARG
    assert rec.calls == []
    # the sized form takes the same batch to the engine, a stripe count per segment
    outs = repair.repair_segments_sized(es, mixed)
    assert [tuple(o.shape) for o in outs] == [(1, 128), (1, 64)]
    (p0, p1), (p2, p3) = mixed[0][1], mixed[1][1]
    assert _no_stream(rec.unpacked()) == [("ec_repair_segments_sized", [
        CTX, 2, [2, 2], [0, 1, 0, 1], [p0.data_ptr(), p1.data_ptr(), p2.data_ptr(), p3.data_ptr()], [1, 1], [2, 3],
        [outs[0].data_ptr(), outs[1].data_ptr()], [2, 1], 0, None])]


def test_uniform_repair_reaches_the_engine(rec):
    pytest.importorskip("torch")
    segs = [([0, 1, 2], [_piece(192), _piece(192), _piece(192)], [3, 4]), ([5, 1], [_piece(192), _piece(192)], [])]
    outs = repair.repair_segments(CTX, segs)
    assert [tuple(o.shape) for o in outs] == [(2, 192), (0, 192)]
    assert _no_stream(rec.unpacked()) == [("ec_repair_segments_sets", [
        CTX, 2, [3, 2], [0, 1, 2, 5, 1], [p.data_ptr() for _, ps, _ in segs for p in ps], [2, 0], [3, 4],
        [outs[0][0].data_ptr(), outs[0][1].data_ptr()], 3, 0, None])]


@pytest.mark.parametrize("call", [repair.repair_segments, repair.repair_segments_sized])
def test_nothing_to_repair(rec, call):
    pytest.importorskip("torch")
    for batch in ([], [([], [], [])], [([], [], []), ([], [], [])]):
        assert call(Scheme(rec), batch) == []
        assert call(CTX, batch, hash_pieces=True) == ([], [])
        assert call(CTX, batch, check=True, hash_pieces=True) == ([], [])
    assert rec.calls == []


@pytest.mark.parametrize("sized", [False, True])
def test_flagged_segments_are_decoded_and_repaired_again(monkeypatch, sized):
    """The check protocol end to end, the engine played by the recorder: the
    first repair flags segment 1 of three, that segment alone goes through
    ec_decode_segments with its own stripe count and is repaired again, and the
    hashes of every regenerated row are taken in one list call."""
    torch = pytest.importorskip("torch")
    flagged = [[0, 1, 0], [0]]

    def set_status(*args):
        words = flagged.pop(0)
        ctypes.memmove(args[10], (ctypes.c_int32 * len(words))(*words), 4 * len(words))

    export = "ec_repair_segments_sized" if sized else "ec_repair_segments_sets"
    rec = Recorder(returns={"ec_share_size": 64, "ec_required": 2}, hooks={export: set_status})
    monkeypatch.setattr(_native, "load", lambda *a, **kw: rec)
    lens = [128, 64, 192] if sized else [128, 128, 128]
    segs = [([0, 1, 2], [_piece(n), _piece(n), _piece(n)], [3, 4]) for n in lens]
    outs, hashes = (repair.repair_segments_sized if sized else repair.repair_segments)(
        CTX, segs, check=True, hash_pieces=True, hash_algo=piecehash.PieceHashAlgorithm.SHA256)
    assert [tuple(o.shape) for o in outs] == [(2, n) for n in lens]
    assert [tuple(h.shape) for h in hashes] == [(2, 32)] * 3
    rows = [o[i].data_ptr() for o in outs for i in range(2)]
    ptrs = [[p.data_ptr() for p in ps] for _, ps, _ in segs]
    stripes = [n // 64 for n in lens]
    calls = _no_stream(rec.unpacked())
    assert [name for name, _ in calls] == [export, "ec_decode_segments", export, "ec_sha256_pieces_list"]
    status = calls[0][1][10]
    assert calls[0][1] == [CTX, 3, [3, 3, 3], [0, 1, 2] * 3, ptrs[0] + ptrs[1] + ptrs[2], [2, 2, 2], [3, 4] * 3, rows,
                           stripes if sized else 2, _native.EC_FLAG_CHECK_SHARES, status]
    scratch = calls[1][1][5]
    assert calls[1][1] == [CTX, 3, [0, 1, 2], ptrs[1], stripes[1], scratch]
    again = calls[2][1][10]
    assert calls[2][1] == [CTX, 1, [3], [0, 1, 2], ptrs[1], [2], [3, 4], rows[2:4], [stripes[1]] if sized else 2,
                           _native.EC_FLAG_CHECK_SHARES, again]
    assert status and again and scratch and len({status, again, scratch}) == 3
    assert calls[3][1] == [CTX, 6, rows, [n for n in lens for _ in range(2)], hashes[0].data_ptr()]
    assert [h.data_ptr() - hashes[0].data_ptr() for h in hashes] == [0, 64, 128]
    # a segment still flagged after the correction: not expected of codewords, TooManyErrors
    flagged[:] = [[1, 0, 0], [1]]
    with pytest.raises(eestream.TooManyErrors):
        (repair.repair_segments_sized if sized else repair.repair_segments)(CTX, segs, check=True)


# ------------------------------------------------------------------ downloads: the decode drivers
@pytest.mark.parametrize("error_detection, export", [(False, "ec_rebuild_segments_sized"),
                                                     (True, "ec_decode_segments_sized")])
def test_decode_downloads_passes_its_geometries(rec, error_detection, export):
    pytest.importorskip("torch")
    es = Scheme(rec)  # stripes of 128 bytes, pieces of 64 per stripe
    sizes = [300, 128, 0, 1]
    assert [downloads.segment_geometry(s, es) for s in sizes] == [(384, 192, 3), (128, 64, 1), (0, 0, 0), (128, 64, 1)]
    batch = [(300, {4: _piece(192), 0: _piece(192)}), (128, {1: _piece(64), 2: _piece(64)}), (0, {}),
             (1, {3: _piece(64), 0: _piece(64)})]
    res = downloads.decode_downloads(es, batch, error_detection=error_detection, collect_errors=error_detection)
    outs, errors = res if error_detection else (res, None)
    assert [o.numel() for o in outs] == sizes
    assert errors is None or errors == [None] * 4
    ptrs = [p.data_ptr() for _, ps in batch for p in ps.values()]
    name, args = _no_stream(rec.unpacked())[0]
    assert len(rec.calls) == 1 and name == export
    assert args[:7] == [CTX, 4, [2, 2, 0, 2], [4, 0, 1, 2, 3, 0], ptrs, [3, 1, 0, 1],
                        [outs[0].data_ptr(), outs[1].data_ptr(), 0, outs[3].data_ptr()]]
    assert args[7:] == ([[0, 0, 0, 0]] if error_detection else [])
    rec.calls.clear()
    # a piece of another length than the download's geometry gives: before any call
    with pytest.raises(eestream.InfectiousError) as ei:
        downloads.decode_downloads(es, [batch[1], (300, {4: _piece(192), 0: _piece(128)})],
                                   error_detection=error_detection)
    assert ei.value.code == _native.EC_ERR_SHARE_SIZE
    assert rec.calls == []


@pytest.mark.parametrize("error_detection, export", [(False, "ec_rebuild_segments_sized"),
                                                     (True, "ec_decode_segments_sized")])
def test_decode_ranges_passes_its_geometries(rec, error_detection, export):
    pytest.importorskip("torch")
    es = Scheme(rec)
    # blocks of 48 bytes (32 of plaintext): bytes [40, 110) of 1000 lie in blocks 1..3, encrypted bytes
    # [48, 192), stripes 0..1; a range of no bytes covers nothing
    geos = [downloads.range_geometry(1000, 40, 70, es, block_size=48),
            downloads.range_geometry(1000, 600, 0, es, block_size=48),
            downloads.range_geometry(5000, 4000, 33, es, block_size=48)]
    assert [(g.first_block, g.nblocks, g.first_stripe, g.nstripes, g.skip, g.enc_length, g.piece_length)
            for g in geos] == [(1, 3, 0, 2, 48, 144, 128), (18, 0, 6, 0, 96, 0, 0), (125, 2, 46, 2, 112, 96, 128)]
    batch = [(geos[0], {1: _piece(128), 0: _piece(128)}), (geos[1], {}), (geos[2], {2: _piece(128), 5: _piece(128)})]
    res = downloads.decode_ranges(es, batch, error_detection=error_detection, collect_errors=error_detection)
    encs, errors = res if error_detection else (res, None)
    assert [e.numel() for e in encs] == [144, 0, 96]
    assert errors is None or errors == [None] * 3
    ptrs = [p.data_ptr() for _, ps in batch for p in ps.values()]
    name, args = _no_stream(rec.unpacked())[0]
    assert len(rec.calls) == 1 and name == export
    # (the outputs are the whole decoded stripes; what comes back is the view at `skip` into them)
    assert args[:7] == [CTX, 3, [2, 0, 2], [1, 0, 2, 5], ptrs, [2, 0, 2],
                        [encs[0].data_ptr() - 48, 0, encs[2].data_ptr() - 112]]
    assert args[7:] == ([[0, 0, 0]] if error_detection else [])
    rec.calls.clear()
    with pytest.raises(eestream.InfectiousError) as ei:
        downloads.decode_ranges(es, [batch[0], (geos[2], {2: _piece(128), 5: _piece(192)})],
                                error_detection=error_detection)
    assert ei.value.code == _native.EC_ERR_SHARE_SIZE
    assert rec.calls == []
