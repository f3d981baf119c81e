"""Decode (infectious' Correct + Rebuild) at the edges of its correction capacity,
through every entry point: ec_decode, ec_decode_segments,
ec_decode_segments_batched and ec_decode_segments_sets.

One table of cases (CASES): a geometry, a share set that always holds share 0
and share n-1 and is handed to the calls in a shuffled order, an error pattern
laid over the oracle-encoded pieces, and the outcome.  Within the capacity
e = (ns - k) // 2 the answer is the codeword that was encoded, whatever the
decoder, so every `ok` case has ground truth of its own.  The CPU tests prove
the table (by counting errors per column, and through the oracle's per-column
Berlekamp-Welch); the GPU tests run every row through the four calls and
compare the output, the pieces corrected in place, and every byte around them.

The patterns (share = position in the sorted set, dim = k + 2e):
  A      rotating: column c is bad in the shares (c*e + t) mod ns, t < e
  B      e whole bad pieces, among them share 0 and the last (B-last: e = 1, the last)
  C      e-1 whole bad pieces plus one more error in each of 300 columns, spread
         over the other shares, off the 64 evenly spaced columns
  D / E  one share bad in exactly 256 / 257 columns (E: one of them with a
         second error in share 0 when e >= 2)
  F      only column 0 (share 0) and the last column (the last share) bad
  G-1    odd surplus: the last share, which the Berlekamp-Welch system leaves
         out, wholly bad;  G-2: that on top of A over the first dim shares
  H      two pieces bad in disjoint halves of the columns
  X1     rotating, e+1 per column            -> TooManyErrors
  X2     e+1 whole bad pieces                -> TooManyErrors
  X3     k+1 shares, a single error          -> NotEnoughShares
  X4     e+1 pieces, each bad in a stretch of columns of its own (one error a
         column: correctable there), and all of them bad in column 1, which lies
         between the evenly spaced columns a decoder would sample to find bad
         pieces                              -> TooManyErrors
After an error return only the bytes around the set's pieces and the outputs are
checked: what Decode leaves in them beyond its capacity is not pinned."""
import ctypes
import zlib
from dataclasses import dataclass

import numpy as np
import pytest

GUARD = 64
PIECE_FILL, OUT_FILL = 0xEE, 0xCD

# name: (k, n, ess, stripes, surpluses)
GEOMETRIES = {
    "G1": (29, 80, 256, 17, (2, 8, 9, 20)),  # production code; 4352 columns: more than 2 x 2048, no multiple of it
    "G2": (4, 10, 16, 257, (4, 5, 6)),       # 4112 columns: no multiple of 256
    "G3": (3, 7, 100, 41, (3, 4)),           # ess % 16 != 0
    "G4": (2, 4, 1024, 4, (2,)),             # all 4 shares
    "G5": (1, 3, 16, 130, (2,)),             # k = 1, all 3 shares
    "G6": (20, 60, 4096, 1, (12,)),          # one stripe of one wide share
}
RC = {"ok": 0, "TooManyErrors": -7, "NotEnoughShares": -6}
ORACLE_CODE = {"TooManyErrors": -13, "NotEnoughShares": -10}


@dataclass(frozen=True)
class Case:
    geo: str
    surplus: int
    pat: str
    expect: str

    @property
    def id(self):
        return f"{self.geo}-k+{self.surplus}-{self.pat}"

    @property
    def dims(self):
        k, n, ess, stripes, _ = GEOMETRIES[self.geo]
        return k, n, ess, stripes, stripes * ess

    @property
    def ns(self):
        return self.dims[0] + self.surplus

    @property
    def e(self):
        return self.surplus // 2

    @property
    def dim(self):
        return self.dims[0] + 2 * self.e

    def rng(self, what):
        return np.random.default_rng(zlib.crc32(f"{self.id}/{what}".encode()))

    def nums(self):
        """the share set, sorted: share 0, share n-1 and a seeded choice of the others"""
        k, n = self.dims[:2]
        rng = np.random.default_rng(zlib.crc32(f"{self.geo}/{self.surplus}".encode()))
        mid = sorted(int(x) for x in rng.permutation(np.arange(1, n - 1))[:self.ns - 2])
        return [0] + mid + [n - 1]

    def order(self):
        """the order the calls are given the set in: positions into nums()"""
        return [int(x) for x in self.rng("order").permutation(self.ns)]

    def mask(self):
        """[ns, plen] bool: which byte of which share (sorted) is wrong"""
        plen, ns, e, dim = self.dims[4], self.ns, self.e, self.dim
        rng = self.rng("mask")
        m = np.zeros((ns, plen), dtype=bool)
        cols = np.arange(plen)
        others = lambda taken, count: [int(x) for x in rng.permutation([i for i in range(ns) if i not in taken])[:count]]
        pat = self.pat
        if pat in ("A", "X1", "G-2"):
            per, mod = (e + 1, ns) if pat == "X1" else (e, dim if pat == "G-2" else ns)
            for t in range(per):
                m[(cols * per + t) % mod, cols] = True
            if pat == "G-2":
                m[ns - 1] = True
        elif pat in ("B", "X2"):
            count = e + 1 if pat == "X2" else e
            bad = [0, ns - 1][:count]
            m[bad + others(bad, count - len(bad))] = True
        elif pat == "B-last" or pat == "G-1":
            m[ns - 1] = True
        elif pat == "C":
            bad = [0] + others([0], e - 2)
            m[bad] = True
            sampled = {i * plen // 64 for i in range(64)}
            free = np.array([c for c in range(plen) if c not in sampled])
            where = rng.permutation(free)[:300]
            rest = np.array([i for i in range(ns) if i not in bad])
            m[rest[rng.integers(0, len(rest), 300)], where] = True
        elif pat in ("D", "E"):
            where = np.sort(rng.permutation(plen)[:256 if pat == "D" else 257])
            m[1 if pat == "D" else ns // 2, where] = True
            if pat == "E" and e >= 2:
                m[0, where[2]] = True
        elif pat == "F":
            m[0, 0] = m[ns - 1, plen - 1] = True
        elif pat == "H":
            m[0, :plen // 2] = True
            m[dim - 1, plen // 2:] = True
        elif pat == "X3":
            m[0, plen // 2] = True
        elif pat == "X4":
            bad = [0, ns - 1] + others([0, ns - 1], e - 1)
            for j, i in enumerate(bad):
                m[i, j * plen // len(bad):(j + 1) * plen // len(bad)] = True
            m[bad, 1] = True
        else:
            raise AssertionError(pat)
        return m

    def corrupt(self, ref_rows):
        """ref_rows [ns, plen]: the set's encoded pieces, sorted -> what is received.
        XOR values: 0x01, 0x80 and seeded others; every seventh error sets the
        received byte to 0 instead."""
        at = np.nonzero(self.mask())
        was = ref_rows[at]
        x = self.rng("xor").integers(1, 256, len(was), dtype=np.uint8)
        x[0::7], x[1::7] = 0x01, 0x80
        x[2::7] = np.where(was[2::7] != 0, was[2::7], 0x01)
        recv = ref_rows.copy()
        recv[at] = was ^ x
        return recv


def _cases():
    out = []
    for geo, (k, n, ess, stripes, surpluses) in GEOMETRIES.items():
        for s in surpluses:
            e, odd = s // 2, s % 2 == 1
            pats = ["A", "B"] + (["B-last"] if e == 1 else []) + (["C"] if e >= 2 else []) + ["D", "E", "F"]
            pats += (["G-1", "G-2"] if odd else []) + (["H"] if e >= 2 else [])
            out += [Case(geo, s, p, "ok") for p in pats]
            if not odd:
                out += [Case(geo, s, p, "TooManyErrors") for p in ("X1", "X2", "X4")]
        out.append(Case(geo, 1, "X3", "NotEnoughShares"))
    return out


CASES = _cases()
OK_CASES = [c for c in CASES if c.expect == "ok"]
X_CASES = [c for c in CASES if c.expect != "ok"]
ids = lambda cases: [c.id for c in cases]

_geo_cache = {}


def geometry(oracle, geo):
    """three seeded segments of the geometry and their pieces by the oracle: (segs [3][k*plen], refs [3, n, plen])"""
    if geo not in _geo_cache:
        k, n, ess, stripes, _ = GEOMETRIES[geo]
        rng = np.random.default_rng(zlib.crc32(geo.encode()))
        f = oracle.FEC(k, n)
        segs = [rng.integers(0, 256, stripes * k * ess, dtype=np.uint8) for _ in range(3)]
        refs = np.stack([f.encode_segment(s, ess, threads=4) for s in segs])
        for a in segs + [refs]:
            a.setflags(write=False)
        _geo_cache[geo] = (segs, refs)
    return _geo_cache[geo]


def received(oracle, case, data=1):
    """the case laid over segment `data` of its geometry: rows in the order of case.nums()"""
    _, refs = geometry(oracle, case.geo)
    return case.corrupt(refs[data][case.nums()])


# ---- the table itself, on the CPU ---------------------------------------------------

def test_table_is_complete():
    """every geometry, surplus and pattern the table is meant to hold"""
    have = {(c.geo, c.surplus, c.pat) for c in CASES}
    assert len(have) == len(CASES)
    for geo, (k, n, ess, stripes, surpluses) in GEOMETRIES.items():
        for s in surpluses:
            want = {"A", "B", "D", "E", "F"}
            want |= {"C", "H"} if s // 2 >= 2 else set()
            want |= {"G-1", "G-2"} if s % 2 else {"X1", "X2"}
            assert want <= {p for g, su, p in have if (g, su) == (geo, s)}, (geo, s)
        assert (geo, 1, "X3") in have
    plen = {geo: g[2] * g[3] for geo, g in GEOMETRIES.items()}
    assert plen["G1"] > 2 * 2048 and plen["G1"] % 2048 and plen["G2"] % 256 and GEOMETRIES["G3"][2] % 16
    assert all(p > 2048 for p in plen.values())  # pattern A: more columns than the kernel has workgroups
    for c in CASES:
        nums = c.nums()
        assert nums == sorted(set(nums)) and len(nums) == c.ns and nums[0] == 0 and nums[-1] == c.dims[1] - 1
        assert sorted(c.order()) == list(range(c.ns))
    assert any(c.order() != list(range(c.ns)) for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=ids(CASES))
def test_table_by_counting(case):
    """Without any decoder: an ok case has at most e errors in every column among
    the first dim sorted shares (the ones Berlekamp-Welch solves on); an X case
    has more in some column.  And the pattern is the one its name says."""
    m = case.mask()
    k, n, ess, stripes, plen = case.dims
    e, ns = case.e, case.ns
    per_col = m[:case.dim].sum(axis=0)
    if case.expect == "ok":
        assert per_col.max() <= e, int(per_col.argmax())
    else:
        assert per_col.max() > e
    whole = [i for i in range(ns) if m[i].all()]
    flagged = int(m.any(axis=0).sum())
    pat = case.pat
    if pat in ("A", "X1"):
        assert (m.sum(axis=0) == (e if pat == "A" else e + 1)).all() and m.any(axis=1).all() and not m[0].all()
        assert plen > 2048
    elif pat in ("B", "X2", "B-last"):
        assert len(whole) == (e + 1 if pat == "X2" else e) and int(m.sum()) == len(whole) * plen
        assert whole[:1] == [0] if pat == "B" or pat == "X2" else whole == [ns - 1]
        assert ns - 1 in whole or (pat == "B" and e == 1)
    elif pat == "C":
        assert len(whole) == e - 1 and int((m.sum(axis=0) == e).sum()) == 300 and m.sum(axis=0).max() == e
    elif pat in ("D", "E"):
        assert flagged == (256 if pat == "D" else 257)
        assert int(m.sum()) == flagged + (1 if pat == "E" and e >= 2 else 0)
    elif pat == "F":
        assert int(m.sum()) == 2 and m[:, 0].any() and m[:, plen - 1].any()
    elif pat == "G-1":
        assert whole == [ns - 1] and int(m.sum()) == plen and case.dim == ns - 1
    elif pat == "G-2":
        assert whole == [ns - 1] and (m.sum(axis=0) == e + 1).all() and m[:case.dim].any(axis=1).all()
    elif pat == "H":
        assert not whole and (m.sum(axis=0) == 1).all() and int(m.any(axis=1).sum()) == 2
    elif pat == "X3":
        assert e == 0 and int(m.sum()) == 1
    elif pat == "X4":
        assert not whole and int(m.any(axis=1).sum()) == e + 1 and int((m.sum(axis=0) > 1).sum()) == 1
        assert (m.sum(axis=0)[[i * plen // 64 for i in range(64)]] == 1).all()


def test_table_values(oracle):
    """XOR values 0x01 and 0x80 occur, and received bytes of 0; share 0 is hit"""
    for case in (CASES[0], Case("G2", 5, "G-2", "ok"), Case("G5", 2, "A", "ok")):
        _, refs = geometry(oracle, case.geo)
        ref = refs[1][case.nums()]
        recv, m = received(oracle, case), case.mask()
        assert np.array_equal(recv != ref, m)
        x = (recv ^ ref)[m]
        assert (x == 0x01).any() and (x == 0x80).any() and (recv[m] == 0).any() and (recv[0] != ref[0]).any()


@pytest.mark.parametrize("case", CASES, ids=ids(CASES))
def test_table_by_oracle(oracle, case):
    """The oracle's Decode (per-column Berlekamp-Welch) of every case: the encoded
    data for ok, the error code for X"""
    k, n = case.dims[:2]
    segs, refs = geometry(oracle, case.geo)
    nums, recv = case.nums(), received(oracle, case)
    f = oracle.FEC(k, n)
    if case.expect == "ok":
        got = f.decode(nums, list(recv))
        assert np.array_equal(got, refs[1][:k].reshape(-1))
    else:
        with pytest.raises(oracle.OracleError) as ei:
            f.decode(nums, list(recv))
        assert ei.value.code == ORACLE_CODE[case.expect]


# ---- through the GPU ---------------------------------------------------------------

class Windows:
    """`count` windows of `size` bytes in one buffer filled with `fill`, GUARD bytes before, between and after"""

    def __init__(self, fill, count, size):
        self.fill, self.count, self.size = fill, count, size
        self.nbytes = GUARD + count * (size + GUARD)

    def at(self, w):
        return GUARD + w * (self.size + GUARD)

    def image(self, contents):
        """contents: {window: bytes}"""
        img = np.full(self.nbytes, self.fill, dtype=np.uint8)
        for w, a in contents.items():
            img[self.at(w):self.at(w) + self.size] = a
        return img

    def span(self, first, count):
        """the bytes of `count` windows from `first` on, with the guard before them (and the one after the last of all)"""
        last = first + count == self.count
        return self.at(first) - GUARD, self.nbytes if last else self.at(first + count) - GUARD

    def first_difference(self, got, want, ignore=(), span=None):
        """None, or (window, offset in it or None for a guard byte, got, want), within
        `span` (lo, hi) of the buffer; windows in `ignore` are not compared"""
        lo, hi = span or (0, self.nbytes)
        got, want = got[lo:hi], want[lo:hi]
        if np.array_equal(got, want):
            return None
        for w in ignore:
            if lo <= self.at(w) < hi:
                got = got.copy() if got.base is not None else got
                got[self.at(w) - lo:self.at(w) - lo + self.size] = want[self.at(w) - lo:self.at(w) - lo + self.size]
        if np.array_equal(got, want):
            return None
        b = lo + int(np.flatnonzero(got != want)[0])
        got, want = got[b - lo:], want[b - lo:]
        w, off = divmod(b - GUARD, self.size + GUARD) if b >= GUARD else (-1, self.size)
        return w, (off if off < self.size else None), int(got[0]), int(want[0])


ENTRIES = ("decode", "segments", "batched", "sets")


def run_segments(torch, lib, ctx, oracle, geo, entry, seglist):
    """One call of `entry` over seglist = [(data index, case or None, set owner)]:
    segment g holds segment `data` of the geometry, received through the set of
    `owner` (a case) and, where `case` is given, corrupted by it.  All n pieces
    of every segment lie in one PIECE_FILL buffer, the outputs in one OUT_FILL
    buffer.  Returns rc and, per segment, None or a description of the first byte
    that is not what it has to be (the bytes before a segment's windows count
    as its own, and those after the last window as the last segment's)."""
    k, n, ess, stripes, _ = GEOMETRIES[geo]
    plen = stripes * ess
    segs, refs = geometry(oracle, geo)
    nseg = len(seglist)
    pw, ow = Windows(PIECE_FILL, nseg * n, plen), Windows(OUT_FILL, nseg, k * plen)
    before, after, outs, ignore = {}, {}, {}, []
    failed = None
    for g, (data, case, owner) in enumerate(seglist):
        for i in range(n):
            before[g * n + i] = after[g * n + i] = refs[data][i]
        # ec_decode sees each piece as one share of plen bytes: the k data shares one after the other
        outs[g] = refs[data][:k].reshape(-1) if entry == "decode" else segs[data]
        if case is not None:
            for i, row in zip(case.nums(), case.corrupt(refs[data][case.nums()])):
                before[g * n + i] = row
            if case.expect != "ok":
                failed = case
                ignore += [g * n + i for i in case.nums()]
    want_p, want_o = pw.image(after), ow.image(outs)
    if entry == "decode":
        pieces, out = pw.image(before), ow.image({})
        base_p, base_o = pieces.ctypes.data, out.ctypes.data
    else:
        d_pieces, d_out = torch.from_numpy(pw.image(before)).cuda(), torch.from_numpy(ow.image({})).cuda()
        base_p, base_o = d_pieces.data_ptr(), d_out.data_ptr()
        stream = torch.cuda.current_stream().cuda_stream
    sets = [[owner.nums()[j] for j in owner.order()] for _, _, owner in seglist]
    ptr = lambda g, i: base_p + pw.at(g * n + i)
    ia = lambda xs: (ctypes.c_int * len(xs))(*xs)
    pa = lambda xs: (ctypes.c_void_p * len(xs))(*xs)
    if entry == "sets":
        flat = [(g, x) for g, s in enumerate(sets) for x in s]
        rc = lib.ec_decode_segments_sets(ctx, nseg, ia([len(s) for s in sets]), ia([x for _, x in flat]),
                                         pa([ptr(g, x) for g, x in flat]), stripes,
                                         pa([base_o + ow.at(g) for g in range(nseg)]), stream)
    else:
        assert all(s == sets[0] for s in sets)
        nums, ptrs = ia(sets[0]), pa([ptr(0, x) for x in sets[0]])
        if entry == "decode":
            assert nseg == 1
            rc = lib.ec_decode(ctx, len(sets[0]), nums, ptrs, plen, base_o + ow.at(0))
        elif entry == "segments":
            assert nseg == 1
            rc = lib.ec_decode_segments(ctx, len(sets[0]), nums, ptrs, stripes, base_o + ow.at(0), stream)
        else:
            rc = lib.ec_decode_segments_batched(ctx, len(sets[0]), nums, ptrs, stripes, nseg, n * (plen + GUARD),
                                                k * plen + GUARD, base_o + ow.at(0), stream)
    if entry != "decode":
        torch.cuda.synchronize()
        pieces, out = d_pieces.cpu().numpy(), d_out.cpu().numpy()
    ignore_o = range(nseg) if failed or rc else ()
    diffs = []
    for g in range(nseg):
        d = pw.first_difference(pieces, want_p, ignore, pw.span(g * n, n))
        if d:
            w, off, got, want = d
            where = f"segment {w // n}, share {w % n}, column {off}" if off is not None else f"the gap after piece window {w}"
            diffs.append(f"pieces: {where}: {got:#04x}, not {want:#04x}")
            continue
        d = ow.first_difference(out, want_o, ignore_o, ow.span(g, 1))
        if not d:
            diffs.append(None)
            continue
        w, off, got, want = d
        if off is None:
            where = f"the guard after window {w}"
        elif entry == "decode":
            where = f"segment {w}, byte {off} (data share {off // plen}, column {off % plen})"
        else:
            where = (f"segment {w}, byte {off} (stripe {off // (k * ess)}, data share {off % (k * ess) // ess}, "
                     f"column {off // (k * ess) * ess + off % ess})")
        diffs.append(f"output: {where}: {got:#04x}, not {want:#04x}")
    return rc, diffs


@pytest.fixture(scope="module")
def gpu():
    """(torch, the library, a context per geometry): the contexts are made on first use and closed at the end"""
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    from uplink_amd import _native
    lib = _native.load()
    made = {}

    def ctx(geo):
        if geo not in made:
            k, n, ess = GEOMETRIES[geo][:3]
            made[geo] = ctypes.c_void_p()
            rc = lib.ec_create(k, n, ess, ctypes.byref(made[geo]))
            assert rc == 0, rc
        return made[geo]

    try:
        yield torch, lib, ctx
    finally:
        torch.cuda.synchronize()
        for c in made.values():
            lib.ec_destroy(c)


def _check(case, rc, diffs):
    assert rc == RC[case.expect], f"{case.id}: rc {rc}, expected {case.expect} ({RC[case.expect]})"
    assert not any(diffs), f"{case.id}: {[d for d in diffs if d]}"


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ENTRIES[:3])
@pytest.mark.parametrize("case", CASES, ids=ids(CASES))
def test_decode_case(oracle, gpu, case, entry):
    """ec_decode (each piece one share of plen bytes), ec_decode_segments, and
    ec_decode_segments_batched over 3 segments of which the middle one carries the
    case: rc; the output; the set's pieces corrected in place; every other piece,
    gap and guard as before (after an error return: those alone)."""
    torch, lib, ctx = gpu
    seglist = [(0, None, case), (1, case, case), (2, None, case)] if entry == "batched" else [(1, case, case)]
    rc, diffs = run_segments(torch, lib, ctx(case.geo), oracle, case.geo, entry, seglist)
    _check(case, rc, diffs)


_sets_runs = {}


@pytest.mark.gpu
@pytest.mark.parametrize("case", OK_CASES, ids=ids(OK_CASES))
def test_decode_sets_ok_case(oracle, gpu, case):
    """ec_decode_segments_sets: all ok cases of a geometry in one call, each a
    segment with its own set and pattern over one of three different segments'
    data, a clean segment with the same set after each.  The call runs once per
    geometry; every case then answers for the call's rc and for its own two
    segments."""
    torch, lib, ctx = gpu
    if case.geo not in _sets_runs:
        mine = [c for c in OK_CASES if c.geo == case.geo]
        seglist = [x for i, c in enumerate(mine) for x in ((i % 3, c, c), ((i + 1) % 3, None, c))]
        _sets_runs[case.geo] = (mine, run_segments(torch, lib, ctx(case.geo), oracle, case.geo, "sets", seglist))
    mine, (rc, diffs) = _sets_runs[case.geo]
    at = mine.index(case)
    assert rc == 0, f"the call of {len(mine)} cases: rc {rc}"
    assert len(diffs) == 2 * len(mine)
    assert diffs[2 * at] is None, f"{case.id} (segment {2 * at} of the call): {diffs[2 * at]}"
    assert diffs[2 * at + 1] is None, f"the clean segment after {case.id} (segment {2 * at + 1}): {diffs[2 * at + 1]}"


@pytest.mark.gpu
@pytest.mark.parametrize("case", X_CASES, ids=ids(X_CASES))
def test_decode_sets_error_case(oracle, gpu, case):
    """ec_decode_segments_sets: an over-capacity case between two clean segments: the error code"""
    torch, lib, ctx = gpu
    rc, diffs = run_segments(torch, lib, ctx(case.geo), oracle, case.geo, "sets", [(0, None, case), (1, case, case), (2, None, case)])
    _check(case, rc, diffs)
