"""The device primitives (csrc/radix.hip) on caller data, element for element
against numpy: the stable LSD radix sort in its five instantiations plus the
single out-of-place pass, the single-pass look-back scan (one row and many) and
the three-launch 64-bit scan.

bwtmi_radix_sort and bwtmi_exclusive_scan hand a host array to the primitive
exactly as the library's stages call it, so the sizes, bit ranges, alignments
and key distributions here are chosen by construction instead of by what a
pipeline happens to sort: every tile-count residue of the XCD tile order, the
16-ticket look-back block and its second level, partial tiles and partial
histogram workgroups, bit ranges that start above bit 0 (the 64-bit sort's
digit-byte hand-off), the scalar against the 16-byte histogram loads, several
look-back windows of the scan, unaligned and more than 64 scan rows, and the
look-back epoch wrap.

Both references are exact (no tolerance anywhere): a stable argsort of the
digits in [bit0, bit1) applied to keys and values, and a shifted cumsum.  A CPU
test holds them against sorted(key=...) and a running sum, so a disagreement on
the GPU names the kernel.  The sizes derive from radix.hip's constants (DESIGN.md
"The primitives' direct test"): kSub = 8192 keys per scatter tile, 1024 keys per
wave, kLbBlk = 16 tickets per look-back block, kTile = 4096 scan elements, 64
tiles per look-back step, kS64Tile = 2048.
"""
import ctypes as C
import functools

import numpy as np
import pytest

E_ARG = -1
SUB = 8192                 # kSub: keys per scatter tile
MID = SUB * 3 + 17         # a few tiles and a partial one
BIG = SUB * 273 + 5        # 274 tiles: under HIST_S = 1, 18 look-back blocks -> a second step of the aggregate loop
KEY_BITS = {"k64v64": 64, "k64v32": 64, "k64": 64, "k32v32": 32, "k16v32": 16, "pass_k32": 32}
KINDS = tuple(KEY_BITS)
DISTS = ("uniform", "equal", "alt2", "asc", "desc", "runs", "ff", "topbit")
_PATTERN = 0x5A3C96E1D2B4A587


# --------------------------------------------------------------------------
# references
# --------------------------------------------------------------------------
def ref_sort(keys, vals, bit0, bit1):
    """keys and vals in the stable order of the key bits [bit0, bit1)."""
    d = (keys.astype(np.uint64) >> np.uint64(bit0)) & np.uint64((1 << (bit1 - bit0)) - 1)
    order = np.argsort(d, kind="stable")
    return keys[order], (vals[order] if vals is not None else None)


def ref_scan_u32(a):
    """Exclusive scan mod 2^32 of every row of a (uint32[rows, n])."""
    a = np.asarray(a, dtype=np.uint32).astype(np.uint64)
    return ((np.cumsum(a, axis=-1) - a) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def ref_scan_i64(a):
    a = np.asarray(a, dtype=np.int64)
    return np.cumsum(a) - a


def make_keys(kind, n, dist, bit0, bit1, seed=0):
    """n keys of `kind` whose bits [bit0, bit1) follow `dist`; every other bit is random."""
    W, w = KEY_BITS[kind], bit1 - bit0
    rng = np.random.default_rng([seed, n, bit0, bit1, DISTS.index(dist), W])
    mask = (1 << w) - 1
    i = np.arange(n, dtype=np.uint64)
    if dist == "uniform":
        d = rng.integers(0, 1 << w, n, dtype=np.uint64)
    elif dist == "equal":          # one digit per pass; every 16-byte load is one run-length add
        d = np.full(n, _PATTERN & mask, dtype=np.uint64)
    elif dist == "alt2":
        d = np.where(i & np.uint64(1), np.uint64(_PATTERN & mask), np.uint64(~_PATTERN & mask))
    elif dist in ("asc", "desc"):
        d = (i << np.uint64(w)) // np.uint64(n) if w <= 32 else i * np.uint64(mask // n)
        if dist == "desc":
            d = d[::-1].copy()
    elif dist == "runs":           # runs of 1..300 equal digits: what the run-length add was written for
        lens = rng.integers(1, 301, n // 100 + 2)
        d = np.repeat(rng.integers(0, 1 << w, len(lens), dtype=np.uint64), lens)[:n]
        assert len(d) == n
    elif dist == "ff":
        d = np.full(n, mask, dtype=np.uint64)
    elif dist == "topbit":
        d = rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(w - 1)
    else:
        raise ValueError(dist)
    outside = rng.integers(0, 1 << W, n, dtype=np.uint64) & np.uint64(((1 << W) - 1) & ~(mask << bit0))
    return (outside | (d << np.uint64(bit0))).astype(_dt(kind)[0])


def _dt(kind):
    from bwtmi import _lib
    _, kt, vt = _lib.SORT_KINDS[kind]
    return kt, vt


def make_vals(kind, n):
    """The index of every pair (in both halves of a 64-bit value): a lost, doubled
    or reordered pair shows in the values."""
    vt = _dt(kind)[1]
    if vt is None:
        return None
    i = np.arange(n, dtype=np.uint64)
    return (i * np.uint64(0x100000001)).astype(vt) if vt == "<u8" else i.astype(vt)


@functools.lru_cache(maxsize=3)
def sort_case(kind, n, dist, bit0, bit1):
    """(keys, vals, expected keys, expected vals), read-only, shared by the tests of one case."""
    keys = make_keys(kind, n, dist, bit0, bit1)
    vals = make_vals(kind, n)
    ek, ev = ref_sort(keys, vals, bit0, bit1)
    for a in (keys, vals, ek, ev):
        if a is not None:
            a.setflags(write=False)
    return keys, vals, ek, ev


def _first_diff(got, want):
    bad = np.flatnonzero(got != want)
    return None if not len(bad) else (int(bad[0]), int(bad[0]) // SUB, len(bad), hex(int(got[bad[0]])),
                                      hex(int(want[bad[0]])))


def check_sort(ctx, kind, n, dist, bit0, bit1, skew=0):
    from bwtmi import _lib
    keys, vals, ek, ev = sort_case(kind, n, dist, bit0, bit1)
    gk, gv = _lib.radix_sort(ctx, kind, keys, vals, bit0, bit1, skew)    # raises unless the call returns 0
    what = (kind, n, dist, bit0, bit1, skew)
    assert np.array_equal(gk, ek), ("keys: (index, tile, wrong, got, want)", what, _first_diff(gk, ek))
    if ev is not None:
        assert np.array_equal(gv, ev), ("values: (index, tile, wrong, got, want)", what, _first_diff(gv, ev))


def full(kind):
    return (0, 8) if kind == "pass_k32" else (0, KEY_BITS[kind])


# --------------------------------------------------------------------------
# the references themselves (CPU)
# --------------------------------------------------------------------------
def test_references_against_plain_python():
    for kind, (b0, b1) in (("k64v64", (8, 24)), ("k64", (0, 40)), ("k32v32", (0, 32)), ("k16v32", (8, 16)),
                           ("pass_k32", (16, 24)), ("k64v32", (56, 64))):
        for dist in DISTS:
            n = 389
            keys, vals = make_keys(kind, n, dist, b0, b1), make_vals(kind, n)
            assert keys.dtype == np.dtype(_dt(kind)[0]) and len(keys) == n
            kl = [int(k) for k in keys]
            dig = [(k >> b0) & ((1 << (b1 - b0)) - 1) for k in kl]
            order = sorted(range(n), key=lambda i: dig[i])          # Python's sort is stable
            ek, ev = ref_sort(keys, vals, b0, b1)
            assert [int(k) for k in ek] == [kl[i] for i in order], (kind, dist)
            if vals is not None:
                assert [int(v) for v in ev] == [int(vals[i]) for i in order], (kind, dist)
                assert int(vals[n - 1]) == (n - 1) * (0x100000001 if vals.dtype.itemsize == 8 else 1)
            # the distributions are what they claim to be
            if dist in ("equal", "ff"):
                assert len(set(dig)) == 1 and (dist != "ff" or dig[0] == (1 << (b1 - b0)) - 1)
            if dist == "alt2":
                assert len(set(dig)) == 2 and dig[0] != dig[1] and dig[0] == dig[2]
            if dist == "asc":
                assert dig == sorted(dig) and dig[0] < dig[-1]
            if dist == "desc":
                assert dig == sorted(dig, reverse=True) and dig[0] > dig[-1]
            if dist == "topbit":
                assert set(dig) == {0, 1 << (b1 - b0 - 1)}
            if b1 - b0 < KEY_BITS[kind]:                            # the bits outside the range vary
                assert len({k & ~(((1 << (b1 - b0)) - 1) << b0) for k in kl}) > n // 2 or KEY_BITS[kind] - (b1 - b0) <= 8
    rng = np.random.default_rng(5)
    a = rng.integers(0, 1 << 32, (3, 211), dtype=np.uint64).astype(np.uint32)
    got = ref_scan_u32(a)
    for r in range(3):
        s = 0
        for i in range(a.shape[1]):
            assert int(got[r, i]) == s % (1 << 32)
            s += int(a[r, i])
        assert s > 1 << 32
    b = rng.integers(-(1 << 40), 1 << 40, 307)
    got, s = ref_scan_i64(b), 0
    for i in range(len(b)):
        assert int(got[i]) == s
        s += int(b[i])


# --------------------------------------------------------------------------
# sort
# --------------------------------------------------------------------------
def _ids(cases):
    return [f"{c[0]}-n{c[1]}-b{c[2]}_{c[3]}" + "".join(f"-{x}" for x in c[4:]) for c in cases]


# one wave's 1024 keys, one 8192-key tile; the full width and one digit (many equal digits: stability)
_SIZES = [(k, n, b0, b1) for k in KINDS for n in (1, 2, 63, 64, 65, 1023, 1025, 8191, 8192, 8193)
          for b0, b1 in {full(k), (0, 8)}]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n,bit0,bit1", _SIZES, ids=_ids(_SIZES))
def test_sort_structure_boundaries(gpu_ctx, kind, n, bit0, bit1):
    check_sort(gpu_ctx, kind, n, "uniform", bit0, bit1)


def _mid_range(kind):
    """Two passes starting above bit 0 where the key is wide enough."""
    return {64: (8, 24), 32: (8, 24), 16: (0, 16)}[KEY_BITS[kind]] if kind != "pass_k32" else (8, 16)


# every residue of the tile count mod 8 (xcd_tile) and both sides of the 16-ticket look-back block
_TILES = [(k, SUB * t + r) + _mid_range(k) for k in KINDS for t in (1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17)
          for r in ((0, 1, 8191) if t == 16 else ((0, 1, 8191)[t % 3],))]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n,bit0,bit1", _TILES, ids=_ids(_TILES))
def test_sort_tile_counts(gpu_ctx, kind, n, bit0, bit1):
    check_sort(gpu_ctx, kind, n, "uniform", bit0, bit1)


_BIG = [(k, BIG) + full(k) + (S,) for k in ("k64v32", "k32v32") for S in (1, 3, 16)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n,bit0,bit1,S", _BIG, ids=_ids(_BIG))
def test_sort_second_lookback_level(gpu_ctx, kind, n, bit0, bit1, S):
    """274 tiles: 274 histogram workgroups under HIST_S = 1 (block 17 sums 17 block
    aggregates in two steps), 92 under 3 (a partial last workgroup: 274 = 91 * 3 + 1),
    18 under 16 (274 = 17 * 16 + 2)."""
    from bwtmi import _lib
    with _lib.knobs(HIST_S=S):
        check_sort(gpu_ctx, kind, n, "uniform", bit0, bit1)


_RANGES = ([(k, MID, b0, b1) for k in ("k64v64", "k64v32", "k64")
            for b0, b1 in ((0, 64), (0, 8), (8, 24), (0, 48), (0, 40), (56, 64), (16, 56), (4, 28))] +
           [("k32v32", MID, b0, b1) for b0, b1 in ((0, 32), (0, 8), (8, 24), (24, 32), (16, 32), (4, 20))] +
           [("k16v32", MID, b0, b1) for b0, b1 in ((0, 16), (0, 8), (8, 16))] +
           [("pass_k32", MID, s, s + 8) for s in (0, 8, 16, 24)])


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n,bit0,bit1", _RANGES, ids=_ids(_RANGES))
def test_sort_bit_ranges(gpu_ctx, kind, n, bit0, bit1):
    """Stability over the digits in range with every other bit random; bit0 > 0 with
    64-bit keys and several passes takes the next-digit-byte hand-off from a pass
    that does not start at bit 0."""
    check_sort(gpu_ctx, kind, n, "uniform", bit0, bit1)
    check_sort(gpu_ctx, kind, n, "runs", bit0, bit1)


def _dist_range(kind):
    """An odd number of passes for 64-bit keys (the result is copied back), the full width otherwise."""
    return (0, 40) if KEY_BITS[kind] == 64 else (16, 24) if kind == "pass_k32" else (0, KEY_BITS[kind])


_DISTS = ([(k, MID) + _dist_range(k) + (d,) for k in KINDS for d in DISTS] +
          [(k, BIG) + _dist_range(k) + (d,) for k in ("k64v32", "k32v32") for d in DISTS])


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n,bit0,bit1,dist", _DISTS, ids=_ids(_DISTS))
def test_sort_key_distributions(gpu_ctx, kind, n, bit0, bit1, dist):
    check_sort(gpu_ctx, kind, n, dist, bit0, bit1)


# skew 1 breaks the 16-byte alignment of every key width (the scalar histogram
# loads); 3 too; the same keys as skew 0 must come out the same
_SKEW = ([(k, MID) + _dist_range(k) + (d,) for k in KINDS for d in ("runs", "uniform")] +
         [(k, BIG) + _mid_range(k) + ("runs",) for k in ("k64v32", "k32v32")])


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n,bit0,bit1,dist", _SKEW, ids=_ids(_SKEW))
def test_sort_alignment(gpu_ctx, kind, n, bit0, bit1, dist):
    for skew in (0, 1, 3) if n == MID else (0, 1):
        check_sort(gpu_ctx, kind, n, dist, bit0, bit1, skew)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_sort_with_device_checks(gpu_ctx, kind):
    """BWTMI_DEVICE_CHECKS = 1 hands both kernels the check word, which changes
    their control flow: the same result, and no check fires (the call returns 0)."""
    from bwtmi import _lib
    with _lib.knobs(DEVICE_CHECKS=1):
        check_sort(gpu_ctx, kind, MID, "runs", *_dist_range(kind))
        check_sort(gpu_ctx, kind, SUB * 17 + 1, "uniform", *_mid_range(kind), skew=1)


# --------------------------------------------------------------------------
# scan
# --------------------------------------------------------------------------
TILE = 4096                # kTile: elements per scan workgroup
_SCAN_N = (1, 15, 16, 17, 4095, 4096, 4097, TILE * 64, TILE * 64 + 1, TILE * 130 + 7)


@functools.lru_cache(maxsize=4)
def scan_input(what, n):
    rng = np.random.default_rng([n, len(what)])
    if what == "small":
        a = rng.integers(0, 1000, n, dtype=np.uint32)
    elif what == "zeros":
        a = np.zeros(n, dtype=np.uint32)
    elif what == "ones":
        a = np.ones(n, dtype=np.uint32)
    else:                      # "wrap": the running sum passes 2^32 (from the second element on)
        a = rng.integers(1 << 31, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    want = ref_scan_u32(a)
    a.setflags(write=False)
    want.setflags(write=False)
    return a, want


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["small", "zeros", "ones", "wrap"])
@pytest.mark.parametrize("n", _SCAN_N)
def test_scan_u32_one_row(gpu_ctx, n, what):
    """Up to three 64-tile look-back windows (131 tiles); 16-byte and scalar
    loads (skew); in place and out of place."""
    from bwtmi import _lib
    a, want = scan_input(what, n)
    for in_place in (False, True):
        for skew in (0, 1):
            got = _lib.exclusive_scan(gpu_ctx, "u32", a, skew=skew, in_place=in_place)
            assert np.array_equal(got, want), (n, what, in_place, skew, _first_diff(got, want))


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [False, True], ids=["stride_n", "stride_4"])
@pytest.mark.parametrize("rows", [4, 64, 65, 94])
def test_scan_u32_rows(gpu_ctx, rows, aligned):
    """Rows scanned independently; stride = n (odd: scalar loads, rows adjacent) or
    rounded up to 4 (vector loads) with the padding between rows untouched; more
    than 64 rows take two launches that share the granule buffer."""
    from bwtmi import _lib
    n = TILE * 3 + 5
    stride = (n + 3) // 4 * 4 if aligned else n
    assert (stride & 3 != 0) == (not aligned)
    total = (rows - 1) * stride + n
    rng = np.random.default_rng([rows, stride])
    a = np.full(total, 0xDEADBEEF, dtype=np.uint32)
    body = rng.integers(0, 1 << 20, (rows, n), dtype=np.uint32)
    body[1] = rng.integers(1 << 31, 1 << 32, n, dtype=np.uint64).astype(np.uint32)   # one row passes 2^32
    row_of = np.arange(rows)[:, None] * stride + np.arange(n)[None, :]
    a[row_of] = body
    pad = np.ones(total, dtype=bool)
    pad[row_of] = False
    assert pad.sum() == (rows - 1) * (stride - n)
    want = ref_scan_u32(body)
    got = _lib.exclusive_scan(gpu_ctx, "u32", a, n=n, rows=rows, stride=stride, in_place=True)
    assert np.array_equal(got[row_of], want), (rows, stride, np.flatnonzero((got[row_of] != want).any(axis=1))[:5])
    assert (got[pad] == 0xDEADBEEF).all()
    out0 = np.full(total, 0x0BADF00D, dtype=np.uint32)
    got = _lib.exclusive_scan(gpu_ctx, "u32", a, n=n, rows=rows, stride=stride, out=out0)
    assert np.array_equal(got[row_of], want), (rows, stride, np.flatnonzero((got[row_of] != want).any(axis=1))[:5])
    assert (got[pad] == 0x0BADF00D).all()


S64 = 2048                 # kS64Tile


@pytest.mark.gpu
@pytest.mark.parametrize("signed", [False, True], ids=["pos", "signed"])
@pytest.mark.parametrize("n", [1, 2047, 2048, 2049, S64 * 256, S64 * 257 + 3, S64 * 600 + 1])
def test_scan_i64(gpu_ctx, n, signed):
    """More than 256 tiles: k_scan64_sums with several tile sums per thread and empty
    trailing threads (601 tiles: 3 per thread, threads 201.. empty); sums far above 2^32."""
    from bwtmi import _lib
    rng = np.random.default_rng([n, signed])
    a = rng.integers(-(1 << 40) if signed else 0, 1 << 40, n)
    a[-1] = 1 << 40
    want = ref_scan_i64(a)
    assert n < 4096 or abs(int(want[-1])) > 1 << 32
    for in_place in (False, True):
        for skew in (0, 1):
            got = _lib.exclusive_scan(gpu_ctx, "i64", a, skew=skew, in_place=in_place)
            assert np.array_equal(got, want), (n, in_place, skew, _first_diff(got, want))


# --------------------------------------------------------------------------
# launches that share the look-back state
# --------------------------------------------------------------------------
def _scan_once(ctx, n, seed, epoch=0, rows=1):
    from bwtmi import _lib
    a = np.random.default_rng(seed).integers(0, 1 << 24, (rows, n), dtype=np.uint32)
    got = _lib.exclusive_scan(ctx, "u32", a, n=n, rows=rows, stride=n, in_place=bool(seed & 1), epoch=epoch)
    assert np.array_equal(got.reshape(rows, n), ref_scan_u32(a)), (n, seed, rows, epoch)


def _sort_once(ctx, kind, n, bit0, bit1, seed):
    from bwtmi import _lib
    keys, vals = make_keys(kind, n, "runs", bit0, bit1, seed), make_vals(kind, n)
    ek, ev = ref_sort(keys, vals, bit0, bit1)
    gk, gv = _lib.radix_sort(ctx, kind, keys, vals, bit0, bit1)
    assert np.array_equal(gk, ek) and np.array_equal(gv, ev), (kind, n, bit0, bit1, seed)


@pytest.mark.gpu
def test_lookback_epoch_wrap(built_lib):
    """lb_prepare draws an epoch per launch and at 2^30 starts again at 1 with the
    granules cleared.  On a context of its own: preset to 2^30 - 3, so the second
    launch after it wraps -- once between the two passes of a sort, once (preset
    again: the epoch is small after a wrap) on a scan of three look-back windows."""
    from bwtmi import _lib
    h = C.c_void_p()
    # an in-process CLI run earlier in the session leaves BWTMI_NUMA_BIND on, and
    # bwtmi_open reads it: this open must not move the session's host threads
    with _lib.knobs(NUMA_BIND=0):
        _lib.check(built_lib.bwtmi_open(0, C.byref(h)))
    try:
        top = (1 << 30) - 3
        _scan_once(h, TILE * 130 + 7, 1)                          # granules of small epochs in the buffer
        _sort_once(h, "k32v32", SUB * 17 + 1, 0, 16, 2)
        _scan_once(h, TILE * 130 + 7, 3, epoch=top)               # launch epoch 2^30 - 2
        _sort_once(h, "k32v32", SUB * 17 + 1, 0, 16, 4)           # passes at 2^30 - 1 and, wrapped, 1
        _scan_once(h, TILE * 3 + 5, 5, rows=94)                   # 2, 3
        _scan_once(h, TILE * 130 + 7, 6)                          # 4
        _scan_once(h, TILE * 64 + 1, 7)
        assert built_lib.bwtmi_exclusive_scan(h, 0, None, None, 0, 1, 0, 0, 0, 5) == E_ARG   # not above the current epoch
        _scan_once(h, TILE * 9, 8, epoch=top)                     # 2^30 - 2
        _scan_once(h, TILE * 70 + 1, 9)                           # 2^30 - 1
        _scan_once(h, TILE * 130 + 7, 10)                         # wrapped: 1
        _sort_once(h, "k64v32", SUB * 17 + 1, 8, 24, 11)
        _scan_once(h, TILE * 130 + 7, 12)                         # one more of each
        _sort_once(h, "k16v32", SUB * 33 + 9, 0, 16, 13)
    finally:
        _lib.check(built_lib.bwtmi_close(h))


@pytest.mark.gpu
def test_back_to_back_launches_share_the_granules(gpu_ctx):
    """Histogram launches (256 granules per workgroup plus block aggregates), row
    scans (a granule range per row) and one-row scans lay the one granule buffer
    out differently; alternated at different sizes, each must see only its own."""
    for rnd in range(3):
        _sort_once(gpu_ctx, "k64v32", SUB * (20 - 7 * rnd) + 11, 0, 24, 20 + rnd)
        _scan_once(gpu_ctx, TILE * (2 + rnd) + 1, 30 + rnd, rows=70 - 30 * rnd)
        _scan_once(gpu_ctx, TILE * (90 - 40 * rnd) + 3, 40 + rnd)
        _sort_once(gpu_ctx, "k16v32", SUB * (3 + 6 * rnd) + 8191, 0, 16, 50 + rnd)
        _scan_once(gpu_ctx, 777 + rnd, 60 + rnd, rows=5)
        _sort_once(gpu_ctx, "pass_k32", SUB * (17 - 8 * rnd), 8, 16, 70 + rnd)


# --------------------------------------------------------------------------
# argument errors
# --------------------------------------------------------------------------
@pytest.mark.gpu
def test_argument_errors(gpu_ctx, built_lib):
    """Every rejected call returns BWTMI_E_ARG and leaves the caller's arrays as they
    were; the context then still sorts and scans right."""
    from bwtmi import _lib
    n = 1000
    k0 = make_keys("k64v32", n, "uniform", 0, 64)
    v0 = make_vals("k64v32", n)

    def sort(kind="k64v32", keys=True, vals=True, n=n, bit0=0, bit1=64, skew=0, ctx=gpu_ctx):
        code = _lib.SORT_KINDS[kind][0] if isinstance(kind, str) else kind
        k, v = k0.copy(), v0.copy()
        rc = built_lib.bwtmi_radix_sort(ctx, code, k.ctypes.data_as(C.c_void_p) if keys else None,
                                        v.ctypes.data_as(C.c_void_p) if vals else None, n, bit0, bit1, skew)
        assert np.array_equal(k, k0) and np.array_equal(v, v0) or rc == 0
        return rc

    assert sort() == 0
    for kw in (dict(kind=6), dict(kind=-1), dict(n=-1), dict(keys=False), dict(vals=False), dict(bit0=-8, bit1=0),
               dict(bit0=-1, bit1=7), dict(bit1=72), dict(bit0=64, bit1=72), dict(bit0=8, bit1=8),
               dict(bit0=16, bit1=8), dict(bit1=60), dict(bit0=3, bit1=64), dict(bit0=4, bit1=8, kind="k64"),
               dict(skew=-1), dict(skew=16), dict(ctx=None),
               dict(kind="k32v32", bit1=40), dict(kind="k16v32", bit1=24), dict(kind="k16v32", bit1=32),
               dict(kind="pass_k32", bit1=16), dict(kind="pass_k32", bit0=28, bit1=36),
               dict(kind="pass_k32", bit0=32, bit1=40), dict(kind="k64v64", vals=False)):
        assert sort(**kw) == E_ARG, kw
        assert built_lib.bwtmi_last_error()
    assert sort(kind="k64", vals=False) == 0                       # keys alone: no values needed
    assert sort(n=0, keys=False, vals=False) == 0
    assert sort(n=0, keys=False, vals=False, bit1=60) == E_ARG     # the range is checked with nothing to sort too

    a0 = np.arange(3 * 1024, dtype=np.uint32)
    o0 = np.full(3 * 1024, 7, dtype=np.uint32)

    def scan(kind=0, a=True, out=True, n=1000, rows=1, stride=0, skew=0, in_place=0, epoch=0, ctx=gpu_ctx):
        a_, o = a0.copy(), o0.copy()
        rc = built_lib.bwtmi_exclusive_scan(ctx, kind, a_.ctypes.data_as(C.c_void_p) if a else None,
                                            o.ctypes.data_as(C.c_void_p) if out else None, n, rows, stride, skew,
                                            in_place, epoch)
        assert np.array_equal(a_, a0) and (np.array_equal(o, o0) or rc == 0)
        return rc

    assert scan() == 0                                             # (the context's epoch is now at least 1)
    for kw in (dict(kind=2), dict(kind=-1), dict(n=-1), dict(rows=0), dict(rows=-2), dict(rows=3, stride=-1024),
               dict(rows=3, stride=999), dict(rows=3, stride=0), dict(a=False), dict(out=False),
               dict(kind=1, rows=2, stride=1000, n=500), dict(skew=-1), dict(skew=16), dict(ctx=None),
               dict(epoch=1), dict(epoch=-5), dict(epoch=1 << 30), dict(epoch=(1 << 30) + 7), dict(epoch=1 << 40)):
        assert scan(**kw) == E_ARG, kw
        assert built_lib.bwtmi_last_error()
    assert scan(rows=3, stride=1024, n=1000) == 0
    assert scan(n=0, a=False, out=False) == 0
    check_sort(gpu_ctx, "k64v32", MID, "runs", 8, 24)
    _scan_once(gpu_ctx, TILE * 5 + 1, 99, rows=3)
