"""BWTCore.smem_long_batch / bwtmi_index_smem_long_batch: SMEM seeding of long
reads over an index built with its reverse index (BWTMI_INDEX_REVERSE),
against the brute-force oracle, texts and queries of tests/test_gpu_smem.py,
and against smem_batch wherever both entries accept the input."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_smem import Oracle, _b, _build_texts, _queries, _random_dna, assert_equal, revcomp

pytestmark = pytest.mark.gpu

_FIELDS = ("offsets", "qstart", "qend", "strand", "count", "pos_offsets", "positions")
CFGS = ["acgt", "gaps", "acgt-fm-bytes"]
E_ARG, E_STATE = -1, -5
MAX_LONG = 1 << 20


def _pieces(text: bytes, cuts, rc=False) -> bytes:
    """Pieces of the text back to back, with a substitution every 200 bytes or so."""
    rng = np.random.default_rng(len(cuts) * 1000 + cuts[0][0])
    q = np.frombuffer(b"".join(text[a:b] for a, b in cuts), dtype=np.uint8).copy()
    for i in range(97, q.size, 200):
        at = i + int(rng.integers(0, 40))
        if at < q.size:
            q[at] = rng.choice([c for c in b"ACGT" if c != q[at]])
    return revcomp(q.tobytes()) if rc else q.tobytes()


_CUTS = {1025: [(50, 600), (1000, 1475)], 2047: [(0, 1100), (1500, 2447)], 2048: [(300, 1500), (2000, 2848)],
         2049: [(10, 1400), (900, 1559)], 4100: [(100, 1500), (200, 2900)]}


def _long_queries(text: bytes):
    out = []
    for m, cuts in _CUTS.items():
        for rc in (False, True):
            out.append(_pieces(text, cuts, rc))
            assert len(out[-1]) == m
    out.append(_random_dna(np.random.default_rng(5), 2000).tobytes())
    out += [text, text + b"A"]
    x = bytearray(text[:2600])
    x[499::500] = b"X" * len(x[499::500])
    out.append(bytes(x))
    return out


@pytest.fixture(scope="module")
def texts(gpu_ctx):
    """name -> (text, BWTCore with its reverse index, Oracle, short queries, long queries)"""
    from bwtmi import BWTCore
    out = {}
    for name, t in _build_texts().items():
        core = BWTCore(t, build_kmer=False, reverse_index=True)
        assert core.has_reverse_index
        out[name] = (t, core, Oracle(t), _queries(t), _long_queries(t))
    return out


def _cfg(texts, cfg):
    from bwtmi import _lib
    return texts[cfg.split("-")[0]], _lib.knobs(FM_BYTES=int(cfg.endswith("fm-bytes")))


def _check_long(core, orc, queries, min_len=1, both=False, max_occ=None, **kw):
    res = core.smem_long_batch(queries, min_len=min_len, both_strands=both, max_occ=max_occ, **kw)
    want = orc.batch(queries, min_len, both, 1024 if max_occ is None else max_occ)
    assert_equal(res, want, (min_len, both, max_occ))
    return res, want


# ------------------------------------------------------------------ 1. where both entries accept the input
@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("min_len", [1, 12, 20])
@pytest.mark.parametrize("cfg", CFGS)
def test_short_entry_agreement(texts, cfg, min_len, both):
    (text, core, orc, queries, _), knob = _cfg(texts, cfg)
    assert max(len(q) for q in queries) == 1024
    with knob:
        res, want = _check_long(core, orc, queries, min_len, both)
        short = core.smem_batch(queries, min_len=min_len, both_strands=both)
    for f in _FIELDS:
        assert getattr(res, f).tobytes() == getattr(short, f).tobytes(), f
    assert (res.positions_total, res.work) == (short.positions_total, short.work)
    assert short.steps == 0 < res.steps < res.work
    assert want["qstart"].size > len(queries) // 2 and (np.diff(want["offsets"]) == 0).any()


# ------------------------------------------------------------------ 2. past 1024 bytes
@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("min_len", [1, 20])
@pytest.mark.parametrize("cfg", CFGS)
def test_long_queries(texts, cfg, min_len, both):
    (text, core, orc, _, queries), knob = _cfg(texts, cfg)
    assert sorted(len(q) for q in queries) == sorted([1025, 2047, 2048, 2049, 4100] * 2 + [2000, 3001, 3002, 2600])
    with knob:
        res, want = _check_long(core, orc, queries, min_len, both)
    assert (want["qend"] - want["qstart"]).max() > 1024
    assert (want["strand"] == 0).any() and (not both or (want["strand"] == 1).any())
    if min_len == 1:
        assert want["count"].max() > 1
    else:
        assert (np.diff(want["offsets"]) == 0).any()
    assert np.all(res.qend - res.qstart >= min_len)
    # one at a time: the same SMEMs (a lane's walk knows nothing of its neighbours)
    with knob:
        one = core.smem_long_batch(queries[8:9], min_len=min_len, both_strands=both)
    a, b = int(res.offsets[8]), int(res.offsets[9])
    assert one.qstart.tolist() == res.qstart[a:b].tolist() and one.count.tolist() == res.count[a:b].tolist()


def test_sentinel_and_absent_bytes(gpu_ctx):
    """The reverse index's sentinel rules (a step by the last byte is legitimate
    exactly at the end of the text, nothing follows it, no match wraps) on both
    rank paths and on a text whose last byte is no '$'; ends at absent bytes."""
    from bwtmi import BWTCore
    for text in (b"TACGTTAGCATCGATTACA$", b"TACGNTAGCATCGATTACA$", b"$ACGTTAG$CATCGATTAC#"):
        core, orc = BWTCore(text, build_kmer=False, reverse_index=True), Oracle(text)
        z = text[-1:]
        queries = [z + text[:4], text[-3:] + text[:3], z, text[-2:], b"A" + z + b"T", b"CA" + z + b"GG", z + b"G",
                   b"T" + z + b"A", text, text + text[:5], text[-7:-1] + z + z, b"A" + z, z + b"A", b"ACGX", b"A" + z + b"X",
                   b"XX", b"AXXA", b"XACA" + z + b"X", text[-40:]]
        for both in (False, True):
            _check_long(core, orc, queries, 1, both)
            _check_long(core, orc, queries, 3, both)


# ------------------------------------------------------------------ 3. SMEMs that overlap almost completely
def test_overlapping_smems(gpu_ctx):
    from bwtmi import BWTCore
    text = b"A" * 1500 + b"$"
    core, orc = BWTCore(text, build_kmer=False, reverse_index=True), Oracle(text)
    res, _ = _check_long(core, orc, [b"A" * 1600, b"A" * 1500], max_occ=4)
    qs, qe, st, cnt, pos = res[0]
    assert qs.tolist() == list(range(101)) and qe.tolist() == list(range(1500, 1601))
    assert cnt.tolist() == [1] * 101 and [p.tolist() for p in pos] == [[0]] * 101
    assert res[1][0].tolist() == [0] and res[1][1].tolist() == [1500] and res[1][3].tolist() == [1]
    # the quadratic case: every SMEM is searched afresh, three times its length
    assert 400_000 < res.steps < 4 * (101 * 1501 + 1600 + 1501 + 1500)


# ------------------------------------------------------------------ 4. steps
def _step_bound(orc, queries, both):
    """4 (sum over the SMEMs at min_len 1 of (len + 1), + m), summed over the searched strings"""
    total = 0
    for q in queries:
        q = _b(q)
        for Q in ([q, revcomp(q)] if both and revcomp(q) != q else [q]):
            total += 4 * (sum(e - s + 1 for s, e in orc.strand_smems(Q, 1)) + len(Q))
    return total


@pytest.mark.parametrize("cfg", CFGS)
def test_step_bound(texts, cfg):
    (text, core, orc, short, queries), knob = _cfg(texts, cfg)
    with knob:
        for qs in (queries, short):
            for both in (False, True):
                res = core.smem_long_batch(qs, min_len=1, both_strands=both)
                bound = _step_bound(orc, qs, both)
                print(cfg, len(qs), both, "steps", res.steps, "bound", bound, "work", res.work)
                assert 0 < res.steps <= bound
        whole = core.smem_long_batch([text], min_len=1)
    m = len(text)
    print(cfg, "whole text: steps", whole.steps, "work", whole.work)
    assert whole.work == m * (m + 1) // 2 and whole.steps <= 16 * m
    assert whole.qstart.tolist() == [0] and whole.qend.tolist() == [m]


# ------------------------------------------------------------------ 5. arguments and state, raw C ABI
def _raw_long(lib, core, queries, min_len=1, flags=0, max_occ=0, max_positions=0, off=None, blob=None):
    if blob is None:
        blob = np.frombuffer(b"".join(queries) or b"\0", dtype=np.uint8)
    if off is None:
        off = np.concatenate([[0], np.cumsum([len(q) for q in queries])])
    off = np.asarray(off, dtype=np.int64)
    ptrs = [C.c_void_p(0xdead) for _ in range(7)]
    counts = [C.c_int64(-7) for _ in range(5)]       # nsmem, npos, positions_total, work, steps
    rc = lib.bwtmi_index_smem_long_batch(core._ctx, core._h, blob.ctypes.data_as(C.c_void_p),
                                         off.ctypes.data_as(C.c_void_p), off.size - 1, min_len, flags, max_occ,
                                         max_positions, *[C.byref(p) for p in ptrs], *[C.byref(v) for v in counts])
    return rc, ptrs, [v.value for v in counts]


def test_c_abi_arguments_and_state(texts, built_lib):
    from bwtmi import BWTCore
    from bwtmi._lib import BwtmiError
    text, core, orc, _, _ = texts["acgt"]
    ok = [b"ACGTAC", b"GG"]
    # an index without its reverse index
    plain = BWTCore(text, build_kmer=False)
    assert not plain.has_reverse_index and built_lib.bwtmi_index_has_reverse(plain._h) == 0
    assert built_lib.bwtmi_index_has_reverse(core._h) == 1 and built_lib.bwtmi_index_has_reverse(None) == 0
    rc, ptrs, counts = _raw_long(built_lib, plain, ok)
    assert rc == E_STATE and b"reverse" in built_lib.bwtmi_last_error()
    assert all(p.value is None for p in ptrs) and counts == [0] * 5
    with pytest.raises(BwtmiError, match="reverse"):
        plain.smem_long_batch(ok)
    # argument errors: nothing reaches the device
    big = np.full(MAX_LONG + 1, ord("A"), dtype=np.uint8)
    for queries, off, min_len, flags, blob in ((ok, [0, 6, 6], 1, 0, None),           # an empty query
                                               (None, [0, MAX_LONG + 1], 1, 0, big),
                                               (ok, None, 0, 0, None), (ok, None, 1, 2, None)):
        rc, ptrs, counts = _raw_long(built_lib, core, queries, min_len, flags, off=off, blob=blob)
        assert rc == E_ARG and built_lib.bwtmi_last_error()
        assert all(p.value is None for p in ptrs) and counts == [0] * 5
    for queries, kw in (([""], {}), (["ACGT", ""], {}), ([big.tobytes()], {}), (["ACGT"], {"min_len": 0})):
        with pytest.raises(ValueError):
            core.smem_long_batch(queries, **kw)
    # the flag on a text whose last byte is not unique: refused, nothing built
    h = C.c_void_p(0xdead)
    t = np.frombuffer(b"ACGA", dtype=np.uint8)
    assert built_lib.bwtmi_index_build(core._ctx, t.ctypes.data_as(C.c_void_p), 4, 32, 128, 2, C.byref(h)) == E_ARG
    assert h.value is None
    assert built_lib.bwtmi_index_build(core._ctx, t.ctypes.data_as(C.c_void_p), 0, 32, 128, 2, C.byref(h)) == E_ARG
    with pytest.raises(ValueError):
        BWTCore(b"ACGA", reverse_index=True)
    # nq = 0: the empty result; `steps` may be NULL
    rc, ptrs, counts = _raw_long(built_lib, core, [])
    assert rc == 0 and counts == [0] * 5 and all(p.value is not None for p in ptrs)
    assert C.cast(ptrs[0], C.POINTER(C.c_int64))[0] == 0 and C.cast(ptrs[5], C.POINTER(C.c_int64))[0] == 0
    for p in ptrs:
        built_lib.bwtmi_free(p)
    res = core.smem_long_batch([])
    assert res.offsets.tolist() == [0] and res.pos_offsets.tolist() == [0] and len(res) == 0 and res.steps == 0
    blob = np.frombuffer(b"ACGT", dtype=np.uint8)
    off = np.array([0, 4], dtype=np.int64)
    ptrs, n1, n2 = [C.c_void_p() for _ in range(7)], C.c_int64(), C.c_int64()
    assert built_lib.bwtmi_index_smem_long_batch(core._ctx, core._h, blob.ctypes.data_as(C.c_void_p),
                                                 off.ctypes.data_as(C.c_void_p), 1, 1, 0, 0, 0,
                                                 *[C.byref(p) for p in ptrs], C.byref(n1), C.byref(n2), None, None,
                                                 None) == 0
    assert n1.value == orc.batch([b"ACGT"])["qstart"].size
    for p in ptrs:
        built_lib.bwtmi_free(p)


def test_position_cap(texts, built_lib):
    from bwtmi._lib import BwtmiError
    text, core, orc, _, queries = texts["acgt"]
    want = orc.batch(queries, 5, True, 50)
    total = want["positions_total"]
    assert total > 100
    res, _ = _check_long(core, orc, queries, 5, True, max_occ=50, max_positions=total)
    assert res.positions_total == total == res.positions.size
    with pytest.raises(BwtmiError, match=str(total)):
        core.smem_long_batch(queries, min_len=5, both_strands=True, max_occ=50, max_positions=total - 1)
    with pytest.raises(ValueError):
        core.smem_long_batch(queries, max_positions=0)
    rc, ptrs, counts = _raw_long(built_lib, core, queries, 5, 1, 50, total - 1)
    assert rc not in (0, E_ARG) and str(total).encode() in built_lib.bwtmi_last_error()
    assert all(p.value is None for p in ptrs) and counts == [0, 0, total, 0, 0]
    rc, ptrs, counts = _raw_long(built_lib, core, queries, 5, 1, 50, total)
    assert rc == 0 and counts[:4] == [want["qstart"].size, total, total, want["work"]] and counts[4] > 0
    for p in ptrs:
        assert p.value is not None
        built_lib.bwtmi_free(p)


# ------------------------------------------------------------------ 6. / 7. what the flag leaves alone
def test_short_entry_keeps_its_limit(texts):
    text, core, orc, _, _ = texts["acgt"]
    with pytest.raises(ValueError, match="1024"):
        core.smem_batch(["A" * 1025])
    assert core.smem_long_batch(["A" * 1025]).qstart.size > 0


@pytest.mark.parametrize("name", ["acgt", "gaps"])
def test_forward_index_unchanged(texts, name):
    from bwtmi import BWTCore
    text, core, _, queries, _ = texts[name]
    plain = BWTCore(text, build_kmer=False)
    assert (core.suffix_array == plain.suffix_array).all() and (core.bwt_arr == plain.bwt_arr).all()
    assert core.suffix_array.size == len(text) and core.sampled_sa == plain.sampled_sa and len(core.sampled_sa) > 1
    assert core.char_counts == plain.char_counts and core.char_totals == plain.char_totals
    assert sorted(core.occ_checkpoints) == sorted(plain.occ_checkpoints)
    for code, cp in core.occ_checkpoints.items():
        assert (cp == plain.occ_checkpoints[code]).all()
    pats = [q.decode("latin-1") for q in queries if len(q) <= 64]
    assert (core.backward_search_batch(pats) == plain.backward_search_batch(pats)).all()
    assert (core.lcp_array() == plain.lcp_array()).all()


# ------------------------------------------------------------------ 8. statistics names
@pytest.mark.parametrize("cfg", CFGS)
def test_statistics_names(texts, gpu_ctx, cfg):
    from bwtmi import _lib
    (text, core, orc, queries, _), knob = _cfg(texts, cfg)
    mine, twin = ("k_smem_walk2", "k_smem_walk") if cfg == "acgt" else ("k_smem_walk", "k_smem_walk2")
    stats = {}
    for entry in (core.smem_long_batch, core.smem_batch):
        with knob:
            _lib.kernel_stats_filter(gpu_ctx, "")
            _lib.kernel_stats(gpu_ctx, enable=True, reset=True)
            try:
                entry(queries[:12], min_len=8, both_strands=True)
            finally:
                stats[entry.__name__] = _lib.kernel_stats(gpu_ctx, enable=False, reset=True)
    count = lambda s, name: s.get(name, (0.0, 0, 0.0))[1]      # noqa: E731
    long, short = stats["smem_long_batch"], stats["smem_batch"]
    assert count(long, mine) == 1 and count(long, twin) == 0, long.keys()
    assert count(long, "k_smem_ms") == count(long, "k_smem_ms2") == 0
    assert count(long, "k_smem_flag") == count(long, "k_smem_compact") == 1
    assert count(short, "k_smem_walk") == count(short, "k_smem_walk2") == 0
    assert count(short, "k_smem_ms2" if cfg == "acgt" else "k_smem_ms") == 1
