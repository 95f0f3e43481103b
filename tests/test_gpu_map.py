"""BWTCore.map_batch / bwtmi_index_map_batch: SMEM seeds chained on the device,
against the brute-force SMEM oracle of tests/test_gpu_smem.py -> anchors -> the
chain oracle of tests/test_gpu_chain.py, on the texts and queries of the SMEM
tests (short and long), and on reads through a tandem-repeat tract."""
import ctypes as C
import random

import numpy as np
import pytest

from test_gpu_chain import DEFAULTS, chain_oracle
from test_gpu_smem import Oracle, _b, _build_texts, _queries, revcomp
from test_gpu_smem_long import _long_queries

gpu = pytest.mark.gpu
E_ARG, E_NOMEM, E_STATE = -1, -4, -5
CFGS = ["acgt", "gaps", "acgt-fm-bytes"]
# a window the Python DP can afford on ~10^4 anchors; the device's window sizes are tests/test_gpu_chain.py's
QUICK = dict(max_pred=48, min_score=25)


# ------------------------------------------------------------------ the oracle
def map_oracle(orc, queries, min_len, both, max_occ=1024, **params):
    """The call's expected arrays, as a dict of the MapResult fields."""
    groups, lens, skipped = [], [], 0
    for q in queries:
        q = _b(q)
        rc = revcomp(q)
        for strand, Q in ((0, q), (1, rc)):
            g = []
            if strand == 0 or (both and rc != q):
                for s, e in orc.strand_smems(Q, min_len):
                    occ = orc.occurrences(Q[s:e])
                    if len(occ) > max_occ:
                        skipped += 1
                    else:
                        g += [(s, p, e - s) for p in occ]
            groups.append(g)
            lens.append(len(q))
    ch = chain_oracle(groups, **params)
    flat = [a for g in groups for a in g]
    group_of = np.repeat(np.arange(len(groups)), np.diff(ch["chain_off"]))
    rev = (group_of % 2).astype(bool)
    m = np.array(lens, np.int64)[group_of] if group_of.size else np.zeros(0, np.int64)
    mq, mr, ml = [], [], []
    for k in range(ch["score"].size):
        for t in ch["member"][ch["member_off"][k]:ch["member_off"][k + 1]].tolist():
            q, r, l = flat[t]
            mq.append(int(m[k]) - q - l if rev[k] else q)
            mr.append(r)
            ml.append(l)
    return {"offsets": ch["chain_off"][::2].copy(), "strand": rev.astype(np.uint8), "score": ch["score"],
            "n_anchors": ch["n_anchors"],
            "qstart": np.where(rev, m - ch["qend"], ch["qstart"]).astype(np.int32),
            "qend": np.where(rev, m - ch["qstart"], ch["qend"]).astype(np.int32),
            "rstart": ch["rstart"], "rend": ch["rend"], "member_offsets": ch["member_off"],
            "member_q": np.array(mq, np.int32), "member_r": np.array(mr, np.int64), "member_len": np.array(ml, np.int32),
            "positions_total": len(flat), "anchors": len(flat), "skipped_smems": skipped, "evals": ch["evals"]}


_FIELDS = ("offsets", "strand", "score", "n_anchors", "qstart", "qend", "rstart", "rend", "member_offsets", "member_q",
           "member_r", "member_len")
_COUNTS = ("positions_total", "anchors", "skipped_smems", "evals")


def assert_equal(res, want, what=None):
    for f in _FIELDS:
        got = getattr(res, f)
        assert got.dtype == want[f].dtype, (f, got.dtype, what)
        assert got.shape == want[f].shape and got.tolist() == want[f].tolist(), (f, what)
    for f in _COUNTS:
        assert getattr(res, f) == want[f], (f, what)


def dl_of(res, k, m):
    """(last qe - first qe) - (last re - first re) of chain k, in the searched string's coordinates"""
    a, b = int(res.member_offsets[k]), int(res.member_offsets[k + 1]) - 1
    qe = [(m - int(res.member_q[t])) if res.strand[k] else int(res.member_q[t]) + int(res.member_len[t]) for t in (a, b)]
    re = [int(res.member_r[t]) + int(res.member_len[t]) for t in (a, b)]
    return (qe[1] - qe[0]) - (re[1] - re[0])


# ------------------------------------------------------------------ the tandem-repeat case
def _str_case():
    rng = random.Random(7)
    dna = lambda n: "".join(rng.choice("ACGT") for _ in range(n))      # noqa: E731
    L, R = dna(300), dna(300)
    text = (dna(200) + L + "CAG" * 20 + R + dna(200) + "$").encode()
    reads, copies = [], []
    for n in (20, 12, 45):
        Q = L[-150:] + "CAG" * n + R[:150]
        for i in (40, 260):
            Q = Q[:i] + ("A" if Q[i] != "A" else "C") + Q[i + 1:]
        reads += [Q.encode(), revcomp(Q.encode())]
        copies += [n, n]
    return text, reads, copies


class _Arrays:
    def __init__(self, d):
        self.__dict__.update(d)


def test_str_case_on_the_oracle():
    """The fixed seed gives what the device test asserts: every read's first
    chain spans the whole read, on the read's strand, with dl = 3 (copies - 20)."""
    text, reads, copies = _str_case()
    want = _Arrays(map_oracle(Oracle(text), reads, 15, True))
    for i, (read, n) in enumerate(zip(reads, copies)):
        k = int(want.offsets[i])
        assert want.offsets[i + 1] > k
        assert (int(want.qstart[k]), int(want.qend[k]), int(want.strand[k])) == (0, len(read), i % 2), i
        assert dl_of(want, k, len(read)) == 3 * (n - 20), i
        assert (int(want.rstart[k]), int(want.rend[k])) == (350, 710)      # 150 bases of each flank
    assert want.anchors > 50 and want.n_anchors.max() > 3 and np.diff(want.offsets).max() > 10


# ------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def texts(gpu_ctx):
    """name -> (text, BWTCore with its reverse index, Oracle, short queries, long queries)"""
    from bwtmi import BWTCore
    out = {}
    for name, t in _build_texts().items():
        out[name] = (t, BWTCore(t, build_kmer=False, reverse_index=True), Oracle(t), _queries(t), _long_queries(t))
    return out


_wanted = {}


def _want(name, orc, queries, min_len, both, max_occ=1024, **params):
    """the oracle's result, computed once per input (the fm-bytes runs share the packed path's)"""
    key = (name, len(queries), min_len, both, max_occ, tuple(sorted(params.items())))
    if key not in _wanted:
        _wanted[key] = map_oracle(orc, queries, min_len, both, max_occ, **params)
    return _wanted[key]


def _cfg(texts, cfg):
    from bwtmi import _lib
    return cfg.split("-")[0], texts[cfg.split("-")[0]], _lib.knobs(FM_BYTES=int(cfg.endswith("fm-bytes")))


# ------------------------------------------------------------------ 1. parity, both entries
@gpu
@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("min_len", [1, 20])
@pytest.mark.parametrize("cfg", CFGS)
def test_brute_force_parity(texts, cfg, min_len, both):
    name, (text, core, orc, queries, _), knob = _cfg(texts, cfg)
    params = QUICK if min_len == 1 else {}
    want = _want(name, orc, queries, min_len, both, **params)
    with knob:
        res = core.map_batch(queries, min_len=min_len, both_strands=both, **params)
        long = core.map_batch(queries, min_len=min_len, both_strands=both, long=True, **params)
    assert_equal(res, want, (cfg, min_len, both))
    assert_equal(long, want, (cfg, min_len, both, "long"))
    # the run is not vacuous
    assert len(res) == len(queries) and (np.diff(want["offsets"]) == 0).any() and want["score"].size > 10
    assert want["n_anchors"].max() > 1 and (not both or (want["strand"] == 1).any())
    assert want["anchors"] > (1000 if min_len == 1 else 30) and want["evals"] > (want["anchors"] if min_len == 1 else 0)
    # what the arrays say of themselves
    assert np.all(res.qstart < res.qend) and np.all(res.rstart < res.rend) and np.all(res.score >= 25)
    assert np.all(np.diff(res.member_offsets) == res.n_anchors)
    i = 22                                            # the first 150 bp read, cut at 100: its first chain lies there
    strand, score, n, qs, qe, rs, re, mem = res[i]
    assert qe[0] - qs[0] > 100 and 100 <= rs[0] < 250 and mem[0].shape == (n[0], 3) and (min_len == 1 or strand[0] == 0)


@gpu
@pytest.mark.parametrize("cfg", CFGS)
def test_long_queries(texts, cfg):
    name, (text, core, orc, _, queries), knob = _cfg(texts, cfg)
    want = _want(name, orc, queries, 20, True)
    with knob:
        res = core.map_batch(queries, min_len=20, both_strands=True, long=True)
    assert_equal(res, want, cfg)
    assert (want["qend"] - want["qstart"]).max() > 1024 and (want["strand"] == 1).any() and want["n_anchors"].max() > 3
    with pytest.raises(ValueError, match="1024"):
        core.map_batch(queries, min_len=20)


@gpu
def test_max_occ_skips_frequent_seeds(texts):
    text, core, orc, queries, _ = texts["acgt"]
    want = _want("acgt", orc, queries, 5, True, 2, **QUICK)
    assert_equal(core.map_batch(queries, min_len=5, both_strands=True, max_occ=2, **QUICK), want)
    assert want["skipped_smems"] > 0 and want["anchors"] > 100


# ------------------------------------------------------------------ 2. a read through a repeat tract
@gpu
def test_str_tract_length(gpu_ctx):
    from bwtmi import BWTCore
    text, reads, copies = _str_case()
    core = BWTCore(text, build_kmer=False, reverse_index=True)
    want = map_oracle(Oracle(text), reads, 15, True)
    for long in (False, True):
        res = core.map_batch(reads, min_len=15, both_strands=True, long=long)
        assert_equal(res, want, long)
        for i, (read, n) in enumerate(zip(reads, copies)):
            k = int(res.offsets[i])
            assert (int(res.qstart[k]), int(res.qend[k]), int(res.strand[k])) == (0, len(read), i % 2)
            assert dl_of(res, k, len(read)) == 3 * (n - 20)


# ------------------------------------------------------------------ 3. cap, state, arguments
def _raw(lib, core, queries, min_len=1, flags=0, max_occ=0, max_positions=0, params=None, off=None):
    from bwtmi._lib import ChainParams
    blob = np.frombuffer(b"".join(queries) or b"\0", dtype=np.uint8)
    if off is None:
        off = np.concatenate([[0], np.cumsum([len(q) for q in queries])])
    off = np.asarray(off, dtype=np.int64)
    p = ChainParams()
    for k, v in (params or {}).items():
        if k == "reserved":
            p.reserved[v] = 1
        else:
            setattr(p, k, v)
    ptrs = [C.c_void_p(0xdead) for _ in range(12)]
    counts = [C.c_int64(-7) for _ in range(6)]    # nchain, nmember, positions_total, skipped, anchors, evals
    rc = lib.bwtmi_index_map_batch(core._ctx, core._h, blob.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p),
                                   off.size - 1, min_len, flags, max_occ, max_positions, C.byref(p),
                                   *[C.byref(x) for x in ptrs], *[C.byref(v) for v in counts])
    return rc, ptrs, [v.value for v in counts]


@gpu
def test_position_cap(texts, built_lib):
    from bwtmi._lib import BwtmiError
    text, core, orc, queries, _ = texts["acgt"]
    queries = queries[:30]
    want = _want("acgt30", orc, queries, 5, True, 50, **QUICK)
    total = want["positions_total"]
    assert total > 100
    res = core.map_batch(queries, min_len=5, both_strands=True, max_occ=50, max_positions=total, **QUICK)
    assert_equal(res, want)
    with pytest.raises(BwtmiError, match=str(total)):
        core.map_batch(queries, min_len=5, both_strands=True, max_occ=50, max_positions=total - 1, **QUICK)
    with pytest.raises(ValueError):
        core.map_batch(queries, max_positions=0)
    rc, ptrs, counts = _raw(built_lib, core, queries, 5, 1, 50, total - 1)
    assert rc == E_NOMEM and str(total).encode() in built_lib.bwtmi_last_error()
    assert all(p.value is None for p in ptrs) and counts == [0, 0, total, 0, 0, 0]


@gpu
def test_c_abi_arguments_and_state(texts, built_lib):
    from bwtmi import BWTCore
    from bwtmi._lib import BwtmiError
    text, core, orc, _, _ = texts["acgt"]
    ok = [b"ACGTAC", b"GG"]
    plain = BWTCore(text, build_kmer=False)
    rc, ptrs, counts = _raw(built_lib, plain, ok, flags=4)
    assert rc == E_STATE and b"reverse" in built_lib.bwtmi_last_error()
    assert all(p.value is None for p in ptrs) and counts == [0] * 6
    with pytest.raises(BwtmiError, match="reverse"):
        plain.map_batch(ok, long=True)
    assert len(plain.map_batch(ok)) == 2
    for queries, off, min_len, flags, params in ((ok, [0, 6, 6], 1, 0, {}),                 # an empty query
                                                 ([b"A" * 1025], None, 1, 0, {}),
                                                 (ok, None, 0, 0, {}), (ok, None, 1, 2, {}), (ok, None, 1, 8, {}),
                                                 (ok, None, 1, 0, {"max_pred": 4097}),
                                                 (ok, None, 1, 0, {"max_gap": 100, "bandwidth": 101}),
                                                 (ok, None, 1, 4, {"reserved": 1})):
        rc, ptrs, counts = _raw(built_lib, core, queries, min_len, flags, off=off, params=params)
        assert rc == E_ARG and built_lib.bwtmi_last_error(), (queries, min_len, flags, params)
        assert all(p.value is None for p in ptrs) and counts == [0] * 6
    for queries, kw in (([""], {}), (["A" * 1025], {}), (["ACGT"], {"min_len": 0}), (["ACGT"], {"max_pred": 4097}),
                        (["ACGT"], {"bandwidth": 600, "max_gap": 500}), (["ACGT"], {"min_score": 0})):
        with pytest.raises(ValueError):
            core.map_batch(queries, **kw)
    with pytest.raises(TypeError):
        core.map_batch(["ACGT"], max_gaps=3)
    # nq = 0: the empty result, on both entries
    for flags in (0, 4, 5):
        rc, ptrs, counts = _raw(built_lib, core, [], flags=flags)
        assert rc == 0 and counts == [0] * 6 and all(p.value not in (None, 0xdead) for p in ptrs)
        assert C.cast(ptrs[0], C.POINTER(C.c_int64))[0] == 0 and C.cast(ptrs[8], C.POINTER(C.c_int64))[0] == 0
        for p in ptrs:
            built_lib.bwtmi_free(p)
    res = core.map_batch([])
    assert res.offsets.tolist() == [0] and res.member_offsets.tolist() == [0] and len(res) == 0
    assert res.strand.dtype == np.uint8 and res.score.dtype == np.int32 and res.rstart.dtype == np.int64
    # every count may be NULL
    blob, off = np.frombuffer(text[100:160], dtype=np.uint8), np.array([0, 60], dtype=np.int64)
    ptrs, n1, n2 = [C.c_void_p() for _ in range(12)], C.c_int64(), C.c_int64()
    assert built_lib.bwtmi_index_map_batch(core._ctx, core._h, blob.ctypes.data_as(C.c_void_p),
                                           off.ctypes.data_as(C.c_void_p), 1, 19, 0, 0, 0, None,
                                           *[C.byref(p) for p in ptrs], C.byref(n1), C.byref(n2), None, None, None,
                                           None) == 0
    assert n1.value >= 1 and n2.value >= 1
    for p in ptrs:
        built_lib.bwtmi_free(p)
    # a chain through the whole text by the index method that only needs a context
    got = core.chain_anchors([0, 2], [0, 30], [0, 30], [20, 20], min_score=1)
    assert got["score"].tolist() == [40] and got["member"].tolist() == [0, 1]
