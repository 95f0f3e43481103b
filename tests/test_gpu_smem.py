"""BWTCore.smem_batch / bwtmi_index_smem_batch: batched SMEM seeding of reads
on one or both strands, against a brute-force restatement of the contract
(include/bwtmi.h) written here: matching statistics by repeated bytes.find
(l(e) <= l(e-1) + 1 bounds the work), the SMEM rule on them, occurrences by a
find loop, the reverse complement from a byte table, work = the sum of l."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _b(q):
    return q.encode() if isinstance(q, str) else bytes(q)


def revcomp(q: bytes) -> bytes:
    return q.translate(_COMP)[::-1]


# ------------------------------------------------------------------ the oracle
class Oracle:
    """The contract over one text; l(e) and the occurrence lists are computed
    once per string and shared by every test that asks again."""

    def __init__(self, text: bytes):
        self.T = bytes(text)
        self._ms, self._occ = {}, {}

    def ms(self, Q: bytes):
        got = self._ms.get(Q)
        if got is None:
            got, l, at = [0] * (len(Q) + 2), 0, 0      # Q[e-1-l, e-1) occurs at `at`
            for e in range(1, len(Q) + 1):
                l += 1
                if self.T[at:at + l] != Q[e - l:e]:     # (else it simply goes on: no search needed)
                    at = self.T.find(Q[e - l:e])
                    while at < 0 and l:
                        l -= 1
                        at = self.T.find(Q[e - l:e])
                got[e] = l
            self._ms[Q] = got
        return got

    def occurrences(self, s: bytes):
        got = self._occ.get(s)
        if got is None:
            got, at = [], self.T.find(s)
            while at >= 0:
                got.append(at)
                at = self.T.find(s, at + 1)
            self._occ[s] = got
        return got

    def strand_smems(self, Q: bytes, min_len: int):
        ell, m = self.ms(Q), len(Q)
        return [(e - ell[e], e) for e in range(1, m + 1)
                if ell[e] >= min_len and (e == m or ell[e + 1] <= ell[e])]

    def query(self, q: bytes, min_len: int, both: bool):
        """(rows, work): rows (qstart, qend, strand, occurrences) by (strand, qstart)."""
        m = len(q)
        rows = [(s, e, 0, self.occurrences(q[s:e])) for s, e in self.strand_smems(q, min_len)]
        work = sum(self.ms(q))
        rc = revcomp(q)
        if both and rc != q:
            minus = [(m - e, m - s, 1, self.occurrences(rc[s:e])) for s, e in self.strand_smems(rc, min_len)]
            rows += sorted(minus, key=lambda r: r[0])
            work += sum(self.ms(rc))
        return rows, work

    def batch(self, queries, min_len=1, both=False, max_occ=1024):
        """The call's expected arrays, as a dict of the SmemResult fields."""
        off, qs, qe, st, cnt, poff, pos, work = [0], [], [], [], [], [0], [], 0
        for q in queries:
            rows, w = self.query(_b(q), min_len, both)
            work += w
            for s, e, strand, occ in rows:
                qs.append(s)
                qe.append(e)
                st.append(strand)
                cnt.append(len(occ))
                if len(occ) <= max_occ:
                    pos += occ
                poff.append(len(pos))
            off.append(len(qs))
        return {"offsets": np.array(off, np.int64), "qstart": np.array(qs, np.int32), "qend": np.array(qe, np.int32),
                "strand": np.array(st, np.uint8), "count": np.array(cnt, np.int64),
                "pos_offsets": np.array(poff, np.int64), "positions": np.array(pos, np.int64),
                "positions_total": len(pos), "work": work}


_FIELDS = ("offsets", "qstart", "qend", "strand", "count", "pos_offsets", "positions")


def assert_equal(res, want, what=None):
    for f in _FIELDS:
        got = getattr(res, f)
        assert got.dtype == want[f].dtype, (f, got.dtype, what)
        assert got.shape == want[f].shape and got.tolist() == want[f].tolist(), (f, what)
    assert res.positions_total == want["positions_total"], what
    assert res.work == want["work"], what


def check(core, orc, queries, min_len=1, both=False, max_occ=None, **kw):
    res = core.smem_batch(queries, min_len=min_len, both_strands=both, max_occ=max_occ, **kw)
    want = orc.batch(queries, min_len, both, 1024 if max_occ is None else max_occ)
    assert_equal(res, want, (min_len, both, max_occ))
    return res, want


# ------------------------------------------------------------------ fixtures
def _random_dna(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].copy()


def _mutate(rng, seg: np.ndarray, nsub: int) -> np.ndarray:
    seg = seg.copy()
    for i in rng.choice(seg.size, size=min(nsub, seg.size), replace=False):
        seg[i] = rng.choice([c for c in b"ACGT" if c != seg[i]])
    return seg


def _build_texts():
    """A random ACGT text of 3,000 bp with planted near-copies (one of them
    reverse-complemented) plus '$', and the same with N runs and an R / Y (the
    byte-Occ rank path): the texts of tests/test_gpu_locate.py."""
    rng = np.random.default_rng(20261020)
    a = _random_dna(rng, 3000)
    a[1500:1700] = _mutate(rng, a[100:300], 2)
    a[2300:2500] = _mutate(rng, np.frombuffer(revcomp(a[100:300].tobytes()), dtype=np.uint8), 3)
    a[2900:2964] = _mutate(rng, a[700:764], 1)
    g = a.copy()
    g[400:420] = ord("N")
    g[1600:1603] = ord("N")
    g[2000] = ord("R")
    g[2001] = ord("Y")
    g[2990:3000] = ord("N")
    return {"acgt": a.tobytes() + b"$", "gaps": g.tobytes() + b"$"}


def _queries(text: bytes):
    """Every length at which a wave or a workgroup of ends fills up, random and
    cut from the text; reads with substitutions, some reverse-complemented; N,
    '$', lower case and an absent byte."""
    rng = np.random.default_rng(77)
    T = np.frombuffer(text, dtype=np.uint8)
    out = []
    for m in (1, 2, 3, 63, 64, 65, 127, 128, 129, 300, 1024):
        out.append(_random_dna(rng, m).tobytes())
        st = int(rng.integers(0, T.size - 1 - m))
        out.append(text[st:st + m])
    for j, st in enumerate((100, 130, 1520, 2310, 700, 2850) + tuple(rng.integers(0, 2800, 4).tolist())):
        read = _mutate(rng, T[st:st + 150], 3).tobytes()      # (an N of the text may be "mutated" too)
        out.append(revcomp(read) if j % 2 else read)
    # the longest stretch the planted copy at 1500 shares with its source at 100: occurs twice
    same = np.concatenate([[False], T[100:300] == T[1500:1700], [False]])
    edges = np.flatnonzero(np.diff(same.astype(np.int8)))
    ln, at = max((b - a, a) for a, b in zip(edges[::2].tolist(), edges[1::2].tolist()))
    assert ln >= 20
    out.append(text[100 + at:100 + at + ln])
    out += [text[380:530], text[1590:1620], b"ACGTNNACGTACGTACGNNNNNNNNNNNNNNNNNNNNNNA",     # N inside
            text[-40:], text[-1:], b"A$", b"$A", text[-7:-1] + b"$$",                       # the sentinel
            b"acgtacgtacgtacgtacgtacgtacgt", b"n", text[200:260].lower(),                   # lower case: absent
            text[900:930] + b"X" + text[931:960], b"X", b"RYR", b"ACGT", b"AATT"]
    return out


@pytest.fixture(scope="module")
def texts(gpu_ctx):
    """name -> (text, BWTCore, Oracle, queries)"""
    from bwtmi import BWTCore
    out = {}
    for name, t in _build_texts().items():
        out[name] = (t, BWTCore(t, build_kmer=False), Oracle(t), _queries(t))
    return out


# ------------------------------------------------------------------ 1. the three rank paths
@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("min_len", [1, 5, 12, 20])
@pytest.mark.parametrize("cfg", ["acgt", "gaps", "acgt-fm-bytes"])
def test_brute_force_parity(texts, cfg, min_len, both):
    from bwtmi import _lib
    text, core, orc, queries = texts[cfg.split("-")[0]]
    with _lib.knobs(FM_BYTES=int(cfg.endswith("fm-bytes"))):
        res, want = check(core, orc, queries, min_len, both)
    # the run is not vacuous
    per_query = np.diff(want["offsets"])
    assert (per_query == 0).any() and want["count"].max() > 1 and want["qstart"].size > len(queries) // 2
    assert (want["strand"] == 0).any() and (not both or (want["strand"] == 1).any())
    assert want["work"] > 1024 * 1024 // 4           # the 1024 bp cut alone: m (m + 1) / 2
    if min_len == 1:
        assert want["positions"].size > 1000
    # what the arrays say of themselves
    assert np.all(res.qend - res.qstart >= min_len)
    assert np.all(np.diff(res.pos_offsets) == np.where(res.count <= 1024, res.count, 0))


# ------------------------------------------------------------------ 2. homopolymer
def test_homopolymer(gpu_ctx):
    from bwtmi import BWTCore
    text = b"A" * 200 + b"$"
    core, orc = BWTCore(text, build_kmer=False), Oracle(text)
    res, _ = check(core, orc, ["A" * 64])
    assert (res.qstart.tolist(), res.qend.tolist(), res.count.tolist()) == ([0], [64], [137])
    assert res.positions.tolist() == list(range(137)) and res.work == 64 * 65 // 2
    res, _ = check(core, orc, ["A" * 250])
    assert res.qstart.tolist() == list(range(51)) and res.qend.tolist() == list(range(200, 251))
    assert res.count.tolist() == [1] * 51 and res.positions.tolist() == [0] * 51
    res, _ = check(core, orc, ["A" * 64 + "C" + "A" * 10])
    assert list(zip(res.qstart.tolist(), res.qend.tolist())) == [(0, 64), (65, 75)]
    res, _ = check(core, orc, ["A" * 64], max_occ=137)
    assert res.positions.tolist() == list(range(137)) and res.positions_total == 137
    res, _ = check(core, orc, ["A" * 64], max_occ=136)
    assert res.count.tolist() == [137] and res.positions.size == 0 and res.pos_offsets.tolist() == [0, 0]
    assert res.positions_total == 0
    # min_len above m, and above every l: no SMEMs, the work is still done
    res, _ = check(core, orc, ["AAAA", "A" * 250], min_len=201)
    assert res.offsets.tolist() == [0, 0, 0] and res.work == 10 + sum(min(e, 200) for e in range(1, 251))


def test_no_match_wraps_round_the_end(gpu_ctx):
    """The rank step alone would find '$' + the text's first bytes (a cyclic
    match); the contract is plain substring equality.  Both rank paths, and a
    text whose last byte also occurs inside it."""
    from bwtmi import BWTCore
    for text in (b"TACGTTAGCATCGATTACA$", b"TACGNTAGCATCGATTACA$", b"AAAACCCC$GGGGTTTT$"):
        core, orc = BWTCore(text, build_kmer=False), Oracle(text)
        queries = [b"$" + text[:4], text[-3:] + text[:3], b"$", text[-2:], b"A$T", b"CCCC$GGGG", b"$G", b"T$A",
                   text, text + text[:5]]
        for both in (False, True):
            res, want = check(core, orc, queries, 1, both)
        assert res[0][1].tolist()[:1] == [1] and res[8][3].tolist()[:1] == [1]      # '$' alone; the whole text, once


# ------------------------------------------------------------------ 3. packing
def test_short_queries_share_waves(texts):
    text, core, orc, _ = texts["gaps"]
    rng = np.random.default_rng(3)
    alphabet = np.frombuffer(b"ACGTN$RX", dtype=np.uint8)
    queries = [alphabet[rng.integers(0, alphabet.size, int(rng.integers(1, 4)))].tobytes() for _ in range(400)]
    for both in (False, True):
        res, _ = check(core, orc, queries, 1, both, max_occ=600)
        again = core.smem_batch(queries, min_len=1, both_strands=both, max_occ=600)
        for f in _FIELDS:
            assert getattr(res, f).tobytes() == getattr(again, f).tobytes(), f
        ones = [core.smem_batch([q], min_len=1, both_strands=both, max_occ=600) for q in queries]
        for f in ("qstart", "qend", "strand", "count", "positions"):
            assert getattr(res, f).tolist() == np.concatenate([getattr(o, f) for o in ones]).tolist(), f
        assert res.offsets.tolist() == np.concatenate([[0], np.cumsum([o.qstart.size for o in ones])]).tolist()
        assert res.pos_offsets.tolist() == np.concatenate([[0], np.cumsum(
            np.concatenate([np.diff(o.pos_offsets) for o in ones]))]).tolist()
        assert res.work == sum(o.work for o in ones) and res.positions_total == sum(o.positions_total for o in ones)
        assert (res.count > 600).any() and (np.diff(res.offsets) == 0).any()


# ------------------------------------------------------------------ 4. strands
def test_strands(texts):
    text, core, orc, _ = texts["acgt"]
    res, want = check(core, orc, ["ACGT", "AATT", "AAC", "GTT"], 1, True)
    assert not res[0][2].any() and not res[1][2].any()            # own reverse complements: '+' only
    assert res.work == sum(sum(orc.ms(q)) for q in (b"ACGT", b"AATT", b"AAC", b"GTT", b"GTT", b"AAC"))
    # the '-' SMEMs of AAC are the '+' SMEMs of GTT, mirrored, at the same forward positions
    qs, qe, st, cnt, pos = res[2]
    ps, pe, pst, pcnt, ppos = res[3]
    minus, plus = np.flatnonzero(st == 1), np.flatnonzero(pst == 0)
    assert minus.size == plus.size >= 1
    assert sorted(zip((3 - qe[minus]).tolist(), (3 - qs[minus]).tolist(), cnt[minus].tolist())) == \
        sorted(zip(ps[plus].tolist(), pe[plus].tolist(), pcnt[plus].tolist()))
    # text[2300:2500] is the reverse complement of text[100:300] with 3 substitutions: a read cut from
    # 100.. finds its longest '-' seed there, in its own coordinates, at a forward-text position
    read = text[120:270]
    res, _ = check(core, orc, [read], 20, True)
    qs, qe, st, cnt, pos = res[0]
    assert (qs[st == 0].tolist(), qe[st == 0].tolist()) == ([0], [150])
    assert (st == 1).any()
    for i in np.flatnonzero(st == 1).tolist():
        seed = revcomp(read[qs[i]:qe[i]])
        assert cnt[i] == len(pos[i]) >= 1
        for p in pos[i].tolist():
            assert text[p:p + len(seed)] == seed and 2300 <= p < 2500


# ------------------------------------------------------------------ 5. cap
def _raw_call(lib, core, queries, min_len=1, flags=0, max_occ=0, max_positions=0, off=None, want_total=True):
    blob = np.frombuffer(b"".join(queries) or b"\0", dtype=np.uint8)
    if off is None:
        off = np.concatenate([[0], np.cumsum([len(q) for q in queries])])
    off = np.asarray(off, dtype=np.int64)
    ptrs = [C.c_void_p(0xdead) for _ in range(7)]
    counts = [C.c_int64(-7) for _ in range(4)]       # nsmem, npos, positions_total, work
    rc = lib.bwtmi_index_smem_batch(core._ctx, core._h, blob.ctypes.data_as(C.c_void_p),
                                    off.ctypes.data_as(C.c_void_p), off.size - 1, min_len, flags, max_occ,
                                    max_positions, *[C.byref(p) for p in ptrs], *[C.byref(v) for v in counts])
    return rc, ptrs, [v.value for v in counts]


def test_position_cap(texts, built_lib):
    from bwtmi._lib import BwtmiError
    text, core, orc, queries = texts["acgt"]
    queries = queries[:30]
    want = orc.batch(queries, 5, True, 50)
    total = want["positions_total"]
    assert total > 100
    res, _ = check(core, orc, queries, 5, True, max_occ=50, max_positions=total)
    assert res.positions_total == total == res.positions.size
    with pytest.raises(BwtmiError, match=str(total)):
        core.smem_batch(queries, min_len=5, both_strands=True, max_occ=50, max_positions=total - 1)
    with pytest.raises(ValueError):
        core.smem_batch(queries, max_positions=0)
    with pytest.raises(ValueError):
        core.smem_batch(queries, max_occ=0)
    rc, ptrs, counts = _raw_call(built_lib, core, queries, 5, 1, 50, total - 1)
    assert rc != 0 and rc != -1 and str(total).encode() in built_lib.bwtmi_last_error()
    assert all(p.value is None for p in ptrs) and counts == [0, 0, total, 0]
    rc, ptrs, counts = _raw_call(built_lib, core, queries, 5, 1, 50, total)
    assert rc == 0 and counts == [want["qstart"].size, total, total, want["work"]]
    for p in ptrs:
        assert p.value is not None
        built_lib.bwtmi_free(p)


# ------------------------------------------------------------------ 6. arguments, raw C ABI
def test_c_abi_reports_argument_errors(texts, built_lib):
    text, core, orc, _ = texts["acgt"]
    ok = [b"ACGTAC", b"GG"]
    for queries, off, min_len, flags in ((ok, [0, 6, 6], 1, 0),            # an empty query
                                         ([b"A" * 1025], None, 1, 0),
                                         (ok, None, 0, 0), (ok, None, -3, 0),
                                         (ok, None, 1, 2), (ok, None, 1, 3)):
        rc, ptrs, counts = _raw_call(built_lib, core, queries, min_len, flags, off=off)
        assert rc == -1 and built_lib.bwtmi_last_error()                   # BWTMI_E_ARG
        assert all(p.value is None for p in ptrs) and counts == [0, 0, 0, 0]
    for queries, kw in (([""], {}), (["ACGT", ""], {}), (["A" * 1025], {}), (["ACGT"], {"min_len": 0})):
        with pytest.raises(ValueError):
            core.smem_batch(queries, **kw)
    # nq = 0: the empty result
    rc, ptrs, counts = _raw_call(built_lib, core, [])
    assert rc == 0 and counts == [0, 0, 0, 0] and all(p.value is not None for p in ptrs)
    assert C.cast(ptrs[0], C.POINTER(C.c_int64))[0] == 0 and C.cast(ptrs[5], C.POINTER(C.c_int64))[0] == 0
    for p in ptrs:
        built_lib.bwtmi_free(p)
    res = core.smem_batch([])
    assert res.offsets.tolist() == [0] and res.pos_offsets.tolist() == [0] and len(res) == 0
    assert res.offsets.dtype == np.int64 and res.qstart.dtype == np.int32 and res.strand.dtype == np.uint8
    # the longest query, and the last two counts may be NULL
    res, _ = check(core, orc, ["A" * 1024, text[:1024]], 12, True)
    blob = np.frombuffer(b"ACGT", dtype=np.uint8)
    off = np.array([0, 4], dtype=np.int64)
    ptrs, n1, n2 = [C.c_void_p() for _ in range(7)], C.c_int64(), C.c_int64()
    assert built_lib.bwtmi_index_smem_batch(core._ctx, core._h, blob.ctypes.data_as(C.c_void_p),
                                            off.ctypes.data_as(C.c_void_p), 1, 1, 0, 0, 0,
                                            *[C.byref(p) for p in ptrs], C.byref(n1), C.byref(n2), None, None) == 0
    assert n1.value == orc.batch([b"ACGT"])["qstart"].size
    for p in ptrs:
        built_lib.bwtmi_free(p)


# ------------------------------------------------------------------ 7. other index geometry
@pytest.mark.parametrize("occ", [1, 100])
def test_occ_block_sizes(texts, occ):
    """d_rank under the new kernel with an Occ block of 1 byte (no tail loop) and
    of 100 bytes (no power of two): the result knows no sample rates."""
    from bwtmi import BWTCore
    text, _, orc, queries = texts["gaps"]
    core = BWTCore(text, 7, occ, build_kmer=False)
    check(core, orc, queries, 12, True)


def test_long_contig_reads(gpu_ctx):
    """Positions past 2^16, several workgroups of lanes, a position key of more
    than one radix pass."""
    from bwtmi import BWTCore, synth
    text = synth.generate_contig(200_000, 5) + b"$"
    core, orc = BWTCore(text, build_kmer=False), Oracle(text)
    rng = np.random.default_rng(40)
    starts = np.sort(rng.integers(0, len(text) - 151, 40))
    reads = [text[s:s + 150] for s in starts.tolist()]
    reads = [revcomp(r) if i % 2 else r for i, r in enumerate(reads)]
    res, want = check(core, orc, reads, 19, True)
    assert res.positions.max() > 1 << 16 and res.qstart.size >= 40 and (res.strand == 1).any()
    assert res.work > 40 * 150 * 151 // 2
    for i, s in enumerate(starts.tolist()):
        qs, qe, st, cnt, pos = res[i]
        whole = np.flatnonzero((qs == 0) & (qe == 150) & (st == i % 2))
        assert whole.size == 1 and s in pos[whole[0]].tolist()
