"""BWTCore.locate_batch / bwtmi_index_locate_batch: batched device locate with
up to 3 substitutions on one or both strands, against a brute-force
restatement of the contract (include/bwtmi.h) written here: a numpy sliding
compare, column by column, with the '$' rule, the reverse complement, the
order and the palindrome rule."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_COMP = np.arange(256, dtype=np.uint8)
for _a, _b in ("AT", "TA", "CG", "GC"):
    _COMP[ord(_a)] = ord(_b)


def _b(p):
    return p.encode() if isinstance(p, str) else bytes(p)


def revcomp(p: bytes) -> bytes:
    return _COMP[np.frombuffer(p, dtype=np.uint8)][::-1].tobytes()


def _windows(T: np.ndarray, q: bytes, k: int):
    """(positions, distances) of the windows of T within k substitutions of q,
    none of them on a '$' of T."""
    n, m = T.size, len(q)
    if m > n:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    W = n - m + 1
    d = np.zeros(W, dtype=np.int64)
    bad = np.zeros(W, dtype=bool)
    for i, ch in enumerate(q):
        col = T[i:i + W]
        ne = col != ch
        d += ne
        bad |= ne & (col == ord("$"))
    ok = (d <= k) & ~bad
    return np.nonzero(ok)[0].astype(np.int64), d[ok]


def oracle_one(T: np.ndarray, p: bytes, k: int, both: bool):
    pos, d = _windows(T, p, k)
    strand = np.zeros(pos.size, dtype=np.int64)
    rc = revcomp(p)
    if both and rc != p:
        pos2, d2 = _windows(T, rc, k)
        pos, d = np.concatenate([pos, pos2]), np.concatenate([d, d2])
        strand = np.concatenate([strand, np.ones(pos2.size, dtype=np.int64)])
    order = np.lexsort((strand, pos))
    return pos[order], d[order], strand[order]


def oracle(text: bytes, pats, k: int, both: bool):
    T = np.frombuffer(text, dtype=np.uint8)
    return [oracle_one(T, _b(p), k, both) for p in pats]


def check_against_oracle(core, text, pats, k, both, **kw):
    res = core.locate_batch(pats, max_mismatches=k, both_strands=both, **kw)
    want = oracle(text, pats, k, both)
    assert res.offsets.dtype == np.int64 and res.positions.dtype == np.int64
    assert res.mismatches.dtype == np.uint8 and res.strand.dtype == np.uint8
    assert res.offsets.size == len(pats) + 1 and res.offsets[0] == 0
    assert res.offsets[-1] == res.positions.size == res.mismatches.size == res.strand.size
    assert res.offsets.tolist() == np.concatenate([[0], np.cumsum([w[0].size for w in want])]).tolist()
    for i, (pos, d, s) in enumerate(want):
        gp, gd, gs = res[i]
        assert gp.tolist() == pos.tolist(), (i, pats[i], k, both)
        assert gd.tolist() == d.tolist(), (i, pats[i], k, both)
        assert gs.tolist() == s.tolist(), (i, pats[i], k, both)
    return res


def _random_dna(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].copy()


def _mutate(rng, seg: np.ndarray, nsub: int) -> np.ndarray:
    seg = seg.copy()
    for i in rng.choice(seg.size, size=min(nsub, seg.size), replace=False):
        seg[i] = rng.choice([c for c in b"ACGT" if c != seg[i]])
    return seg


@pytest.fixture(scope="module")
def texts(gpu_ctx):
    """name -> (text bytes, BWTCore): a random ACGT text of 3,000 bp with planted
    near-copies (one of them reverse-complemented), and the same with N runs
    and an R / Y (the byte-Occ rank path)."""
    from bwtmi import BWTCore
    rng = np.random.default_rng(20261020)
    a = _random_dna(rng, 3000)
    a[1500:1700] = _mutate(rng, a[100:300], 2)
    a[2300:2500] = _mutate(rng, np.frombuffer(revcomp(a[100:300].tobytes()), dtype=np.uint8), 3)
    a[2900:2964] = _mutate(rng, a[700:764], 1)
    acgt = a.tobytes() + b"$"
    g = a.copy()
    g[400:420] = ord("N")
    g[1600:1603] = ord("N")
    g[2000] = ord("R")
    g[2001] = ord("Y")
    g[2990:3000] = ord("N")
    gaps = g.tobytes() + b"$"
    out = {}
    for name, t in (("acgt", acgt), ("gaps", gaps)):
        out[name] = (t, BWTCore(t, build_kmer=False))
    return out


# ------------------------------------------------------------------ 1. exact
@pytest.mark.parametrize("cfg", ["acgt", "gaps", "acgt-fm-bytes"])
def test_exact_equals_locate_positions(texts, cfg):
    from bwtmi import _lib
    text, core = texts[cfg.split("-")[0]]
    s = text.decode()
    pats = sorted({s[i:i + m] for m in range(1, 7) for i in range(len(s) - 1 - m + 1)})
    pats += ["ACGTTGCATTAGGC" * 3, "NNNNNNNNNNNNNNNNNNNNN", "RYR", "X", "acgt",   # absent
             "$", "A$", "$A", "C$A", s[-2:], s[-7:], s[-40:]]                   # '$' inside / the sentinel last
    with _lib.knobs(FM_BYTES=int(cfg.endswith("fm-bytes"))):
        res = core.locate_batch(pats)
        assert not res.mismatches.any() and not res.strand.any()
        for i, p in enumerate(pats):
            assert res[i][0].tolist() == core.locate_positions(p), p
    assert res.offsets[-1] == res.positions.size


# ------------------------------------------------------------------ 2. parity
def _parity_patterns(rng, T, k, lengths=(2, 3, 4, 8, 9, 16, 17, 33, 64, 200)):
    """Pieces of the `texts` fixture's text (its planted copies, the N run, the
    end, random places) with 0 .. k + 1 substitutions, some reverse-complemented,
    and one random pattern per length."""
    pats = []
    for m in lengths:
        if m < k + 1:
            continue
        starts = [100, 1500 + (200 - m) // 2, 2300, 395, 2990 - m // 2] + rng.integers(0, T.size - 1 - m, 3).tolist()
        for j, st in enumerate(starts):
            st = min(st, T.size - 1 - m)
            seg = _mutate(rng, T[st:st + m], j % (k + 2))      # 0 .. k + 1 substitutions
            pats.append(seg.tobytes())
            if j % 3 == 0:
                pats.append(revcomp(seg.tobytes()))
        pats.append(_random_dna(rng, m).tobytes())
    return pats


@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("k", [0, 1, 2, 3])
@pytest.mark.parametrize("name", ["acgt", "gaps"])
def test_brute_force_parity(texts, name, k, both):
    text, core = texts[name]
    T = np.frombuffer(text, dtype=np.uint8)
    rng = np.random.default_rng(1000 + 10 * k + int(both))
    pats = _parity_patterns(rng, T, k)
    res = check_against_oracle(core, text, pats, k, both)
    assert res.positions.size > len(pats) // 2      # the cases are not vacuous
    if k and both:
        assert res.mismatches.max() == k and res.strand.any()


@pytest.mark.parametrize("sa,occ", [(1, 1), (7, 16), (33, 100), (1000, 2048)])
def test_sample_rates_do_not_change_hits(texts, sa, occ):
    """The hits do not depend on the index's sample rates: the gap text (seed
    search over the byte Occ, d_rank with a block of occ bytes) and the ACGT
    text under BWTMI_FM_BYTES=1, rebuilt at other rates, against the brute
    force, which knows no rates."""
    from bwtmi import BWTCore, _lib
    rng = np.random.default_rng(4000 + sa)
    for name, fm_bytes in (("gaps", 0), ("acgt", 1)):
        text = texts[name][0]
        pats = _parity_patterns(rng, np.frombuffer(text, dtype=np.uint8), 1, lengths=(4, 33))
        assert 20 <= len(pats) <= 30
        core = BWTCore(text, sa, occ, build_kmer=False)
        with _lib.knobs(FM_BYTES=fm_bytes):
            res = check_against_oracle(core, text, pats, 1, True)
        assert res.positions.size > len(pats) // 2 and res.strand.any()


# ------------------------------------------------------------------ 3. dedup
@pytest.mark.parametrize("unit,pat", [("A", "AAAAAAAA"), ("AC", "ACACACAC")])
def test_every_window_reported_once(gpu_ctx, unit, pat):
    from bwtmi import BWTCore
    text = (unit * (5000 // len(unit))).encode() + b"$"
    core = BWTCore(text, build_kmer=False)
    want = list(range(0, 5000 - 8 + 1, len(unit)))
    assert want[-1] in (4992,) and (unit != "A" or len(want) == 4993)
    for k in (1, 2, 3):
        res = core.locate_batch([pat], max_mismatches=k)
        pos, d, s = res[0]
        exact = pos[d == 0]
        assert exact.tolist() == want, k
        assert np.all(np.diff(pos) > 0)          # each position once, ascending
        check_against_oracle(core, text, [pat], k, False)


# ------------------------------------------------------------------ 4. edges
def test_edges(gpu_ctx, built_lib):
    from bwtmi import BWTCore
    from bwtmi._lib import BwtmiError
    text = b"GGGACGTTAGCATCGATCGGATTACAGCTAGCTAGGATCCAAGTTTTACGT$"
    n = len(text)
    core = BWTCore(text, build_kmer=False)
    # m = k + 1: every piece one byte
    for k in (0, 1, 2, 3):
        pats = ["ACGT"[:k + 1], "TTTT"[:k + 1], "G" * (k + 1), "N" * (k + 1)]
        check_against_oracle(core, text, pats, k, True)
    # m = k, the empty pattern, k outside 0..3: errors, never an empty result
    for pats, k in ((["AC"], 2), (["ACG", "AC"], 3), ([""], 0), (["ACGT", ""], 1), (["ACGTACGT"], 4),
                    (["ACGTACGT"], -1), (["A" * 1025], 0)):
        with pytest.raises(ValueError):
            core.locate_batch(pats, max_mismatches=k)
    assert isinstance(BwtmiError("x"), RuntimeError)
    with pytest.raises(ValueError):
        core.locate_batch(["ACGT"], max_candidates=0)
    # the longest supported pattern, and one longer than the text: legal, no hits
    res = check_against_oracle(core, text, ["A" * 1024, text.decode() + "A", "ACGT" * 20], 3, True)
    assert res.positions.size == 0
    assert core.locate_batch([]).offsets.tolist() == [0]
    # hits at position 0 and at n - 1 - m
    res = check_against_oracle(core, text, ["GGGACG", "TTACGT", "GGGTCG", "TTACGA"], 1, False)
    assert res[0][0].tolist() == [0] and res[1][0].tolist() == [n - 1 - 6]
    assert res[2][0].tolist() == [0] and res[3][0].tolist() == [n - 1 - 6]
    # seeds whose implied start is negative ("GGGA" at 0 as the second piece) or
    # whose window passes n ("ACGT" at n - 5 as the first piece)
    res = check_against_oracle(core, text, ["TTTTGGGA", "ACGTAAAA", "CAGGGA", "ACGTAC"], 1, False)
    assert res.positions.size == 0
    # the sentinel is never substituted; spelled out it matches
    res = check_against_oracle(core, text, ["TACGTA", "TACGT$", "ACGTAA"], 2, False)
    assert text[n - 6:] == b"TACGT$" and n - 6 not in res[0][0].tolist() and res[0][0].size
    assert res[1][0].tolist()[-1] == n - 6 and res[1][1].tolist()[-1] == 0
    assert core.locate_batch(["TACGT$"])[0][0].tolist() == [n - 6]
    # the text "$" alone
    one = BWTCore(b"$", build_kmer=False)
    res = check_against_oracle(one, b"$", ["$", "A", "AC"], 0, True)
    assert res.offsets.tolist() == [0, 1, 1, 1]
    check_against_oracle(one, b"$", ["A", "$"], 0, False)
    assert one.locate_batch(["AA"], max_mismatches=1).positions.size == 0


def test_inner_sentinel_is_never_bridged(gpu_ctx):
    from bwtmi import BWTCore
    text = b"AAAACCCC$GGGGTTTT$"
    core = BWTCore(text, build_kmer=False)
    for k in (1, 2, 3):
        res = check_against_oracle(core, text, ["CCCCAGGGG", "CCCC$GGGG", "ACCCCGGGG", "CCC$GGG", "CCCAGGG"], k, True)
        assert res[0][0].size == 0 and res[1][0].tolist() == [4] and res[1][1].tolist() == [0]


def test_c_abi_reports_argument_errors(gpu_ctx, built_lib, texts):
    _, core = texts["acgt"]
    blob = np.frombuffer(b"ACGTAC", dtype=np.uint8)
    ptrs = [C.c_void_p() for _ in range(4)]
    nh = C.c_int64(-7)

    def call(off, k, flags=0, cap=0):
        off = np.asarray(off, dtype=np.int64)
        return built_lib.bwtmi_index_locate_batch(core._ctx, core._h, blob.ctypes.data_as(C.c_void_p),
                                                  off.ctypes.data_as(C.c_void_p), off.size - 1, k, flags, cap,
                                                  *[C.byref(p) for p in ptrs], C.byref(nh), None)
    for off, k, flags in (([0, 4, 6], 4, 0), ([0, 4, 4], 0, 0), ([0, 4, 6], 2, 0), ([0, 4, 6], 0, 2)):
        assert call(off, k, flags) == -1            # BWTMI_E_ARG
        assert built_lib.bwtmi_last_error()
        assert all(p.value is None for p in ptrs) and nh.value == 0
    assert call([0, 4, 6], 1, 1) == 0
    off_out = np.ctypeslib.as_array(C.cast(ptrs[0], C.POINTER(C.c_int64)), shape=(3,)).copy()
    assert off_out[0] == 0 and off_out[2] == nh.value >= 1
    for p in ptrs:
        built_lib.bwtmi_free(p)


# ------------------------------------------------------------------ 5. strands
def test_strands(gpu_ctx, texts):
    text, core = texts["gaps"]
    res = check_against_oracle(core, text, ["ACGT", "AATT", "AAC", "GTT", "ANC", "GNT", "NNNN", "RY"], 1, True)
    assert not res[0][2].any() and not res[1][2].any()        # own reverse complements: '+' only
    minus_aac = res[2][0][res[2][2] == 1].tolist(), res[2][1][res[2][2] == 1].tolist()
    plus_gtt = res[3][0][res[3][2] == 0].tolist(), res[3][1][res[3][2] == 0].tolist()
    assert minus_aac == plus_gtt and minus_aac[0]
    assert res[4][0][res[4][2] == 1].tolist() == res[5][0][res[5][2] == 0].tolist()     # N maps to N
    assert not res[6][2].any() and res[6][0].size
    # one position within k on both strands: both rows, '+' first
    from bwtmi import BWTCore
    t2 = b"TTGGACGTCCAA$"
    c2 = BWTCore(t2, build_kmer=False)
    r2 = check_against_oracle(c2, t2, ["ACGA"], 1, True)     # "ACGT" is 1 off "ACGA" and 1 off "TCGT"
    at4 = r2[0][0] == 4
    assert r2[0][2][at4].tolist() == [0, 1] and r2[0][1][at4].tolist() == [1, 1]


# ------------------------------------------------------------------ 6. cap
def test_candidate_cap(gpu_ctx):
    from bwtmi import BWTCore
    from bwtmi._lib import BwtmiError
    text = b"A" * 4096 + b"$"
    core = BWTCore(text, build_kmer=False)
    with pytest.raises(BwtmiError, match="8186"):
        core.locate_batch(["AAAAAAAA"], max_mismatches=1, max_candidates=8185)
    res = check_against_oracle(core, text, ["AAAAAAAA"], 1, False, max_candidates=8186)
    assert res.positions.size == 4089 and res.candidates == 8186
    assert core.locate_batch(["AAAAAAAA"], max_mismatches=1).positions.size == 4089      # the default cap


# ------------------------------------------------------------------ 7. batch width
def test_all_motifs_exact(gpu_ctx):
    from bwtmi import BWTCore, MotifUtils, synth
    text = synth.generate_contig(20_000, 3) + b"$"
    core = BWTCore(text, build_kmer=False)
    pats = [m for k in range(1, 11) for m in MotifUtils.enumerate_motifs(k)]
    assert len(pats) == 145338
    iv = core.backward_search_batch(pats)
    width = np.where(iv[:, 0] >= 0, iv[:, 1] - iv[:, 0] + 1, 0)
    res = core.locate_batch(pats)
    assert np.diff(res.offsets).tolist() == width.tolist()
    sa = core.suffix_array.astype(np.int64)
    want = np.concatenate([np.sort(sa[sp:ep + 1]) for (sp, ep), w in zip(iv.tolist(), width.tolist()) if w])
    assert res.positions.tolist() == want.tolist()
    assert not res.mismatches.any() and not res.strand.any()
    assert (width == 0).sum() > len(pats) // 2       # most patterns are empty


# ------------------------------------------------------------------ 8. many tiles
def test_megabase_both_strands(gpu_ctx):
    from bwtmi import BWTCore, synth
    text = synth.generate_contig(1_000_000, 7) + b"$"
    T = np.frombuffer(text, dtype=np.uint8)
    core = BWTCore(text, build_kmer=False)
    rng = np.random.default_rng(8)
    k, m, npat = 2, 24, 2000
    origin = rng.integers(0, T.size - 1 - m, npat)
    pats, planted = [], []
    for i, st in enumerate(origin.tolist()):
        seg = T[st:st + m]
        ok = np.isin(seg, np.frombuffer(b"ACGT", dtype=np.uint8)).all()
        q = _mutate(rng, seg, int(rng.integers(0, k + 1))) if ok else seg.copy()
        d = int((q != seg).sum())
        p = q.tobytes()
        if i % 2:
            p = revcomp(p)
        pats.append(p)
        planted.append((st, i % 2 if revcomp(p) != p else 0, d))
    res = core.locate_batch(pats, max_mismatches=k, both_strands=True)
    assert res.offsets[-1] == res.positions.size >= npat
    # every hit re-verifies with its stated distance; keys strictly increase per pattern
    pid = np.repeat(np.arange(npat), np.diff(res.offsets))
    P = np.frombuffer(b"".join(pats), dtype=np.uint8).reshape(npat, m)
    R = np.frombuffer(b"".join(revcomp(p) for p in pats), dtype=np.uint8).reshape(npat, m)
    Q = np.where(res.strand[:, None] == 0, P[pid], R[pid])
    assert res.positions.min() >= 0 and res.positions.max() + m <= T.size
    win = T[res.positions[:, None] + np.arange(m)[None, :]]
    assert ((win != Q).sum(axis=1) == res.mismatches).all() and res.mismatches.max() <= k
    assert not ((win != Q) & (win == ord("$"))).any()
    key = (pid.astype(np.int64) << 40) | (res.positions << 1) | res.strand
    assert np.all(np.diff(key) > 0)
    have = set(zip(pid.tolist(), res.positions.tolist(), res.strand.tolist(), res.mismatches.tolist()))
    for i, (st, s, d) in enumerate(planted):
        assert (i, st, s, d) in have, (i, st, s, d)
    # the exact '+' subset is locate_positions
    for i in range(0, npat, 97):
        pos, d, s = res[i]
        assert pos[(d == 0) & (s == 0)].tolist() == core.locate_positions(pats[i].decode()), i
    # the full list of a seeded 16 of them against the brute force
    for i in np.random.default_rng(16).choice(npat, 16, replace=False).tolist():
        pos, d, s = oracle_one(T, pats[i], k, True)
        gp, gd, gs = res[i]
        assert (gp.tolist(), gd.tolist(), gs.tolist()) == (pos.tolist(), d.tolist(), s.tolist()), i
