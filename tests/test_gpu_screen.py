"""The device screen (csrc/nested.hip) on synthetic hit lists, output for output
against an all-pairs numpy reference.

bwtmi_screen_hits hands screen_hits_device a caller's hit list, so every branch
of the screen is selected by construction (and asserted to have run) instead of
by what a scanned text happens to contain: the 256- and 1024-thread segmented
workgroups, the per-level fallback, the thread-per-hit and wave-per-hit level
kernels, the decision rounds, the one-key and two-sort orders, the one- and
two-word record layouts, the multi-tile prefix max, the integer threshold
tests, the drop and the cut bits.

The reference below shares nothing with the device's windowing (no prefix max,
no segments, no buckets): levels in descending motif length, every hit of a
level against every kept span of a longer motif, the overlap ratio and the
motif ratio as float64 divisions against 0.1 / 0.3 / 0.5 / 0.8 as the reference
program writes them.  A CPU test holds it against oracle.post's
suppress_nested + dedup, so a disagreement on the GPU names the kernel.
"""
import contextlib
import ctypes as C
import functools
import re

import numpy as np
import pytest


# --------------------------------------------------------------------------
# reference
# --------------------------------------------------------------------------
def ref_kept(S, E, M):
    """kept[i]: hit i survives the nested suppression (bwt.py:3402-3497, thr 0.5)."""
    n = len(S)
    kept = np.zeros(n, dtype=bool)
    ks = np.empty(0, np.int64)   # kept spans of strictly longer motifs
    ke = np.empty(0, np.int64)
    km = np.empty(0, np.int64)
    for m in np.unique(M)[::-1]:
        idx = np.flatnonzero(M == m)
        nested = np.zeros(len(idx), dtype=bool)
        if len(ks):
            step = max(1, (1 << 22) // len(ks))
            for a in range(0, len(idx), step):
                c = idx[a:a + step]
                s, e = S[c][:, None], E[c][:, None]
                qi, ki = np.nonzero((ks[None, :] < e) & (ke[None, :] > s))   # the pairs with ov > 0
                sq, eq = S[c][qi], E[c][qi]
                ov = np.minimum(eq, ke[ki]) - np.maximum(sq, ks[ki])
                assert (ov > 0).all()
                frac = ov / (eq - sq)
                ratio = km[ki] / m
                thr = np.where(ratio >= 10, 0.1, np.where(ratio >= 5, 0.3, 0.5))
                hit = frac >= thr
                if m == 1:
                    hit |= (km[ki] > 1) & (frac >= 0.8)
                nested[a + qi[hit]] = True
        kept[idx] = ~nested
        new = idx[~nested]
        ks = np.concatenate([ks, S[new]])
        ke = np.concatenate([ke, E[new]])
        km = np.concatenate([km, M[new]])
    return kept


def ref_reach(s, e, m, mc):
    """screen_reach(s, e, max(1, m), mc, unit1_maximal=True) of common.h."""
    m = np.maximum(m, 1)
    mi = np.where(m >= 4, np.minimum(m // 2, 10), 1)
    ext = np.maximum(3 * m, 4 * mi)
    r = np.maximum(e, s + m * mc) + 2 * ext
    return np.where(m == 1, e, r)


def _isolated_before(s, e, m, mc):
    """fold_cut of common.h: s[k] - max_{j<k} reach(j) > max(1, m[k]) + 1 (k == 0: always)."""
    cut = np.ones(len(s), dtype=bool)
    if len(s) > 1:
        before = np.maximum.accumulate(ref_reach(s, e, m, mc))[:-1]
        cut[1:] = s[1:] - before > np.maximum(m[1:], 1) + 1
    return cut


def ref_rows(hits, mc):
    """(start, len, prim, cut) of the screened hits, drop off."""
    hits = np.asarray(hits, dtype=np.int64).reshape(-1, 5)
    S, E, M = hits[:, 0], hits[:, 1], hits[:, 3]
    k = ref_kept(S, E, M)
    s, e, m = S[k], E[k], M[k]
    o = np.lexsort((-m, e, s))
    s, e, m = s[o], e[o], m[o]
    if len(s):
        first = np.r_[True, (s[1:] != s[:-1]) | (e[1:] != e[:-1]) | (m[1:] != m[:-1])]
        s, e, m = s[first], e[first], m[first]
    cut = _isolated_before(s, e, m, mc)
    return np.stack([s, e - s, m, cut.astype(np.int64)], axis=1).reshape(-1, 4)


def ref_droppable(rows, mc):
    """The rule above k_drop_flags on the screened hits `rows`, with the true next
    kept hit: fails the final filter, out of every earlier hit's reach, and out of
    merging distance of the next hit."""
    s, ln, m = rows[:, 0], rows[:, 1], np.maximum(rows[:, 2], 1)
    e = s + ln
    passes = (ln // m >= mc) & (ln >= 6)
    after = np.ones(len(s), dtype=bool)
    if len(s) > 1:
        after[:-1] = s[1:] - e[:-1] > np.maximum(m[:-1], m[1:]) + 1
    return ~passes & _isolated_before(s, e, rows[:, 2], mc) & after


def _hits(start, end, prim, rng=None):
    """int64[k,5] hit rows; unit_len / copies as a scan would set them (the screen reads neither)."""
    start, end, prim = (np.asarray(x, dtype=np.int64) for x in (start, end, prim))
    h = np.zeros((len(start), 5), dtype=np.int64)
    h[:, 0], h[:, 1], h[:, 2], h[:, 3] = start, end, prim, prim
    h[:, 4] = (end - start) // np.maximum(prim, 1)
    if rng is not None:
        h = h[rng.permutation(len(h))]
    return h


# --------------------------------------------------------------------------
# families
# --------------------------------------------------------------------------
MOTIFS = {"mixed": (1, 2, 3, 5, 10, 11, 20, 50, 100), "two": (1, 7), "pow2": (1, 2, 4, 8, 16, 32, 64)}
SCALES = (2, 5, 30)
TEXTS = (200, 5_000, 100_000)
NS = (1, 2, 63, 64, 65, 511, 512, 513, 4095, 4097)


@functools.lru_cache(maxsize=None)
def random_hits(n, text_len, mset, scale):
    """n hits: motif lengths from the set, lengths exponential around m * scale; a
    fifth of them duplicates, half of those differing only in unit_len / copies."""
    rng = np.random.default_rng([n, text_len, sorted(MOTIFS).index(mset), scale])
    nd = (n + 3) // 5
    base = n - nd
    m = rng.choice(MOTIFS[mset], base).astype(np.int64)
    ln = np.minimum(1 + np.floor(rng.exponential(m * float(scale))).astype(np.int64), text_len)
    st = np.floor(rng.random(base) * (text_len - ln + 1)).astype(np.int64)
    h = np.zeros((n, 5), dtype=np.int64)
    h[:base] = _hits(st, st + ln, m)
    h[base:] = h[rng.integers(0, base, nd)]
    h[base + nd // 2:, 2] *= 2      # the same span found at a multiple of its unit
    h[base + nd // 2:, 4] //= 2
    h = h[rng.permutation(n)]
    h.setflags(write=False)
    return h


@functools.lru_cache(maxsize=None)
def random_ref(n, text_len, mset, scale, mc=3):
    r = ref_rows(random_hits(n, text_len, mset, scale), mc)
    r.setflags(write=False)
    return r


def _klass(M, m):
    """(p, q): the overlap fraction p / q at which a span of motif M nests one of motif m."""
    return (1, 10) if M >= 10 * m else (3, 10) if M >= 5 * m else (1, 2)


@functools.lru_cache(maxsize=None)
def threshold_family():
    """One isolated (nester, query) pair per 4000 bp region, the query's overlap the
    smallest integer on the class threshold and one below.  Returns the hits, the
    text length and per pair (m, M, query start, query length, main grid)."""
    cases = []
    for m in (1, 2, 3, 7):
        for M in (5 * m - 1, 5 * m, 10 * m - 1, 10 * m, 2 * m):
            p, q = _klass(M, m)
            for rl in (6, 10, 30, 97, 1000):
                ov = -(-p * rl // q)
                cases += [(m, M, rl, ov, True), (m, M, rl, ov - 1, True)]
    for M in (2, 4, 5, 10):
        for rl in (6, 10, 30, 97, 1000):
            ov = -(-4 * rl // 5)
            cases += [(1, M, rl, ov, False), (1, M, rl, ov - 1, False)]
    S, E, P, info = [], [], [], []
    for i, (m, M, rl, ov, main) in enumerate(cases):
        base = 4000 * i
        ns, ne = base + 1200, base + 2700
        qs = ne - ov if i % 2 == 0 else ns + ov - rl     # over the nester's right / left end
        S += [ns, qs]
        E += [ne, qs + rl]
        P += [M, m]
        info.append((m, M, qs, rl, main))
    return _hits(S, E, P, np.random.default_rng(7)), 4000 * len(cases), info


DOLLS = ((200, 40, 8, 2, 1), (500, 250, 100, 50, 20, 7, 3, 1), (640, 64, 60, 12, 6, 1), (90, 30, 10, 9, 3, 2, 1))


@functools.lru_cache(maxsize=None)
def doll_family(nstacks, cover):
    """Stacks of dolls: doll j straddles the end of doll j - 1 by just enough to be
    nested by it (a quarter of them one base short) and starts past doll j - 2, so
    each decision hangs on the one above.  cover: one motif-1 span over everything
    (it nests nothing and puts every stack into one segment).  Returns the hits,
    the text length and per stack the (start, len, prim) of its dolls."""
    rng = np.random.default_rng(11)
    S, E, P, stacks = [], [], [], []
    for k in range(nstacks):
        ms = DOLLS[k % len(DOLLS)]
        depth = int(rng.integers(1, len(ms) + 1))
        L = 600
        s, e, e_above = 2000 * k + 100, 2000 * k + 700, None
        dolls = [(s, L, ms[0])]
        for j in range(1, depth):
            L2 = L // 2
            p, q = _klass(ms[j - 1], ms[j])
            ov = -(-p * L2 // q) + (int(rng.integers(0, 2)) if rng.random() >= 0.25 else -1)
            s2 = e - ov
            assert ov <= L2 and (e_above is None or s2 >= e_above)
            e_above, s, e, L = e, s2, s2 + L2, L2
            dolls.append((s, L, ms[j]))
        stacks.append(dolls)
        for (a, ln, m) in dolls:
            S.append(a)
            E.append(a + ln)
            P.append(m)
    text_len = 2000 * nstacks + 100
    if cover:
        S.append(0)
        E.append(text_len)
        P.append(1)
    return _hits(S, E, P, rng), text_len, stacks


CHAIN_M = (1, 2, 3, 5, 11)


def _chain(base, L, rng):
    i = np.arange(L, dtype=np.int64)
    return base + 3 * i, base + 3 * i + 10, rng.choice(CHAIN_M, L)


@functools.lru_cache(maxsize=None)
def chain_family(L, off):
    """A chain of L overlapping hits (3i, 3i + 10, m_i) at rank `off` of the position
    order: `off` isolated hits (one segment each) before it, 300 hits in short
    segments after it."""
    rng = np.random.default_rng([L, off])
    j = np.arange(off, dtype=np.int64)
    S = [10 * j]
    E = [10 * j + rng.integers(2, 7, off)]
    P = [rng.choice((1, 2, 3), off)]
    base = 10 * off + 50
    cs, ce, cm = _chain(base, L, rng)
    S.append(cs)
    E.append(ce)
    P.append(cm)
    g = np.arange(300, dtype=np.int64)
    ps = base + 3 * L + 100 + 40 * (g // 3) + 5 * (g % 3)   # groups of three overlapping hits
    S.append(ps)
    E.append(ps + rng.integers(4, 30, 300))
    P.append(rng.choice((1, 2, 4, 9, 30), 300))
    S, E, P = (np.concatenate(x) for x in (S, E, P))
    return _hits(S, E, P, rng), int(E.max()) + 10


@functools.lru_cache(maxsize=None)
def large_level_family(with_chain):
    """70 000 disjoint motif-1 hits (one level above the wave kernel's 65536) under
    3000 random hits of longer motifs; with_chain: and a 5000 chain (one segment
    past the large workgroup: the screen falls back by itself)."""
    rng = np.random.default_rng(5)
    i = np.arange(70_000, dtype=np.int64)
    span = 8 * 70_000
    m = rng.choice((2, 3, 7, 12), 3000).astype(np.int64)
    ln = 1 + np.floor(rng.exponential(m * 5.0)).astype(np.int64)
    st = np.floor(rng.random(3000) * (span - ln + 1)).astype(np.int64)
    S, E, P = [8 * i, st], [8 * i + 6, st + ln], [np.ones(70_000, np.int64), m]
    text_len = span
    if with_chain:
        cs, ce, cm = _chain(span + 1000, 5000, rng)
        S.append(cs)
        E.append(ce)
        P.append(cm)
        text_len = int(ce.max()) + 10
    S, E, P = (np.concatenate(x) for x in (S, E, P))
    return _hits(S, E, P, rng), text_len


WALKS = (65, 128, 129, 300, 5000)


@functools.lru_cache(maxsize=None)
def walk_family(D):
    """A query whose only nester sits D ranks before it in the position order, the
    ranks between filled by spans that start after the nester and end before the
    query; and the mirror case, where a longer motif suppresses that nester and
    the query stays.  Returns the hits, the text length and the two queries."""
    S, E, P, queries = [], [], [], []
    for mirror, base in ((False, 1000), (True, 1000 + D + 3000)):
        s0 = base + D + 5
        queries.append((s0, 20, 2))
        j = np.arange(D - 1, dtype=np.int64)
        S += [base, s0] + list(base + 1 + j)
        E += [s0 + 25, s0 + 20] + list(base + 1 + j + 1 + j % 3)
        P += [30, 2] + list(np.array((1, 2, 3, 50))[j % 4])
        assert max(E[-(D - 1):]) <= s0
        if mirror:
            y = -(-(D + 30) // 10) + 1     # >= 0.1 of the nester, short of the query
            assert base + y <= s0
            S.append(base - 40)
            E.append(base + y)
            P.append(400)
    text_len = 1000 + 2 * D + 3000 + 1000
    return _hits(S, E, P, np.random.default_rng(D)), text_len, queries


WIDE_TEXT = 2 ** 32 - 2


def _both_ends(rng, n, text_len, motifs):
    """n ordinary hits, half within 200 kbp of either end of [0, text_len)."""
    m = rng.choice(motifs, n).astype(np.int64)
    ln = 1 + np.floor(rng.exponential(m * 5.0)).astype(np.int64)
    st = np.floor(rng.random(n) * (200_000 - ln)).astype(np.int64)
    st[n // 2:] += text_len - 200_000
    return st, st + ln, m


@functools.lru_cache(maxsize=None)
def wide_family(giant_m):
    """text_len 2^32 - 2, one span of 3e9 and a longest motif of 1000: 32 + 32 + 10
    key bits, two sorts, two-word records; about 2000 ordinary hits near both ends."""
    rng = np.random.default_rng([3, giant_m])
    s, e, m = _both_ends(rng, 2000, WIDE_TEXT, (1, 2, 3, 5, 10, 50, 200))
    S = np.r_[s, 1000, WIDE_TEXT - 5000, WIDE_TEXT - 700, 3]
    E = np.r_[e, 1000 + 3_000_000_000, WIDE_TEXT, WIDE_TEXT, 700]
    P = np.r_[m, giant_m, 1000, 3, 1000]
    return _hits(S, E, P, rng)


LAYOUTS = ((2 ** 21 - 1, 1023), (2 ** 21, 1023), (2 ** 21 - 1, 1024), (2 ** 20 - 1, 1024),   # 32, 33, 33, 32 bits
           (2 ** 20 - 1, 2047), (2 ** 20, 2047))                                              # 32, 33


@functools.lru_cache(maxsize=None)
def layout_family(maxlen, lmax):
    """bits(maxlen) + bits(lmax) + 1 on either side of 32 (one word per record or
    two), starts above 2^31, a hit with both the longest span and the longest motif."""
    rng = np.random.default_rng([maxlen, lmax])
    s, e, m = _both_ends(rng, 600, WIDE_TEXT, (1, 2, 3, 5, 10, 50, 200))
    top = WIDE_TEXT - 200_000 - 3 * maxlen
    S = np.r_[s, top, top + maxlen + 500, 100, WIDE_TEXT - 9]
    E = np.r_[e, top + maxlen, top + 2 * maxlen + 500, 100 + lmax * 3, WIDE_TEXT]
    P = np.r_[m, lmax, 1, lmax, 1]
    return _hits(S, E, P, rng)


@functools.lru_cache(maxsize=None)
def sparse_hits():
    """Mostly isolated short hits, a few close enough to merge or overlapping."""
    rng = np.random.default_rng(23)
    n = 3000
    gap = rng.choice((2, 3, 5, 9, 30, 60), n, p=(0.05, 0.05, 0.1, 0.1, 0.4, 0.3))
    ln = rng.integers(2, 14, n)
    st = np.cumsum(gap + 8) - 8
    st[rng.random(n) < 0.05] -= 6          # some overlap the hit before
    st = np.maximum(st, 0)
    h = _hits(st, st + ln, rng.choice((1, 2, 3, 4, 6), n), rng)
    h.setflags(write=False)
    return h, int((st + ln).max()) + 50


# --------------------------------------------------------------------------
# CPU: the reference against oracle.post, the families against their purpose
# --------------------------------------------------------------------------
def _oracle_rows(hits):
    from oracle import post
    pipe = post.Pipeline({}, {}, {}, 3)
    recs = [post.Rec(chrom="c", start=int(s), end=int(e), motif="A" * int(m), tier=2, confidence=0.95)
            for s, e, m in zip(hits[:, 0], hits[:, 1], hits[:, 3])]
    out = pipe.dedup(pipe.suppress_nested(recs, 0.5))
    return [(r.start, r.end - r.start, len(r.motif)) for r in out]


@pytest.mark.parametrize("n", [x for x in NS if x < 4000] + [1500])
def test_reference_matches_oracle(n):
    """The all-pairs reference == oracle.post suppress_nested (thr 0.5) + dedup on the random family."""
    combos = [(t, ms, sc) for t in TEXTS for ms in sorted(MOTIFS) for sc in SCALES]
    if n == 1500:
        combos = combos[::4]
    for text_len, mset, scale in combos:
        h = random_hits(n, text_len, mset, scale)
        got = [tuple(r) for r in random_ref(n, text_len, mset, scale)[:, :3].tolist()]
        assert got == _oracle_rows(h), (n, text_len, mset, scale)


def _present(rows, key):
    return bool(((rows[:, 0] == key[0]) & (rows[:, 1] == key[1]) & (rows[:, 2] == key[2])).any())


def _check_thresholds(rows, info):
    """Both outcomes in every (m, M) class of the main grid; below the class
    threshold kept, on it suppressed."""
    seen = {}
    for k, (m, M, qs, rl, main) in enumerate(info):
        kept = _present(rows, (qs, rl, m))
        if main:
            seen.setdefault((m, M), set()).add(kept)
            assert kept == (k % 2 == 1), (m, M, qs, rl)
        else:
            assert not kept, (m, M, qs, rl)    # 0.8 and just below: past the class threshold either way
    assert len(seen) == 20 and all(v == {True, False} for v in seen.values())


def _check_dolls(rows, stacks):
    """Deep stacks whose decisions alternate down to the last doll occur."""
    alternating = 0
    for dolls in stacks:
        kept = [_present(rows, d) for d in dolls]
        assert kept[0]
        if len(dolls) >= 5 and all(kept[j] != kept[j - 1] for j in range(1, len(dolls))):
            alternating += 1
    assert alternating >= 10


def test_families_reach_their_cases():
    """By the reference alone: the threshold family has both outcomes in every
    class, the doll stacks alternate, the far nester of the walk family decides
    its query.  (What the device tests then compare is not vacuous.)"""
    h, _, info = threshold_family()
    _check_thresholds(ref_rows(h, 3), info)
    for cover in (False, True):
        h, _, stacks = doll_family(300, cover)
        assert len(h) <= 4096
        _check_dolls(ref_rows(h, 3), stacks)
    for D in WALKS:
        h, _, (plain, mirror) = walk_family(D)
        rows = ref_rows(h, 3)
        assert not _present(rows, plain) and _present(rows, mirror)
        o = np.lexsort((-h[:, 3], h[:, 1] - h[:, 0], h[:, 0]))
        rank = {tuple(h[i, [0, 1, 3]]): r for r, i in enumerate(o)}
        assert rank[(plain[0], plain[0] + 20, 2)] - rank[(1000, plain[0] + 25, 30)] == D


# --------------------------------------------------------------------------
# GPU
# --------------------------------------------------------------------------
_SCREEN = re.compile(r"screen: (\d+) hits, (\d+) overflow windows, fallback (\d+)")


def _screen(ctx, hits, text_len, **kw):
    from bwtmi import _lib
    return _lib.screen_hits(ctx, hits, text_len, **kw)


def _screen_stats(capfd, ctx, hits, text_len, **kw):
    """rows and (hits, overflow windows, fallback) of the call's BWTMI_STATS line."""
    from bwtmi import _lib
    capfd.readouterr()
    with _lib.knobs(STATS=1):
        rows = _lib.screen_hits(ctx, hits, text_len, **kw)
    found = _SCREEN.findall(capfd.readouterr().err)
    assert len(found) == 1, found
    n, ovf, fb = (int(x) for x in found[0])
    assert n == len(hits)
    return rows, ovf, fb


@contextlib.contextmanager
def _kernels(ctx):
    """The kernel statistics of the launches made inside the block."""
    from bwtmi import _lib
    out = {}
    _lib.kernel_stats_filter(ctx, "")
    _lib.kernel_stats(ctx, enable=True, reset=True)
    try:
        yield out
    finally:
        out.update(_lib.kernel_stats(ctx, enable=False, reset=True))


def _same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, (what, int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("n", NS)
def test_random_lists(gpu_ctx, n):
    """Every text length, motif set and length scale; segmented and per-level
    screens; the longest span given and reduced on the device."""
    from bwtmi import _lib
    for text_len in TEXTS:
        for mset in sorted(MOTIFS):
            for scale in SCALES:
                h = random_hits(n, text_len, mset, scale)
                want = random_ref(n, text_len, mset, scale)
                longest = int((h[:, 1] - h[:, 0]).max())
                for seg in (1, 0):
                    with _lib.knobs(SEG_LEVELS=seg):
                        for maxlen in (longest, -1):
                            _same(_screen(gpu_ctx, h, text_len, maxlen=maxlen), want,
                                  (n, text_len, mset, scale, seg, maxlen))


@pytest.mark.gpu
@pytest.mark.parametrize("seg", [1, 0])
def test_thresholds(gpu_ctx, seg):
    """ov / rl exactly on 0.1 / 0.3 / 0.5 / 0.8 and one base below, M / m exactly on
    5 and 10 and just below: the kernel's integer tests against the float ones."""
    from bwtmi import _lib
    h, text_len, info = threshold_family()
    with _lib.knobs(SEG_LEVELS=seg):
        got = _screen(gpu_ctx, h, text_len)
    _same(got, ref_rows(h, 3), seg)
    _check_thresholds(got, info)


@pytest.mark.gpu
@pytest.mark.parametrize("cover", [False, True])
def test_dependent_decisions(gpu_ctx, capfd, cover):
    """Up to eight decisions deep, each hanging on the one above: the rounds of
    k_seg_levels (separate segments: the 256-thread workgroups; under one
    covering span: one segment in a 1024-thread workgroup) and the level order."""
    from bwtmi import _lib
    h, text_len, stacks = doll_family(300, cover)
    want = ref_rows(h, 3)
    got, ovf, fb = _screen_stats(capfd, gpu_ctx, h, text_len)
    print(f"dolls cover={cover}: {len(h)} hits, {ovf} overflow windows, fallback {fb}")
    _same(got, want, cover)
    _check_dolls(got, stacks)
    assert fb == 0 and (ovf >= 1 if cover else ovf == 0)
    with _lib.knobs(SEG_LEVELS=0):
        _same(_screen(gpu_ctx, h, text_len), want, (cover, "levels"))


# chain lengths on either side of what a window holds, at rank 0 of a window
# (the window holds the chain alone) and, for the other offsets, the lengths that
# put the window's hits (off % 512 + L) on either side of 1024 and 4096
CHAINS = {0: (1024, 1025, 1500, 4096, 4097, 5000),
          511: (1024, 1025, 1500, 4096, 4097, 5000, 513, 514, 3585, 3586),
          700: (1024, 1025, 1500, 4096, 4097, 5000, 836, 837, 3908, 3909)}


@pytest.mark.gpu
@pytest.mark.parametrize("off", sorted(CHAINS))
def test_segment_sizes(gpu_ctx, capfd, off):
    """One long segment at rank `off`: the window that holds its head holds
    off % 512 + L hits (the isolated hits before it since the window's start, and
    the chain).  Up to 1024 of them stay in the 256-thread workgroups, up to 4096
    go to the overflow list and the 1024-thread workgroup, more fall back to the
    per-level launches.  At rank 0 that is: no overflow for 1024; overflow and no
    fallback for 1025..4096; fallback for 4097 and 5000."""
    seen = []
    try:
        for L in CHAINS[off]:
            h, text_len = chain_family(L, off)
            got, ovf, fb = _screen_stats(capfd, gpu_ctx, h, text_len)
            seen.append(f"chain {L} at rank {off}: {len(h)} hits, {ovf} overflow windows, fallback {fb}")
            _same(got, ref_rows(h, 3), (L, off))
            held = off % 512 + L
            if held <= 1024:
                assert ovf == 0 and fb == 0, (L, off, ovf, fb)
            elif held <= 4096:
                assert ovf >= 1 and fb == 0, (L, off, ovf, fb)
            else:
                assert fb == 1, (L, off, ovf, fb)
    finally:
        print("\n".join(seen))   # (each call's capture starts by dropping what was printed before it)


@pytest.mark.gpu
def test_large_level(gpu_ctx, capfd):
    """A level of more than 65536 hits takes the thread-per-hit kernel, the others
    the wave-per-hit kernel: under BWTMI_SEG_LEVELS=0, and when a 5000-hit
    segment makes the segmented screen fall back by itself."""
    from bwtmi import _lib
    h, text_len = large_level_family(False)
    with _lib.knobs(SEG_LEVELS=0), _kernels(gpu_ctx) as ks:
        got = _screen(gpu_ctx, h, text_len)
    assert ks.get("k_level", (0, 0))[1] == 1 and ks.get("k_level_wave", (0, 0))[1] == 4, sorted(ks)
    _same(got, ref_rows(h, 3), "levels")
    h, text_len = large_level_family(True)
    with _kernels(gpu_ctx) as ks:
        got, ovf, fb = _screen_stats(capfd, gpu_ctx, h, text_len)
    print(f"large level with a 5000 chain: {len(h)} hits, {ovf} overflow windows, fallback {fb}")
    assert fb == 1
    assert ks.get("k_level", (0, 0))[1] >= 1 and ks.get("k_level_wave", (0, 0))[1] >= 1, sorted(ks)
    _same(got, ref_rows(h, 3), "fallback")


@pytest.mark.gpu
@pytest.mark.parametrize("D", WALKS)
def test_long_walks(gpu_ctx, capfd, D):
    """The only nester D ranks behind the query: more than one 64-rank step of the
    wave kernel, and for 5000 a walk across a 4096 tile of the prefix max."""
    from bwtmi import _lib
    h, text_len, (plain, mirror) = walk_family(D)
    want = ref_rows(h, 3)
    with _lib.knobs(SEG_LEVELS=0), _kernels(gpu_ctx) as ks:
        got = _screen(gpu_ctx, h, text_len)
    assert "k_level_wave" in ks and "k_level" not in ks, sorted(ks)
    _same(got, want, (D, "levels"))
    assert not _present(got, plain) and _present(got, mirror)
    got, ovf, fb = _screen_stats(capfd, gpu_ctx, h, text_len)
    _same(got, want, (D, "segments"))
    assert fb == (1 if D > 4096 else 0)


def _layout_runs(ctx, h, want, what):
    from bwtmi import _lib
    longest = int((h[:, 1] - h[:, 0]).max())
    for wide in (0, 1):
        for seg in (1, 0):
            with _lib.knobs(SCREEN_WIDE=wide, SEG_LEVELS=seg):
                for maxlen in (-1, longest):
                    _same(_screen(ctx, h, WIDE_TEXT, maxlen=maxlen), want, (what, wide, seg, maxlen))


@pytest.mark.gpu
@pytest.mark.parametrize("giant_m", [1000, 1])
def test_wide_keys(gpu_ctx, capfd, giant_m):
    """Start, span and motif keys of 32 + 32 + 10 bits: two stable sorts
    (k_keys_start) and two-word records, coordinates up to 2^32 - 2.
    (A text of 2^32 - 2 grows the shared context's bucket slot to 256 MiB.)"""
    h = wide_family(giant_m)
    want = ref_rows(h, 3)
    with _kernels(gpu_ctx) as ks:
        got, ovf, fb = _screen_stats(capfd, gpu_ctx, h, WIDE_TEXT)
    print(f"wide keys, giant motif {giant_m}: {len(h)} hits, {ovf} overflow windows, fallback {fb}")
    assert ks.get("k_keys_start", (0, 0))[1] >= 1, sorted(ks)
    _same(got, want, giant_m)
    assert (got[:, 1] == 3_000_000_000).sum() == 1 and got[:, 0].max() > 2 ** 32 - 6000
    _layout_runs(gpu_ctx, h, want, giant_m)


@pytest.mark.gpu
@pytest.mark.parametrize("maxlen,lmax", LAYOUTS)
def test_record_layouts(gpu_ctx, maxlen, lmax):
    """bits(longest span) + bits(longest motif) + 1 on either side of 32: one word
    per record with the motif up to bit 62 and the cut bit above it, or two; every
    case again with BWTMI_SCREEN_WIDE=1.  (The same 256 MiB bucket slot.)"""
    h = layout_family(maxlen, lmax)
    want = ref_rows(h, 3)
    assert ((want[:, 1] == maxlen) & (want[:, 2] == lmax)).any() and want[:, 0].max() > 2 ** 31
    _layout_runs(gpu_ctx, h, want, (maxlen, lmax))


def _drop_lists():
    for n in (64, 513, 4095):
        for i, text_len in enumerate(TEXTS):
            yield (n, text_len, "mixed", SCALES[i]), random_hits(n, text_len, "mixed", SCALES[i]), text_len
    for n, text_len in ((513, 100_000), (4097, 100_000), (65, 5_000)):     # short and sparse: more to drop
        yield (n, text_len, "two", 2), random_hits(n, text_len, "two", 2), text_len
    h, text_len = sparse_hits()
    yield "sparse", h, text_len


@pytest.mark.gpu
@pytest.mark.parametrize("mc", [1, 2, 3, 7])
def test_drop_and_cuts(gpu_ctx, mc):
    """The cut bits equal the reference's; the drop removes only hits the rule above
    k_drop_flags allows, never one that passes the final filter, leaves the
    survivors' cut bits alone, removes exactly the reference's set where every
    kept hit has a kept neighbour within the 64-rank probe, and nothing with
    BWTMI_SCREEN_DROP=0."""
    from bwtmi import _lib
    removed_total = 0
    for what, h, text_len in _drop_lists():
        want = random_ref(*what, mc) if what != "sparse" else ref_rows(h, mc)
        keep = _screen(gpu_ctx, h, text_len, min_copies=mc)
        _same(keep, want, (what, mc))
        with _lib.knobs(SCREEN_DROP=0):
            _same(_screen(gpu_ctx, h, text_len, min_copies=mc, drop=True), want, (what, mc, "drop off"))
        drop = _screen(gpu_ctx, h, text_len, min_copies=mc, drop=True)
        index = {tuple(r[:3]): k for k, r in enumerate(want.tolist())}
        at = np.array([index.get(tuple(r[:3]), -1) for r in drop.tolist()], dtype=np.int64)
        assert (at >= 0).all() and (np.diff(at) > 0).all(), (what, mc)       # a subset, in order
        _same(drop, want[at], (what, mc, "survivors"))                        # the same cut bits
        gone = np.ones(len(want), dtype=bool)
        gone[at] = False
        may = ref_droppable(want, mc)
        assert not (gone & ~may).any(), (what, mc, want[gone & ~may][:3].tolist())
        m = np.maximum(want[:, 2], 1)
        assert not (gone & (want[:, 1] // m >= mc) & (want[:, 1] >= 6)).any()
        removed_total += int(gone.sum())
        if what == "sparse":
            # the rank, in the order of all hits, of every screened hit: the next
            # one (or the end of the list) lies within the probe
            o = np.lexsort((-h[:, 3], h[:, 1], h[:, 0]))
            first = {}
            for r, i in enumerate(o):
                first.setdefault((int(h[i, 0]), int(h[i, 1] - h[i, 0]), int(h[i, 3])), r)
            rank = np.array([first[tuple(r[:3])] for r in want.tolist()] + [len(h)])
            assert np.diff(rank).max() <= 64
            assert (gone == may).all() and gone.sum() > 100 and (~gone).sum() > 100, (mc, gone.sum(), may.sum())
    assert removed_total > 0


def _raw(ctx, arr, n, text_len, mc=3, drop=0, maxlen=-1, out=True, nout=True):
    from bwtmi import _lib
    o, k = C.c_void_p(), C.c_int64(-7)
    rc = _lib.lib().bwtmi_screen_hits(ctx, arr.ctypes.data_as(C.c_void_p) if arr is not None else None, n, text_len,
                                      mc, drop, maxlen, C.byref(o) if out else None, C.byref(k) if nout else None)
    if rc == 0:
        _lib.lib().bwtmi_free(o)
    return rc, k.value


@pytest.mark.gpu
def test_argument_errors(gpu_ctx):
    """Every rejected input returns BWTMI_E_ARG before anything reaches the device,
    and the next valid call on the context is right."""
    from bwtmi import _lib
    from bwtmi.records import _HIT_DTYPE
    E_ARG = -1
    h = random_hits(513, 5_000, "mixed", 5)
    want = random_ref(513, 5_000, "mixed", 5)
    longest = int((h[:, 1] - h[:, 0]).max())

    def packed(rows):
        arr = np.zeros(len(rows), dtype=_HIT_DTYPE)
        for k, name in enumerate(_HIT_DTYPE.names):
            arr[name] = rows[:, k]
        return arr

    def valid():
        _same(_screen(gpu_ctx, h, 5_000), want, "after an error")

    good = packed(h)
    assert _raw(gpu_ctx, good, len(h), 5_000)[0] == 0
    for kw in (dict(out=False), dict(nout=False), dict(mc=0), dict(mc=-3), dict(maxlen=0), dict(maxlen=longest - 1),
               dict(maxlen=-2)):
        assert _raw(gpu_ctx, good, len(h), 5_000, **kw)[0] == E_ARG, kw
        valid()
    assert _raw(None, good, len(h), 5_000)[0] == E_ARG
    assert _raw(gpu_ctx, None, len(h), 5_000)[0] == E_ARG
    assert _raw(gpu_ctx, good, -1, 5_000)[0] == E_ARG
    assert _raw(gpu_ctx, good, len(h), longest - 1)[0] == E_ARG      # a span past text_len
    valid()
    for col, value in ((0, -1), (1, None), (1, "start"), (1, 5_001), (3, 0), (3, -1)):
        bad = h.copy()
        i = int(np.argmax(bad[:, 1]))      # the bad hit is in the middle of the list
        bad[i, col] = bad[i, 0] if value == "start" else bad[i, 0] - 1 if value is None else value
        assert _raw(gpu_ctx, packed(bad), len(bad), 5_000)[0] == E_ARG, (col, value)
        with pytest.raises(_lib.BwtmiError, match="error -1"):
            _screen(gpu_ctx, bad, 5_000)
        valid()
    assert _raw(gpu_ctx, good, len(h), 5_000, maxlen=longest)[0] == 0
    assert _raw(gpu_ctx, good, 0, 5_000) == (0, 0) and _raw(gpu_ctx, None, 0, 0) == (0, 0)
    assert _screen(gpu_ctx, np.zeros((0, 5), np.int64), 100).shape == (0, 4)
    valid()
