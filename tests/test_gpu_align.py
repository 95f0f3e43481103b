"""BWTCore.align_chains / bwtmi_index_align_chains: base-level alignment of
chains on the device -- a banded edit-distance DP with traceback per gap
between anchors, one CIGAR per chain -- against the contract (include/bwtmi.h)
restated here in plain Python: `gap_align` is the gap DP and its traceback,
`chain_cigar` the blocks and gaps of one chain, `align_oracle` a whole call.
The device's arrays must equal the oracle's, dtypes included."""
import ctypes as C
import itertools
import random
from types import SimpleNamespace

import numpy as np
import pytest

from test_gpu_map import _str_case, map_oracle
from test_gpu_smem import Oracle, _build_texts, _queries, revcomp

gpu = pytest.mark.gpu
E_ARG, E_NOMEM = -1, -4
INF = 1 << 40
OPCODE = {"I": 1, "D": 2, "=": 7, "X": 8}


# ------------------------------------------------------------------ the oracle
def _rle(ops):
    out = []
    for op, n in ops:
        if n == 0:
            continue
        if out and out[-1][0] == op:
            out[-1][1] += n
        else:
            out.append([op, n])
    return [(op, n) for op, n in out]


def gap_align(a: bytes, b: bytes, W=None):
    """The contract's gap DP and traceback on a (query bytes) against b (text
    bytes): (run-length operations [(op, len)], D[m][n]).  W = None: no band."""
    m, n = len(a), len(b)
    d = n - m
    lo, hi = (-m, n) if W is None else (min(0, d) - W, max(0, d) + W)
    D = [[INF] * (n + 1) for _ in range(m + 1)]     # INF: not in the band
    D[0][0] = 0
    for i in range(m + 1):
        Di, Dp = D[i], D[i - 1] if i else None
        for j in range(max(0, i + lo), min(n, i + hi) + 1):
            if i == 0 and j == 0:
                continue
            best = INF
            if i and j and Dp[j - 1] < INF:
                best = Dp[j - 1] + (a[i - 1] != b[j - 1])
            if j and Di[j - 1] < INF and Di[j - 1] + 1 < best:
                best = Di[j - 1] + 1
            if i and Dp[j] < INF and Dp[j] + 1 < best:
                best = Dp[j] + 1
            Di[j] = best
    assert D[m][n] < INF
    i, j, ops = m, n, []
    while i or j:
        v = D[i][j]
        if i and j and D[i - 1][j - 1] < INF and D[i - 1][j - 1] + (a[i - 1] != b[j - 1]) == v:
            ops.append(("=" if a[i - 1] == b[j - 1] else "X", 1))
            i, j = i - 1, j - 1
        elif j and D[i][j - 1] < INF and D[i][j - 1] + 1 == v:
            ops.append(("D", 1))
            j -= 1
        else:
            assert i and D[i - 1][j] + 1 == v
            ops.append(("I", 1))
            i -= 1
    return _rle(ops[::-1]), D[m][n]


def gap_cells(m, n, W):
    return (m + 1) * (abs(n - m) + 2 * W + 1) if m > 0 and n > 0 else 0


def chain_gaps(anchors):
    """(qa, m, rb, n, t) of every gap of a chain, anchors (q, r, len) in the searched string's coordinates"""
    out = []
    for (q0, r0, l0), (q1, r1, l1) in zip(anchors, anchors[1:]):
        dq, dr = (q1 + l1) - (q0 + l0), (r1 + l1) - (r0 + l0)
        assert dq > 0 and dr > 0
        t = min(l1, dq, dr)
        out.append((q0 + l0, dq - t, r0 + l0, dr - t, t))
    return out


def chain_cigar(S: bytes, T: bytes, anchors, W):
    """One chain: (operations [(op, len)], nm, n_eq, cols, (q_0, qe_last, r_0, re_last))"""
    ops = [("=", anchors[0][2])]
    for qa, m, rb, n, t in chain_gaps(anchors):
        ops += gap_align(S[qa:qa + m], T[rb:rb + n], W)[0]
        ops.append(("=", t))
    ops = _rle(ops)
    nm = sum(n for op, n in ops if op != "=")
    n_eq = sum(n for op, n in ops if op == "=")
    q, r, l = anchors[-1]
    return ops, nm, n_eq, nm + n_eq, (anchors[0][0], q + l, anchors[0][1], r + l)


def cigar_text(ops):
    return "".join(f"{n}{op}" for op, n in ops)


def searched_anchors(res, k, m):
    """chain k's anchors in the searched string's coordinates (query length m)"""
    a, b = int(res.member_offsets[k]), int(res.member_offsets[k + 1])
    rev = bool(int(res.strand[k]))
    return [((m - int(res.member_q[t]) - int(res.member_len[t])) if rev else int(res.member_q[t]), int(res.member_r[t]),
             int(res.member_len[t])) for t in range(a, b)]


def align_oracle(T: bytes, queries, res, W=32):
    """The call's expected arrays, as a dict of the AlignResult fields, plus
    `trivial` (gaps with m = 0, n = 0 or m = n = 1) and `ngaps` (all with m + n > 0)."""
    off, cig, nm, neq, cols, qs, qe, rs, re, cells, trivial, ngaps = [0], [], [], [], [], [], [], [], [], 0, 0, 0
    for qi, Q in enumerate(queries):
        Q = Q.encode() if isinstance(Q, str) else bytes(Q)
        for k in range(int(res.offsets[qi]), int(res.offsets[qi + 1])):
            rev = bool(int(res.strand[k]))
            anchors = searched_anchors(res, k, len(Q))
            ops, a, b, c, (s0, s1, r0, r1) = chain_cigar(revcomp(Q) if rev else Q, T, anchors, W)
            cig += [n << 4 | OPCODE[op] for op, n in ops]
            off.append(len(cig))
            nm.append(a)
            neq.append(b)
            cols.append(c)
            qs.append(len(Q) - s1 if rev else s0)
            qe.append(len(Q) - s0 if rev else s1)
            rs.append(r0)
            re.append(r1)
            for _, m, _, n, _ in chain_gaps(anchors):
                cells += gap_cells(m, n, W)
                ngaps += m + n > 0
                trivial += m + n > 0 and (m == 0 or n == 0 or (m == 1 and n == 1))
    return {"cigar_offsets": np.array(off, np.int64), "cigar": np.array(cig, np.uint32), "nm": np.array(nm, np.int32),
            "n_eq": np.array(neq, np.int32), "cols": np.array(cols, np.int32), "qstart": np.array(qs, np.int32),
            "qend": np.array(qe, np.int32), "rstart": np.array(rs, np.int64), "rend": np.array(re, np.int64),
            "cells_total": cells, "trivial": trivial, "ngaps": ngaps}


_FIELDS = ("cigar_offsets", "cigar", "nm", "n_eq", "cols", "qstart", "qend", "rstart", "rend")


def assert_equal(got, want, what=None):
    for f in _FIELDS:
        g = getattr(got, f)
        assert g.dtype == want[f].dtype, (f, g.dtype, what)
        if g.shape != want[f].shape or g.tolist() != want[f].tolist():
            bad = next((k for k in range(len(got)) if got.cigar_string(k) != _want_string(want, k)), None)
            assert False, (f, what, bad, bad is not None and (got.cigar_string(bad), _want_string(want, bad)))
    assert got.cells_total == want["cells_total"], what
    assert sum(got.gaps) == want["ngaps"] and got.gaps[0] == want["trivial"], (got.gaps, what)


def _want_string(want, k):
    a, b = int(want["cigar_offsets"][k]), int(want["cigar_offsets"][k + 1])
    return "".join(f"{int(v) >> 4}{'?ID????=X'[int(v) & 15]}" for v in want["cigar"][a:b])


def check_cigar(S: bytes, T: bytes, ops, span, nm, n_eq, cols, blocks_match=True):
    """What a CIGAR says of itself, with no DP: it consumes exactly its span,
    every '=' column has equal bytes and every 'X' column unequal ones."""
    q, q1, r, r1 = span
    for op, n in ops:
        assert n > 0 and op in "IDX="
        if op in "=X":
            if blocks_match or op == "X":
                assert all((S[q + x] == T[r + x]) == (op == "=") for x in range(n)), (op, q, r)
            q, r = q + n, r + n
        elif op == "I":
            q += n
        else:
            r += n
    assert (q, r) == (q1, r1)
    assert all(x[0] != y[0] for x, y in zip(ops, ops[1:]))
    assert nm == sum(n for op, n in ops if op != "=") and n_eq == sum(n for op, n in ops if op == "=")
    assert cols == nm + n_eq


def decode(res, k):
    a, b = int(res.cigar_offsets[k]), int(res.cigar_offsets[k + 1])
    return [("?ID????=X"[int(v) & 15], int(v) >> 4) for v in res.cigar[a:b]]


# ------------------------------------------------------------------ inputs
def _dna(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n)).encode()


def _edit(rng, s: bytes, rate=None, count=None):
    """s with random substitutions, insertions and deletions: each base with probability `rate`, or `count` in all"""
    out = list(s)
    where = ([i for i in range(len(out)) if rng.random() < rate] if count is None
             else [rng.randrange(max(len(out), 1)) for _ in range(count)])
    for i in sorted(where, reverse=True):
        kind = rng.randrange(3)
        if kind == 0 and i < len(out):
            out[i] = rng.choice([c for c in b"ACGT" if c != out[i]])
        elif kind == 1:
            out.insert(i, rng.choice(b"ACGT"))
        elif i < len(out):
            del out[i]
    return bytes(out)


def _chains(items):
    """The arrays of a MapResult from hand-made chains: items = [(S, strand,
    anchors)], one query per chain, S the searched string and the anchors in
    its coordinates; the query is revcomp(S) on strand 1.  -> (queries, arrays)"""
    queries, strand, moff, mq, mr, ml = [], [], [0], [], [], []
    for S, st, anchors in items:
        queries.append(revcomp(S) if st else S)
        strand.append(st)
        for q, r, l in anchors:
            mq.append(len(S) - q - l if st else q)
            mr.append(r)
            ml.append(l)
        moff.append(len(mq))
    n = len(items)
    return queries, SimpleNamespace(offsets=np.arange(n + 1, dtype=np.int64), strand=np.array(strand, np.uint8),
                                    member_offsets=np.array(moff, np.int64), member_q=np.array(mq, np.int32),
                                    member_r=np.array(mr, np.int64), member_len=np.array(ml, np.int32))


def _one_gap(a: bytes, rb: int, n: int, st=0):
    """a against T[rb, rb + n) as the gap between two one-byte anchors (taken on trust)"""
    return b"G" + a + b"T", st, [(0, rb - 1, 1), (1 + len(a), rb + n, 1)]


def _text():
    """every string over {A, C} of up to 4 bytes, then random ACGT"""
    rng = random.Random(20261021)
    ac = b"G".join("".join(p).encode() for k in range(1, 5) for p in itertools.product("AC", repeat=k))
    return b"TG" + ac + b"G" + _dna(rng, 3000) + b"$"


def _random_chains(rng, T, count, sizes=(1, 2, 9)):
    """chains of true matches with edited gaps, some anchors grown backwards over their gap and their predecessor"""
    items = []
    for x in range(count):
        k = sizes[x % len(sizes)]
        r = rng.randrange(1, 1200)
        S, anchors = b"", []
        for i in range(k):
            if i:
                n = rng.choice((0, 0, 1, 1, 2, 3, 5, 8, 20))
                b = T[r:r + n]
                a = rng.choice((b, _edit(rng, b, 0.3), _dna(rng, rng.randrange(0, 6)), b[:1] + _dna(rng, 3) + b[-1:]))
                if not a and not b:
                    a = b"A"
                S, r = S + a, r + n
            l = rng.randrange(1, 30)
            grow = rng.choice((0, 0, 0, 1, 4, 12)) if i else 0
            grow = min(grow, len(S), r - 1)
            anchors.append((len(S) - grow, r - grow, l + grow))
            S, r = S + T[r:r + l], r + l
        items.append((S, x % 4 == 3, anchors))
    return items


# ------------------------------------------------------------------ CPU: the oracle itself
def test_oracle_cigars_are_valid():
    rng = random.Random(5)
    T = _text()
    seen = set()
    for S, st, anchors in _random_chains(rng, T, 60):
        for W in (0, 2, 32):
            ops, nm, n_eq, cols, span = chain_cigar(S, T, anchors, W)
            exact = all(S[q:q + l] == T[r:r + l] for q, r, l in anchors)     # (a grown anchor need not match)
            check_cigar(S, T, ops, span, nm, n_eq, cols, blocks_match=exact)
            seen |= {op for op, _ in ops}
    assert seen == set("IDX=")


def test_wide_band_is_unbanded():
    rng = random.Random(6)
    for _ in range(60):
        b = _dna(rng, rng.randrange(0, 40))
        a = _edit(rng, b, 0.2) if rng.random() < 0.7 else _dna(rng, rng.randrange(0, 40))
        assert gap_align(a, b, max(len(a), len(b))) == gap_align(a, b, None)


def test_narrow_band_differs():
    rng = random.Random(8)
    differ = 0
    for _ in range(40):
        b = _dna(rng, 60)
        a = _edit(rng, b, count=8)
        banded, free = gap_align(a, b, 0), gap_align(a, b, None)
        assert banded[1] >= free[1]
        differ += banded[1] != free[1]
    print("W = 0 differs from the unbanded DP in", differ, "of 40")
    assert differ >= 1


_STR_WANT = {20: ("40=1X219=1X99=", 2), 12: ("40=1X145=24D74=1X75=", 26), 45: ("40=1X169=75I150=", 76)}


def test_str_case_on_the_oracle():
    text, reads, copies = _str_case()
    want = SimpleNamespace(**map_oracle(Oracle(text), reads, 15, True))
    for i, (read, n) in enumerate(zip(reads, copies)):
        k = int(want.offsets[i])
        assert int(want.strand[k]) == i % 2
        S = revcomp(read) if i % 2 else read
        for W in (0, 32):
            ops, nm, n_eq, cols, span = chain_cigar(S, text, searched_anchors(want, k, len(read)), W)
            assert (cigar_text(ops), nm) == _STR_WANT[n], (i, W)
            check_cigar(S, text, ops, span, nm, n_eq, cols)


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def env(gpu_ctx):
    from bwtmi import BWTCore
    T = _text()
    return T, BWTCore(T, build_kmer=False)


def _run(core, T, items, W, what=None, **kw):
    queries, arrays = _chains(items)
    want = align_oracle(T, queries, arrays, 32 if W is None else W)
    got = core.align_chains(queries, arrays, band=W, **kw)
    assert_equal(got, want, what)
    return got, want


@gpu
@pytest.mark.parametrize("W", [0, 1, 32])
def test_every_pair_over_two_letters(env, W):
    """every pair of strings over {A, C} of length 0..4 as one gap each: the tie
    rules, and the 0 x n, m x 0 and 1 x 1 shortcuts"""
    T, core = env
    strings = [b""] + ["".join(p).encode() for k in range(1, 5) for p in itertools.product("AC", repeat=k)]
    items = []
    for a in strings:
        for b in strings:
            rb = T.find(b"G" + b + b"G") + 1
            assert rb >= 1 and T[rb:rb + len(b)] == b
            items.append(_one_gap(a, rb, len(b)))
    assert len(items) == 961
    got, want = _run(core, T, items, W)
    assert got.gaps[0] == 31 + 31 - 1 - 1 + 4 and got.gaps[1] == 961 - 1 - got.gaps[0] and got.gaps[2] == 0


@gpu
def test_sides_swept(env):
    """gap sides 0..40 independently, random 15 % edits: both sides of the one-lane / one-wave threshold"""
    T, core = env
    rng = random.Random(11)
    items = []
    for m in range(41):
        for n in range(41):
            rb = rng.randrange(200, 2500)
            a = _edit(rng, T[rb:rb + max(m, n) + 8], 0.15)[:m]
            a += _dna(rng, m - len(a))
            items.append(_one_gap(a, rb, n))
    for W in (None, 2):
        got, want = _run(core, T, items, W, W)
        assert got.gaps[1] > 200 and got.gaps[2] > 1000


@gpu
def test_band_widths(env):
    """bands of 63, 64, 65, 127, 128, 129 columns (the wave kernel's chunks of
    64) on rows of 1, 2, 64, 65 and 300; delta = +- the width's bound at W = 0;
    and a band above the LDS rows' 1023 columns"""
    T, core = env
    rng = random.Random(12)
    by_w = {}
    for wb in (63, 64, 65, 127, 128, 129):
        half = (wb - 1) // 2
        for W, delta in ((0, wb - 1), (0, -(wb - 1)), (half, wb - 1 - 2 * half), (half - 3, -(wb - 1 - 2 * (half - 3)))):
            for m in (1, 2, 64, 65, 300):
                n = m + delta
                if n < 0:
                    continue
                assert abs(delta) + 2 * W + 1 == wb
                rb = rng.randrange(200, 2500 - n)
                a = _edit(rng, T[rb:rb + max(m, n) + 40], 0.1)[:m]
                a += _dna(rng, m - len(a))
                by_w.setdefault(W, []).append(_one_gap(a, rb, n))
    by_w[0] += [_one_gap(_dna(rng, 3), 300, 3 + 1100), _one_gap(T[300:1400], 300, 2)]     # 1101 columns: rows in global memory
    a = _edit(rng, T[400:640], 0.05)[:200]
    by_w.setdefault(1, []).append(_one_gap(a + _dna(rng, 200 - len(a)), 400, 200 + 1040))  # 1043 columns, 200 rows
    for W, items in sorted(by_w.items()):
        got, want = _run(core, T, items, W, W)
        assert got.gaps[2] >= len(items) - 6


@gpu
def test_narrow_band_on_a_long_gap(env):
    T, core = env
    rng = random.Random(13)
    b = T[500:830]
    # 10 bases more in front, 40 fewer later, 10 % edits everywhere: the best path leaves the diagonals -3 .. 33
    a = (_dna(rng, 10) + _edit(rng, b[:100] + b[140:], 0.1) + _dna(rng, 300))[:300]
    banded, free = gap_align(a, b, 3), gap_align(a, b, None)
    assert banded[1] != free[1]                    # the band, not the strings, decides this alignment
    got, want = _run(core, T, [_one_gap(a, 500, 330)], 3)
    assert got.nm[0] == banded[1] and got.gaps == (0, 0, 1) and got.cells_total == 301 * 37


@gpu
def test_chains_of_anchors(env):
    """chains of 1, 2 and 9 anchors: overlapping anchors, '=' merged across block boundaries, strand 1"""
    T, core = env
    rng = random.Random(14)
    items = _random_chains(rng, T, 90)
    dq_cut = dr_cut = fused = 0
    for S, st, anchors in items:
        for (q0, r0, l0), (q, r, l) in zip(anchors, anchors[1:]):
            dq, dr = q + l - q0 - l0, r + l - r0 - l0
            dq_cut += dq < l and dq <= dr                   # t_i = dq < len_i
            dr_cut += dr < l and dr < dq                    # t_i = dr < len_i
        fused += sum(op == "=" for op, _ in chain_cigar(S, T, anchors, 32)[0]) < len(anchors)
    assert dq_cut > 3 and dr_cut > 3 and fused > 3 and sum(st for _, st, _ in items) > 10
    assert sorted({len(a) for _, _, a in items}) == [1, 2, 9]
    for W in (None, 0, 1):
        _run(core, T, items, W, W)
    # the gap's first and last bytes match and its middle two do not: the blocks fuse with the gap at both ends
    other = bytes(ord("A") if c != ord("A") else ord("C") for c in T[111:113])
    S = T[100:111] + other + T[113:120]
    got, _ = _run(core, T, [(S, 0, [(0, 100, 10), (14, 114, 6)])], 32)
    assert got.cigar_string(0) == "11=2X7="


@gpu
def test_other_bytes_and_strand_one(gpu_ctx):
    """queries with N, lower case and an absent byte against the text with N runs and R / Y, on both strands"""
    from bwtmi import BWTCore
    T = _build_texts()["gaps"]
    core = BWTCore(T, build_kmer=False)
    items = []
    for st in (0, 1):
        items += [_one_gap(b"NNNN" + T[404:412].lower() + b"X" + T[413:425], 400, 30, st),
                  _one_gap(T[1990:2010], 1992, 25, st), _one_gap(b"N", 1601, 1, st), _one_gap(b"n", 1601, 1, st),
                  _one_gap(b"ACGTNNRYacgtXX$" + T[2000:2040], 1995, 50, st),
                  (T[1580:1640], st, [(0, 1580, 15), (22, 1602, 10), (40, 1620, 20)])]
    for W in (None, 0):
        got, want = _run(core, T, items, W, W)
    for k in (0, 6):                                                    # bytes compare by equality: N is N, n is not
        assert got.cigar_string(k + 2) == "3=" and got.cigar_string(k + 3) == "1=1X1="
    assert (want["qstart"][-1], want["qend"][-1]) == (0, 60)


def _validate(T, queries, res, aln):
    for qi, Q in enumerate(queries):
        for k in range(int(res.offsets[qi]), int(res.offsets[qi + 1])):
            rev = bool(int(res.strand[k]))
            m = len(Q)
            s0, s1 = (m - int(aln.qend[k]), m - int(aln.qstart[k])) if rev else (int(aln.qstart[k]), int(aln.qend[k]))
            check_cigar(revcomp(Q) if rev else Q, T, decode(aln, k), (s0, s1, int(aln.rstart[k]), int(aln.rend[k])),
                        int(aln.nm[k]), int(aln.n_eq[k]), int(aln.cols[k]))


@gpu
def test_map_then_align_str_case(gpu_ctx):
    from bwtmi import BWTCore
    text, reads, copies = _str_case()
    core = BWTCore(text, build_kmer=False)
    res = core.map_batch(reads, min_len=15, both_strands=True)
    for W in (None, 0):
        aln = core.align_chains(reads, res, band=W)
        assert_equal(aln, align_oracle(text, reads, res, 32 if W is None else W), W)
        _validate(text, reads, res, aln)
        for i, n in enumerate(copies):
            k = int(res.offsets[i])
            assert (aln.cigar_string(k), int(aln.nm[k])) == _STR_WANT[n], (i, W)
            assert (int(aln.qstart[k]), int(aln.qend[k]), int(aln.rstart[k]), int(aln.rend[k])) == \
                (0, len(reads[i]), 350, 710)
    assert len(aln) == res.strand.size and aln.cols.tolist() == (aln.nm + aln.n_eq).tolist()


@gpu
@pytest.mark.parametrize("name", ["acgt", "gaps"])
def test_map_then_align_smem_queries(gpu_ctx, name):
    from bwtmi import BWTCore
    T = _build_texts()[name]
    core = BWTCore(T, build_kmer=False)
    queries = _queries(T)
    res = core.map_batch(queries, min_len=12, both_strands=True, min_score=20, max_gap=400, bandwidth=60)
    assert res.strand.size > 20 and res.n_anchors.max() > 2 and (res.strand == 1).any()
    aln = core.align_chains(queries, res)
    want = align_oracle(T, queries, res)
    assert_equal(aln, want, name)
    _validate(T, queries, res, aln)
    assert want["ngaps"] > 10 and aln.nm.max() > 0
    again = core.align_chains(queries, res)               # nothing is kept between calls
    assert_equal(again, want, "again")
    other = core.align_chains(queries[:3], SimpleNamespace(
        offsets=res.offsets[:4], strand=res.strand[:res.offsets[3]], member_offsets=res.member_offsets[:res.offsets[3] + 1],
        member_q=res.member_q[:res.member_offsets[res.offsets[3]]], member_r=res.member_r[:res.member_offsets[res.offsets[3]]],
        member_len=res.member_len[:res.member_offsets[res.offsets[3]]]))
    assert len(other) == int(res.offsets[3])
    assert_equal(core.align_chains(queries, res), want, "after another call")


# ------------------------------------------------------------------ cap, arguments, the empty call
def _raw(lib, core, queries, arr, band=-1, max_cells=0, reserved=None, off=None, nchain=None, nmember=None):
    from bwtmi._lib import AlignParams
    blob = np.frombuffer(b"".join(queries) or b"\0", dtype=np.uint8)
    if off is None:
        off = np.concatenate([[0], np.cumsum([len(q) for q in queries])])
    off = np.asarray(off, dtype=np.int64)
    p = AlignParams()
    p.band, p.max_cells = band, max_cells
    if reserved is not None:
        p.reserved[reserved] = 1
    cols = [np.ascontiguousarray(a, dtype=t) for a, t in ((arr.offsets, np.int64), (arr.strand, np.uint8),
                                                          (arr.member_offsets, np.int64), (arr.member_q, np.int32),
                                                          (arr.member_r, np.int64), (arr.member_len, np.int32))]
    ptrs = [C.c_void_p(0xdead) for _ in range(9)]
    nc, cells = C.c_int64(-7), C.c_int64(-7)
    gaps = (C.c_int64 * 3)(-7, -7, -7)
    rc = lib.bwtmi_index_align_chains(core._ctx, core._h, blob.ctypes.data_as(C.c_void_p),
                                      off.ctypes.data_as(C.c_void_p), off.size - 1,
                                      *[a.ctypes.data_as(C.c_void_p) for a in cols],
                                      cols[1].size if nchain is None else nchain,
                                      cols[3].size if nmember is None else nmember, C.byref(p),
                                      *[C.byref(x) for x in ptrs], C.byref(nc), C.byref(cells), gaps)
    return rc, ptrs, [nc.value, cells.value] + list(gaps)


def _mod(arr, **kw):
    d = {k: np.array(v) for k, v in vars(arr).items()}
    for k, (i, v) in kw.items():
        d[k][i] = v
    return SimpleNamespace(**d)


@gpu
def test_argument_errors(env, built_lib):
    T, core = env
    items = [(T[100:160], 0, [(0, 100, 20), (25, 125, 10), (40, 140, 20)]), (T[200:240], 1, [(0, 200, 40)])]
    queries, arr = _chains(items)
    rc, ptrs, counts = _raw(built_lib, core, queries, arr)
    assert rc == 0 and counts[0] >= 2 and all(p.value not in (None, 0xdead) for p in ptrs)
    for p in ptrs:
        built_lib.bwtmi_free(p)
    n = len(T)
    long_q = [T[100:101] * 70000, queries[1]]
    bad = {
        "chain offsets decrease": dict(arr=_mod(arr, offsets=(1, 3))),
        "chain offsets do not end at nchain": dict(arr=_mod(arr, offsets=(2, 1))),
        "member offsets decrease": dict(arr=_mod(arr, member_offsets=(1, 5))),
        "member offsets do not start at 0": dict(arr=_mod(arr, member_offsets=(0, 1))),
        "query offsets decrease": dict(off=[0, 100, 60]),
        "strand 2": dict(arr=_mod(arr, strand=(1, 2))),
        "a chain with no member": dict(arr=_mod(arr, member_offsets=(1, 0))),
        "len 0": dict(arr=_mod(arr, member_len=(1, 0))),
        "a member before its query": dict(arr=_mod(arr, member_q=(0, -1))),
        "a member past its query": dict(arr=_mod(arr, member_len=(2, 21))),
        "a member past its query on strand 1": dict(arr=_mod(arr, member_q=(3, 1))),
        "r below 0": dict(arr=_mod(arr, member_r=(0, -1))),
        "a member past the text": dict(arr=_mod(arr, member_r=(3, n - 39))),
        "dq = 0": dict(arr=_mod(arr, member_q=(1, 10), member_len=(1, 10))),
        "dq < 0": dict(arr=_mod(arr, member_q=(1, 5), member_len=(1, 10))),
        "dr = 0": dict(arr=_mod(arr, member_r=(1, 110))),
        "a gap side above 65535": dict(queries=long_q, arr=_mod(arr, member_q=(2, 69980), member_r=(2, 140))),
        "band 1025": dict(band=1025),
        "a reserved field": dict(reserved=2),
    }
    for what, kw in bad.items():
        rc, ptrs, counts = _raw(built_lib, core, kw.pop("queries", queries), kw.pop("arr", arr), **kw)
        assert rc == E_ARG and built_lib.bwtmi_last_error(), what
        assert all(p.value is None for p in ptrs) and counts == [0] * 5, what
    # a gap side of exactly 65,535 is legal (the text side is empty: no DP, one 'I' run)
    ok = _mod(arr, member_q=(1, 20 + 65535), member_r=(1, 120), member_len=(1, 1))
    ok.member_q[2], ok.member_r[2] = 20 + 65535 + 6, 140
    res = core.align_chains(long_q, ok)
    assert res.cigar_string(0).startswith("20=65535I") and res.gaps[0] >= 1
    for kw in (dict(band=-1), dict(band=1025), dict(max_cells=0)):
        with pytest.raises(ValueError):
            core.align_chains(queries, arr, **kw)
    with pytest.raises(ValueError):
        core.align_chains(queries[:1], arr)


@gpu
def test_cell_cap(env, built_lib):
    from bwtmi._lib import BwtmiError
    T, core = env
    rng = random.Random(15)
    items = [_one_gap(_edit(rng, T[r:r + n], 0.2), r, n) for r, n in ((300, 5), (400, 30), (500, 1), (600, 70), (700, 0))]
    queries, arr = _chains(items)
    want = align_oracle(T, queries, arr, 4)
    total = want["cells_total"]
    assert total > 500
    assert_equal(core.align_chains(queries, arr, band=4, max_cells=total), want)
    with pytest.raises(BwtmiError, match=str(total)) as e:
        core.align_chains(queries, arr, band=4, max_cells=total - 1)
    assert e.value.cells_total == total
    rc, ptrs, counts = _raw(built_lib, core, queries, arr, band=4, max_cells=total - 1)
    assert rc == E_NOMEM and str(total).encode() in built_lib.bwtmi_last_error()
    assert all(p.value is None for p in ptrs) and counts == [0, total, 0, 0, 0]


@gpu
def test_no_chains(env, built_lib):
    T, core = env
    none = SimpleNamespace(offsets=np.zeros(3, np.int64), strand=np.zeros(0, np.uint8), member_offsets=np.zeros(1, np.int64),
                           member_q=np.zeros(0, np.int32), member_r=np.zeros(0, np.int64),
                           member_len=np.zeros(0, np.int32))
    for queries, arr in (([b"ACGT", b"GG"], none), ([], SimpleNamespace(**{**vars(none), "offsets": np.zeros(1, np.int64)}))):
        res = core.align_chains(queries, arr)
        assert len(res) == 0 and res.cigar_offsets.tolist() == [0] and res.cigar.size == 0 and res.cells_total == 0
        assert res.cigar_offsets.dtype == np.int64 and res.cigar.dtype == np.uint32 and res.nm.dtype == np.int32
        assert res.rstart.dtype == np.int64 and res.qend.dtype == np.int32 and res.gaps == (0, 0, 0)
        rc, ptrs, counts = _raw(built_lib, core, queries, arr)
        assert rc == 0 and counts == [0] * 5 and all(p.value not in (None, 0xdead) for p in ptrs)
        assert C.cast(ptrs[0], C.POINTER(C.c_int64))[0] == 0
        for p in ptrs:
            built_lib.bwtmi_free(p)
    # params = NULL and every count NULL
    queries, arr = _chains([_one_gap(b"ACG", 300, 4)])
    blob, off = np.frombuffer(b"".join(queries), dtype=np.uint8), np.array([0, len(queries[0])], dtype=np.int64)
    ptrs, nc = [C.c_void_p() for _ in range(9)], C.c_int64()
    cols = (arr.offsets, arr.strand, arr.member_offsets, arr.member_q, arr.member_r, arr.member_len)
    assert built_lib.bwtmi_index_align_chains(core._ctx, core._h, blob.ctypes.data_as(C.c_void_p),
                                              off.ctypes.data_as(C.c_void_p), 1,
                                              *[a.ctypes.data_as(C.c_void_p) for a in cols], 1, 2, None,
                                              *[C.byref(p) for p in ptrs], C.byref(nc), None, None) == 0
    assert nc.value >= 1
    for p in ptrs:
        built_lib.bwtmi_free(p)
