"""BWTCore.align_chains(extend=True) / bwtmi_index_align_extend: every chain
extended past its outer anchors towards the read's ends, a scored banded DP
with X-drop per head and tail, against the contract (include/bwtmi.h) restated
here in plain Python: `ext_align` is one extension (the tail rule; a head is
the same on the reversed strings), `extend_oracle` a whole call over the gap
oracle of tests/test_gpu_align.py.  The device's arrays must equal the
oracle's, dtypes included."""
import ctypes as C
import itertools
import random
from types import SimpleNamespace

import numpy as np
import pytest

from test_gpu_align import (OPCODE, _chains, _dna, _edit, _mod, _one_gap, _random_chains, _rle, _text, assert_equal,
                            chain_cigar, chain_gaps, cigar_text, decode, gap_cells, searched_anchors)
from test_gpu_smem import _build_texts, revcomp

gpu = pytest.mark.gpu
E_ARG, E_NOMEM = -1, -4
DEFAULTS = dict(We=32, A=1, B=3, G=3, X=30)


# ------------------------------------------------------------------ the oracle
def ext_align(a: bytes, b: bytes, We=32, A=1, B=3, G=3, X=30):
    """The contract's tail rule on a (the query bytes past the anchor) against
    b (all the text bytes past it): (run-length operations, score, i*, j*, rows)."""
    m, n = len(a), min(len(b), len(a) + We)
    if m == 0 or n == 0:
        return [], 0, 0, 0, 0
    H = [{j: -G * j for j in range(min(n, We) + 1)}]
    best, bi, bj, rows = 0, 0, 0, 0
    for i in range(1, m + 1):
        prev, row = H[i - 1], {}
        for j in range(max(0, i - We), min(n, i + We) + 1):
            cand = []
            if j and j - 1 in prev:
                cand.append(prev[j - 1] + (A if a[i - 1] == b[j - 1] else -B))
            if j and j - 1 in row:
                cand.append(row[j - 1] - G)
            if j in prev:
                cand.append(prev[j] - G)
            row[j] = max(cand)
        if not row:
            break
        H.append(row)
        rows = i
        for j in sorted(row):
            if row[j] > best:
                best, bi, bj = row[j], i, j
        if best - max(row.values()) > X:
            break
    i, j, ops = bi, bj, []
    while i or j:
        v = H[i][j]
        if i and j and j - 1 in H[i - 1] and H[i - 1][j - 1] + (A if a[i - 1] == b[j - 1] else -B) == v:
            ops.append(("=" if a[i - 1] == b[j - 1] else "X", 1))
            i, j = i - 1, j - 1
        elif j and j - 1 in H[i] and H[i][j - 1] - G == v:
            ops.append(("D", 1))
            j -= 1
        else:
            assert i and j in H[i - 1] and H[i - 1][j] - G == v      # the trace always finds a source
            ops.append(("I", 1))
            i -= 1
    return _rle(ops[::-1]), best, bi, bj, rows


def ops_score(ops, A=1, B=3, G=3):
    return sum(n * {"=": A, "X": -B, "I": -G, "D": -G}[op] for op, n in ops)


def ops_consume(ops):
    return sum(n for op, n in ops if op != "D"), sum(n for op, n in ops if op != "I")


def chain_ends(S: bytes, T: bytes, anchors, We=32, A=1, B=3, G=3, X=30):
    """(head, tail) of one chain, each as ext_align returns it; the head's operations already reversed"""
    q0, r0, _ = anchors[0]
    q, r, l = anchors[-1]
    tail = ext_align(S[q + l:], T[r + l:r + l + len(S) - q - l + We], We, A, B, G, X)
    head = ext_align(S[:q0][::-1], T[max(0, r0 - q0 - We):r0][::-1], We, A, B, G, X)
    return (head[0][::-1],) + head[1:], tail


def extend_oracle(T: bytes, queries, res, W=32, We=32, A=1, B=3, G=3, X=30):
    """The call's expected arrays: the fields of test_gpu_align.align_oracle plus
    head_score, tail_score, ext_rows, and per chain the (head, tail) operations in `ends`."""
    off, cig, nm, neq, cols, qs, qe, rs, re, hs, ts, ends = [0], [], [], [], [], [], [], [], [], [], [], []
    cells = trivial = ngaps = rows = 0
    for qi, Q in enumerate(queries):
        Q = Q.encode() if isinstance(Q, str) else bytes(Q)
        for k in range(int(res.offsets[qi]), int(res.offsets[qi + 1])):
            rev = bool(int(res.strand[k]))
            S = revcomp(Q) if rev else Q
            anchors = searched_anchors(res, k, len(Q))
            mid, _, _, _, (s0, s1, r0, r1) = chain_cigar(S, T, anchors, W)
            head, tail = chain_ends(S, T, anchors, We, A, B, G, X)
            ops = _rle(head[0] + mid + tail[0])
            a = sum(n for op, n in ops if op != "=")
            b = sum(n for op, n in ops if op == "=")
            s0, s1, r0, r1 = s0 - head[2], s1 + tail[2], r0 - head[3], r1 + tail[3]
            cig += [n << 4 | OPCODE[op] for op, n in ops]
            off.append(len(cig))
            nm.append(a)
            neq.append(b)
            cols.append(a + b)
            qs.append(len(Q) - s1 if rev else s0)
            qe.append(len(Q) - s0 if rev else s1)
            rs.append(r0)
            re.append(r1)
            hs.append(head[1])
            ts.append(tail[1])
            ends.append((head[0], tail[0]))
            rows += head[4] + tail[4]
            q0, rr0, _ = anchors[0]
            q, r, l = anchors[-1]
            for m_, n_, e in ((q0, min(rr0, q0 + We), head), (len(S) - q - l, min(len(T) - r - l, len(S) - q - l + We), tail)):
                if m_ > 0 and n_ > 0:
                    cells += (e[2] + 1) * (2 * We + 1)
            for _, m, _, n, _ in chain_gaps(anchors):
                cells += gap_cells(m, n, W)
                ngaps += m + n > 0
                trivial += m + n > 0 and (m == 0 or n == 0 or (m == 1 and n == 1))
    return {"cigar_offsets": np.array(off, np.int64), "cigar": np.array(cig, np.uint32), "nm": np.array(nm, np.int32),
            "n_eq": np.array(neq, np.int32), "cols": np.array(cols, np.int32), "qstart": np.array(qs, np.int32),
            "qend": np.array(qe, np.int32), "rstart": np.array(rs, np.int64), "rend": np.array(re, np.int64),
            "cells_total": cells, "trivial": trivial, "ngaps": ngaps, "head_score": np.array(hs, np.int32),
            "tail_score": np.array(ts, np.int32), "ext_rows": rows, "ends": ends}


def assert_equal_ext(got, want, what=None):
    assert_equal(got, want, what)
    for f in ("head_score", "tail_score"):
        g = getattr(got, f)
        assert g.dtype == np.int32 and g.tolist() == want[f].tolist(), (f, what)
    assert got.ext_rows == want["ext_rows"], (got.ext_rows, want["ext_rows"], what)


# ------------------------------------------------------------------ inputs
def _tail(a: bytes, rb: int, st=0):
    """a as the tail of a one-byte anchor (taken on trust) that ends at text position rb"""
    return b"G" + a, st, [(0, rb - 1, 1)]


def _head(a: bytes, re: int, st=0):
    """a (in the reversed order the rule reads it) as the head of a one-byte anchor that starts at text position re"""
    return a[::-1] + b"G", st, [(len(a), re, 1)]


def _two_letter(limit):
    return [b""] + ["".join(p).encode() for k in range(1, limit + 1) for p in itertools.product("AC", repeat=k)]


def _pair_text():
    """'T' + b + 38 x 'G' for every b over {A, C} of up to 5 bytes: whatever a
    band of 32 sees past b, or before it, matches no byte of a query over {A, C}"""
    blocks, text = {}, b""
    for b in _two_letter(5):
        blocks[b] = len(text) + 1
        text += b"T" + b + b"G" * 38
    return text + b"$", blocks


def _edited_tails(rng, T, count, longest, rate=0.12):
    items = []
    for x in range(count):
        n = rng.randrange(1, longest + 1)
        r = rng.randrange(100, len(T) - 200)
        a = _edit(rng, T[r:r + n + 6], rate)[:n]
        items.append(_tail(a, r, x % 3 == 2) if x % 2 else _head(a[::-1], r + n, x % 3 == 2))
    return items


# ------------------------------------------------------------------ CPU: the oracle itself
def _self_check(a, b, **kw):
    ops, score, bi, bj, rows = ext_align(a, b, **kw)
    p = {k: kw.get(k, DEFAULTS[k]) for k in "ABG"}
    assert ops_score(ops, **p) == score and ops_consume(ops) == (bi, bj), (a, b, kw)
    assert not ops or ops[-1][0] == "=", (a, b, kw)           # an extension never ends in X, I or D
    assert bi <= rows <= len(a) and score >= 0
    return ops, score, bi, bj, rows


def test_oracle_small_pairs():
    """every pair over two letters: the operations' score is the best score and they consume (i*, j*)"""
    for a in _two_letter(4):
        for b in _two_letter(5):
            for We in (0, 1, 2, 32):
                for X in (0, 2, 1000):
                    ops, score, bi, bj, rows = _self_check(a, b, We=We, X=X)
                    if not a or not b:
                        assert (ops, score, bi, bj, rows) == ([], 0, 0, 0, 0)
    assert ext_align(b"AAC", b"AAC")[:4] == ([("=", 3)], 3, 3, 3)
    assert ext_align(b"CAACA", b"AAACA")[:4] == ([("X", 1), ("=", 4)], 1, 5, 5)
    assert ext_align(b"CAAAA", b"AAAAA")[:4] == ([("I", 1), ("=", 4)], 1, 5, 4)   # equal scores: the smaller j
    assert ext_align(b"CAA", b"AAA")[:4] == ([], 0, 0, 0)      # -3 + 1 + 1 stays below 0


def test_oracle_random_tails():
    rng = random.Random(21)
    T = _text()
    seen, stopped = set(), 0
    for x in range(300):
        n = rng.randrange(1, 80)
        r = rng.randrange(100, 2000)
        a = _edit(rng, T[r:r + n + 6], 0.1)[:n]
        kw = (dict(), dict(We=3), dict(A=2, B=0, G=1), dict(A=1, B=4, G=6), dict(X=5))[x % 5]
        ops, score, bi, bj, rows = _self_check(a, T[r:r + n + 40], **kw)
        seen |= {op for op, _ in ops}
        stopped += rows < len(a)
    assert seen == set("IDX=") and stopped >= 3


def test_oracle_xdrop_and_ties():
    rng = random.Random(22)
    T = _text()
    far = T[700:720] + _dna(rng, 40) + T[760:860]
    rows = {X: _self_check(far, T[700:900], X=X) for X in (0, 10, 1000)}
    assert rows[0][2] < 60 and rows[10][2] < 60 and rows[1000][2] == 160 and rows[0][4] <= rows[10][4] < 160
    assert rows[1000][4] == 160 and rows[1000][1] > rows[10][1]
    # all mismatches: the best cell stays (0, 0)
    assert ext_align(b"A" * 12, b"C" * 40)[:4] == ([], 0, 0, 0)
    # ties keep the smaller i, then the smaller j
    assert ext_align(b"AC", b"AA")[:4] == ([("=", 1)], 1, 1, 1)


def test_extend_parser_flags():
    from bwtmi import map as mapcli
    a = mapcli.build_parser().parse_args(["in.fa", "reads.txt", "-o", "out.paf"])
    assert (a.extend, a.xdrop, a.ext_band, a.cigar) == (False, None, None, False)
    a = mapcli.build_parser().parse_args(["in.fa", "reads.txt", "--extend", "-o", "o"])
    assert (a.extend, a.xdrop, a.ext_band) == (True, None, None)
    a = mapcli.build_parser().parse_args(["in.fa", "reads.txt", "--extend", "--xdrop", "50", "--ext-band", "8", "-o", "o"])
    assert (a.extend, a.xdrop, a.ext_band, a.align_band) == (True, 50, 8, None)
    with pytest.raises(SystemExit):
        mapcli.build_parser().parse_args(["in.fa", "reads.txt", "--xdrop", "x", "-o", "o"])


def test_align_result_stays_positional():
    from bwtmi.core import AlignResult
    z = np.zeros(0, np.int32)
    r = AlignResult(np.zeros(1, np.int64), z, z, z, z, z, z, z, z, 5, (1, 2, 3))
    assert (r.cells_total, r.gaps, r.head_score, r.tail_score, r.ext_rows) == (5, (1, 2, 3), None, None, None)
    assert AlignResult(np.zeros(1, np.int64), z, z, z, z, z, z, z, z).ext_rows is None


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def env(gpu_ctx):
    from bwtmi import BWTCore
    T = _text()
    return T, BWTCore(T, build_kmer=False)


@pytest.fixture(scope="module")
def pair_env(gpu_ctx):
    from bwtmi import BWTCore
    T, blocks = _pair_text()
    return T, blocks, BWTCore(T, build_kmer=False)


def _kw(We=None, A=None, B=None, G=None, X=None):
    return dict(ext_band=We, match=A, mismatch=B, gap=G, xdrop=X)


def _run(core, T, items, what=None, W=None, **p):
    queries, arrays = _chains(items)
    want = extend_oracle(T, queries, arrays, 32 if W is None else W, **{**DEFAULTS, **p})
    got = core.align_chains(queries, arrays, band=W, extend=True, **_kw(**p))
    assert_equal_ext(got, want, what)
    return got, want


@gpu
@pytest.mark.parametrize("We", [0, 1, 32])
@pytest.mark.parametrize("X", [0, 2, 1000])
def test_every_pair_over_two_letters(pair_env, We, X):
    """every string over {A, C} of up to 4 bytes against every one of up to 5, as a tail and as a head"""
    T, blocks, core = pair_env
    items = []
    for a in _two_letter(4):
        for b, at in blocks.items():
            assert T[at:at + len(b)] == b
            items.append(_tail(a, at))
            items.append(_head(a, at + len(b)))
    assert len(items) == 2 * 31 * 63
    got, want = _run(core, T, items, (We, X), We=We, X=X)
    assert got.gaps == (0, 0, 0) and (got.head_score > 0).sum() > 300 and (got.tail_score > 0).sum() > 300
    assert {cigar_text(h + t) for h, t in want["ends"]} >= {"", "1=", "4="}


@gpu
def test_text_edges(env):
    T, core = env
    n = len(T)
    rng = random.Random(31)
    S = T[n - 60:n - 10]
    items = [
        (S[:40] + T[n - 20:n - 10] + b"N" * 30, 0, [(0, n - 60, 40)]),           # a tail that meets the text's end: n < m
        (S[:40] + T[n - 20:], 0, [(0, n - 60, 40)]),                             # ... with the text's last byte in it
        (_dna(rng, 30) + T[0:8] + T[8:40], 0, [(38, 8, 32)]),                     # a head that meets the text's start: r_0 < q_0
        (T[0:40], 0, [(8, 8, 32)]),                                              # ... and reaches it exactly
        (T[300:340], 0, [(0, 300, 40)]), (T[300:340], 1, [(0, 300, 40)]),        # q_0 = 0 and qe_last = |S|: no extension
        (T[n - 30:] + b"ACGT", 0, [(0, n - 30, 30)]),                            # re_last = tn: n = 0
        (b"ACGT" + T[:30], 1, [(4, 0, 30)]),                                     # r_0 = 0: n = 0
    ]
    got, want = _run(core, T, items)
    assert want["ends"][0][1] and want["ends"][2][0] and int(got.rend[0]) == n - 10
    assert int(got.rstart[2]) == 0 and int(got.rstart[3]) == 0 and got.cigar_string(3) == "40="
    assert got.head_score[4:].tolist() == [0] * 4 and got.tail_score[4:].tolist() == [0] * 4
    assert [got.cigar_string(k) for k in (4, 5, 6, 7)] == ["40=", "40=", "30=", "30="]
    _run(core, T, items, "We 0", We=0)


@gpu
@pytest.mark.parametrize("We", [31, 32, 33, 95, 1024])
def test_band_widths(env, We):
    """bands of 63, 65, 67, 191 and 2049 columns (the wave's chunks of 64; the widest the LDS rows hold)"""
    T, core = env
    rng = random.Random(32)
    items = []
    for x in range(12):
        r = rng.randrange(300, 2400)
        b = T[r:r + 46] if x % 2 else T[r - 6:r + 40][::-1]        # what the rule reads, in its order
        u, v = rng.randrange(6, 16), rng.randrange(22, 32)
        a = (b[:u] + b[u + 1:v] + _dna(rng, 1) + b[v:])[:40]       # one base gone, one base more
        items.append(_tail(a, r, x % 4 == 3) if x % 2 else _head(a, r + 40, x % 4 == 2))
    got, want = _run(core, T, items, We, We=We, X=1000)
    assert {op for h, t in want["ends"] for op, _ in h + t} >= set("=ID")
    assert all(sum(ops_consume(e)) >= 70 for h, t in want["ends"] for e in (h, t) if e)       # both indels crossed


@gpu
def test_xdrop(env):
    """20 matches, 40 random bases, 100 matches: a small X stops before the far match, a large one crosses it"""
    T, core = env
    rng = random.Random(22)
    far = T[700:720] + _dna(rng, 40) + T[760:860]
    raf = T[1140:1160][::-1] + _dna(rng, 40) + T[1000:1100][::-1]      # the same shape, read backwards from 1160
    for X, crosses in ((0, False), (10, False), (1000, True)):
        got, want = _run(core, T, [_tail(far, 700), _head(raf, 1160)], X, X=X)
        assert got.ext_rows == want["ext_rows"] and got.tail_score.tolist() == want["tail_score"].tolist()
        assert got.head_score.tolist() == want["head_score"].tolist()
        assert (got.ext_rows == 320) == crosses and (got.ext_rows < 120) != crosses
        assert (int(got.qend[0]) == 161) == crosses and (int(got.qstart[1]) == 0) == crosses
        assert (int(got.tail_score[0]) >= 40) == crosses and (int(got.head_score[1]) >= 40) == crosses


@gpu
def test_ties(gpu_ctx):
    from bwtmi import BWTCore
    rng = random.Random(37)
    unit, left, right = b"ACGTTGCA", b"GGATCCTTGGATCCAAGGTTAACCGGTTCCAA", b"TTCCAAGGTTCCAAGG"
    T = _dna(rng, 600) + left + unit * 6 + right + _dna(rng, 600) + b"$"
    core = BWTCore(T, build_kmer=False)
    at = 600
    read = left + unit * 5 + right + T[at + 96:at + 126]                  # one copy missing in the read
    items = [
        (T[100:130] + b"N" * 20, 0, [(0, 100, 30)]),                     # no byte of the tail is in the text
        (b"N" * 20 + T[100:130], 1, [(20, 100, 30)]),
        (read, 0, [(0, at, 32)]),                                        # the tail runs through the tract
        (read, 0, [(len(read) - 30, at + 96, 30)]),                      # and the head
        (read, 1, [(0, at, 32)]),
    ]
    got, want = _run(core, T, items, X=1000)
    assert [got.cigar_string(k) for k in (0, 1)] == ["30=", "30="]
    assert (int(got.qstart[0]), int(got.qend[0]), int(got.qstart[1]), int(got.qend[1])) == (0, 30, 0, 30)
    assert got.tail_score[:2].tolist() == [0, 0] and got.head_score[:2].tolist() == [0, 0]
    for k in (2, 3, 4):
        assert sum(n for op, n in decode(got, k) if op == "D") == 8 == int(got.nm[k]), got.cigar_string(k)
        assert (int(got.qstart[k]), int(got.qend[k])) == (0, len(read))
    # the deletion sits where the preference puts it: not at the same end of the tract from both sides
    assert got.cigar_string(2) != got.cigar_string(3)


@gpu
def test_other_bytes_and_both_strands(gpu_ctx):
    """N, lower case and an absent byte in heads and tails, against a text with N runs; every searched string on
    both strands, and every read on both strands"""
    from bwtmi import BWTCore
    T = _build_texts()["gaps"]
    core = BWTCore(T, build_kmer=False)
    items = [(T[390:400] + b"NN" + T[402:412].lower() + T[412:440] + b"x" + T[441:470], 0, [(24, 414, 14)]),
             (T[1570:1650], 0, [(30, 1600, 20)]), (b"NNNN" + T[1604:1660] + b"nnnn", 0, [(10, 1610, 30)]),
             (T[1990:2070], 0, [(20, 2010, 25), (50, 2040, 10)])]
    both = []
    for S, _, anchors in items:
        both += [(S, 0, anchors), (S, 1, anchors),
                 (revcomp(S), 1, [(5, 500, 20)])]                        # the first one's read, searched on strand 1
    queries, arr = _chains(both)
    assert all(queries[3 * k] == queries[3 * k + 2] != queries[3 * k + 1] for k in range(len(items)))
    for We in (32, 0):
        got, want = _run(core, T, both, We, We=We)
        assert got.head_score[0::3].tolist() == got.head_score[1::3].tolist()
        assert got.tail_score[0::3].tolist() == got.tail_score[1::3].tolist()
    assert all(h and t for h, t in want["ends"][9:11]) and any(h for h, _ in want["ends"][:9])


@gpu
def test_long_tail(gpu_ctx):
    """3,000 rows at We = 8 (17 columns), and the same strings mirrored as a head; then a band of three chunks"""
    from bwtmi import BWTCore
    rng = random.Random(33)
    T = _dna(rng, 4000) + b"$"
    a = _edit(rng, T[500:3560], 0.01)[:3000]
    assert len(a) == 3000
    core = BWTCore(T, build_kmer=False)
    got, want = _run(core, T, [_tail(a, 500)], We=8, X=100)
    assert int(got.tail_score[0]) > 2500 and got.ext_rows == 3000 and int(got.qend[0]) == 3001
    Tm = T[:-1][::-1] + b"$"                                            # T[500 + j] is Tm[3499 - j]
    core_m = BWTCore(Tm, build_kmer=False)
    got_m, want_m = _run(core_m, Tm, [_head(a, 3500)], We=8, X=100)
    assert got_m.head_score.tolist() == got.tail_score.tolist() and got_m.ext_rows == 3000
    assert int(got_m.qstart[0]) == 0 and int(got_m.rend[0]) - int(got_m.rstart[0]) == int(got.rend[0]) - int(got.rstart[0])
    _run(core, T, [_tail(a[:400], 500), _head(a[:400], 3500, 1)], We=95, X=100)


@gpu
@pytest.mark.parametrize("scores", [(2, 0, 1), (1, 4, 6)])
def test_other_scores(env, scores):
    T, core = env
    A, B, G = scores
    items = _edited_tails(random.Random(34), T, 50, 60)
    got, want = _run(core, T, items, scores, A=A, B=B, G=G)
    assert (got.head_score > 0).any() and (got.tail_score > 0).any()
    assert {op for h, t in want["ends"] for op, _ in h + t} >= set("=X")


def _expand(ops):
    return [op for op, n in ops for _ in range(n)]


@gpu
def test_the_middle_does_not_move(env):
    """the chains of test_gpu_align.test_chains_of_anchors: without the head and
    tail operations the oracle reports, the new entry's CIGARs are the old entry's"""
    T, core = env
    rng = random.Random(14)
    plain = _random_chains(rng, T, 90)              # they start and end on an anchor: no extension at all
    queries, arr = _chains(plain)
    got, want = _run(core, T, plain, "plain")
    old = core.align_chains(queries, arr)
    assert got.cigar.tolist() == old.cigar.tolist() and got.cells_total == old.cells_total
    assert got.ext_rows == 0 and not got.head_score.any() and not got.tail_score.any()
    items = []
    for S, st, anchors in plain:                    # the same chains inside edited flanks of the text
        r0, (q, r, l) = anchors[0][1], anchors[-1]
        x, y = rng.randrange(0, min(25, r0) + 1), rng.randrange(0, 25)
        left, right = _edit(rng, T[r0 - x:r0], 0.1), _edit(rng, T[r + l:r + l + y], 0.1)
        items.append((left + S + right, st, [(q + len(left), r, l) for q, r, l in anchors]))
    queries, arr = _chains(items)
    for W in (None, 0, 1):
        got, want = _run(core, T, items, W, W=W)
        old = core.align_chains(queries, arr, band=W)
        assert old.head_score is None and old.tail_score is None and old.ext_rows is None
        grew = 0
        for k, (h, t) in enumerate(want["ends"]):
            full = _expand(decode(got, k))
            nh, nt = len(_expand(h)), len(_expand(t))
            grew += nh + nt > 0
            assert _rle([(op, 1) for op in full[nh:len(full) - nt]]) == decode(old, k), (k, W)
            dh, dt = ops_consume(h), ops_consume(t)
            rev = bool(items[k][1])
            assert int(got.rstart[k]) == int(old.rstart[k]) - dh[1] and int(got.rend[k]) == int(old.rend[k]) + dt[1]
            assert int(got.qstart[k]) == int(old.qstart[k]) - (dt[0] if rev else dh[0])
            assert int(got.qend[k]) == int(old.qend[k]) + (dh[0] if rev else dt[0])
        assert grew > 20
        assert got.gaps == old.gaps and got.cells_total > old.cells_total


def _example(second):
    rng = random.Random(35)
    T = _dna(rng, 2000) + b"$"
    read = bytearray(T[700:850])
    for at in (10, second):
        read[at] = ord("A") if read[at] != ord("A") else ord("C")
    return T, bytes(read)


def test_example_on_the_oracle():
    T, read = _example(139)
    arr = SimpleNamespace(offsets=np.array([0, 1]), strand=np.array([0], np.uint8), member_offsets=np.array([0, 1]),
                          member_q=np.array([11], np.int32), member_r=np.array([711]), member_len=np.array([128], np.int32))
    want = extend_oracle(T, [read], arr)
    assert (want["head_score"].tolist(), want["tail_score"].tolist()) == ([7], [7])
    assert cigar_text(want["ends"][0][0] + [("=", 128)] + want["ends"][0][1]) == "10=1X128=1X10="


@gpu
def test_the_example(gpu_ctx):
    from bwtmi import BWTCore
    T, read = _example(139)
    core = BWTCore(T, build_kmer=False)
    res = core.map_batch([read])
    assert res.strand.size == 1
    got = core.align_chains([read], res, extend=True)
    assert_equal_ext(got, extend_oracle(T, [read], res))
    assert got.cigar_string(0) == "10=1X128=1X10=" and (int(got.qstart[0]), int(got.qend[0])) == (0, 150)
    assert (int(got.rstart[0]), int(got.rend[0])) == (700, 850) and int(got.nm[0]) == 2 and int(got.n_eq[0]) == 148
    assert (got.head_score.tolist(), got.tail_score.tolist()) == ([7], [7])
    plain = core.align_chains([read], res, extend=False)
    assert plain.cigar_string(0) == "128=" and (int(plain.qstart[0]), int(plain.qend[0])) == (11, 139)
    assert int(plain.nm[0]) == 0 and plain.head_score is None
    # both strands of the read give the same alignment
    rc = revcomp(read)
    res2 = core.map_batch([rc], both_strands=True)
    got2 = core.align_chains([rc], res2, extend=True)
    assert_equal_ext(got2, extend_oracle(T, [rc], res2))
    assert res2.strand.tolist() == [1] and got2.cigar_string(0) == "10=1X128=1X10="
    assert (int(got2.qstart[0]), int(got2.qend[0])) == (0, 150)
    # a substitution three bases from the end: they stay out
    T, read = _example(147)
    res = core.map_batch([read])
    got = core.align_chains([read], res, extend=True)
    assert_equal_ext(got, extend_oracle(T, [read], res))
    assert got.cigar_string(0) == "10=1X136=" and int(got.qend[0]) == 147 and got.tail_score.tolist() == [0]


# ------------------------------------------------------------------ arguments, the cap, the empty call
def _raw(lib, core, queries, arr, off=None, nchain=None, nmember=None, reserved=None, **fields):
    from bwtmi._lib import ExtendParams
    blob = np.frombuffer(b"".join(queries) or b"\0", dtype=np.uint8)
    if off is None:
        off = np.concatenate([[0], np.cumsum([len(q) for q in queries])])
    off = np.asarray(off, dtype=np.int64)
    p = ExtendParams()
    p.band = p.ext_band = p.match = p.mismatch = p.gap = p.xdrop = -1
    for k, v in fields.items():
        setattr(p, k, v)
    if reserved is not None:
        p.reserved[reserved] = 1
    cols = [np.ascontiguousarray(a, dtype=t) for a, t in ((arr.offsets, np.int64), (arr.strand, np.uint8),
                                                          (arr.member_offsets, np.int64), (arr.member_q, np.int32),
                                                          (arr.member_r, np.int64), (arr.member_len, np.int32))]
    ptrs = [C.c_void_p(0xdead) for _ in range(11)]
    nc, cells, rows = C.c_int64(-7), C.c_int64(-7), C.c_int64(-7)
    gaps = (C.c_int64 * 3)(-7, -7, -7)
    rc = lib.bwtmi_index_align_extend(core._ctx, core._h, blob.ctypes.data_as(C.c_void_p),
                                      off.ctypes.data_as(C.c_void_p), off.size - 1,
                                      *[a.ctypes.data_as(C.c_void_p) for a in cols],
                                      cols[1].size if nchain is None else nchain,
                                      cols[3].size if nmember is None else nmember, C.byref(p),
                                      *[C.byref(x) for x in ptrs], C.byref(nc), C.byref(cells), gaps, C.byref(rows))
    return rc, ptrs, [nc.value, cells.value] + list(gaps) + [rows.value]


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
        "ext_band 1025": dict(ext_band=1025),
        "match 0": dict(match=0),
        "match 65": dict(match=65),
        "mismatch 65": dict(mismatch=65),
        "gap 0": dict(gap=0),
        "gap 65": dict(gap=65),
        "xdrop above 2^20": dict(xdrop=(1 << 20) + 1),
        "reserved 0": dict(reserved=0),
        "reserved 1": dict(reserved=1),
        # every error of the old entry
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
    }
    for what, kw in bad.items():
        rc, ptrs, counts = _raw(built_lib, core, kw.pop("queries", queries), kw.pop("arr", arr), **kw)
        assert rc == E_ARG and built_lib.bwtmi_last_error(), what
        assert all(p.value is None for p in ptrs) and counts == [0] * 6, what
    # the limits themselves are legal
    rc, ptrs, counts = _raw(built_lib, core, queries, arr, ext_band=1024, match=64, mismatch=64, gap=64, xdrop=1 << 20)
    assert rc == 0
    for p in ptrs:
        built_lib.bwtmi_free(p)
    rc, ptrs, counts = _raw(built_lib, core, queries, arr, ext_band=0, mismatch=0, xdrop=0)
    assert rc == 0
    for p in ptrs:
        built_lib.bwtmi_free(p)
    for kw in (dict(ext_band=-1), dict(ext_band=1025), dict(match=0), dict(gap=0), dict(xdrop=-1), dict(band=1025),
               dict(mismatch=65)):
        with pytest.raises(ValueError):
            core.align_chains(queries, arr, extend=True, **kw)
    with pytest.raises(ValueError):
        core.align_chains(queries, arr, xdrop=5)               # an extension keyword without extend=True
    # the old entry goes on refusing a nonzero reserved field
    from test_gpu_align import _raw as _raw_old
    assert _raw_old(built_lib, core, queries, arr, reserved=1)[0] == E_ARG


@gpu
def test_cell_cap(env, built_lib):
    from bwtmi._lib import BwtmiError
    T, core = env
    rng = random.Random(36)
    items = _edited_tails(rng, T, 6, 40) + [_one_gap(_edit(rng, T[620:650], 0.2), 620, 30)]
    queries, arr = _chains(items)
    want = extend_oracle(T, queries, arr, 4, **{**DEFAULTS, "We": 5})
    total = want["cells_total"]
    assert total > 500
    got = core.align_chains(queries, arr, band=4, extend=True, ext_band=5, max_cells=total)
    assert_equal_ext(got, want)
    with pytest.raises(BwtmiError, match=str(total)) as e:
        core.align_chains(queries, arr, band=4, extend=True, ext_band=5, max_cells=total - 1)
    assert e.value.cells_total == total
    rc, ptrs, counts = _raw(built_lib, core, queries, arr, band=4, ext_band=5, max_cells=total - 1)
    assert rc == E_NOMEM and str(total).encode() in built_lib.bwtmi_last_error()
    assert all(p.value is None for p in ptrs) and counts == [0, total, 0, 0, 0, 0]
    assert_equal_ext(core.align_chains(queries, arr, band=4, extend=True, ext_band=5), want, "after the failure")


@gpu
def test_no_chains(env, built_lib):
    T, core = env
    none = SimpleNamespace(offsets=np.zeros(3, np.int64), strand=np.zeros(0, np.uint8), member_offsets=np.zeros(1, np.int64),
                           member_q=np.zeros(0, np.int32), member_r=np.zeros(0, np.int64),
                           member_len=np.zeros(0, np.int32))
    for queries, arr in (([b"ACGT", b"GG"], none), ([], SimpleNamespace(**{**vars(none), "offsets": np.zeros(1, np.int64)}))):
        res = core.align_chains(queries, arr, extend=True)
        assert len(res) == 0 and res.cigar_offsets.tolist() == [0] and res.cigar.size == 0 and res.cells_total == 0
        assert res.head_score.dtype == np.int32 and res.tail_score.dtype == np.int32 and res.head_score.size == 0
        assert res.ext_rows == 0 and res.gaps == (0, 0, 0)
        rc, ptrs, counts = _raw(built_lib, core, queries, arr)
        assert rc == 0 and counts == [0] * 6 and all(p.value not in (None, 0xdead) for p in ptrs)
        for p in ptrs:
            built_lib.bwtmi_free(p)
    # params = NULL and every count NULL
    queries, arr = _chains([_tail(T[300:320], 300)])
    blob, off = np.frombuffer(b"".join(queries), dtype=np.uint8), np.array([0, len(queries[0])], dtype=np.int64)
    ptrs, nc = [C.c_void_p() for _ in range(11)], C.c_int64()
    cols = (arr.offsets, arr.strand, arr.member_offsets, arr.member_q, arr.member_r, arr.member_len)
    assert built_lib.bwtmi_index_align_extend(core._ctx, core._h, blob.ctypes.data_as(C.c_void_p),
                                              off.ctypes.data_as(C.c_void_p), 1,
                                              *[a.ctypes.data_as(C.c_void_p) for a in cols], 1, 1, None,
                                              *[C.byref(p) for p in ptrs], C.byref(nc), None, None, None) == 0
    assert nc.value == 1 and C.cast(ptrs[10], C.POINTER(C.c_int32))[0] == 20
    for p in ptrs:
        built_lib.bwtmi_free(p)
