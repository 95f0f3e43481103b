"""bwtmi_chain_anchors: the device chainer on a caller's anchors against a plain
Python restatement of the contract (include/bwtmi.h) written here: sort by (re,
qe), the integer DP with its break and its strict comparison, the extraction by
(f descending, index).  Every output array must be exactly equal, and so must
the DP's evaluated-predecessor count."""
import ctypes as C
import random

import numpy as np
import pytest

DEFAULTS = dict(max_gap=5000, bandwidth=500, max_pred=1024, min_score=40, min_anchors=1)
SMALL = dict(max_gap=200, bandwidth=50, max_pred=16, min_score=30, min_anchors=2)


# ------------------------------------------------------------------ the oracle
def cost(d):
    return 0 if d == 0 else (d >> 4) + (d.bit_length() >> 1)


def chain_group(anch, max_gap, bandwidth, max_pred, min_score, min_anchors):
    """One group's chains: ([(score, [input indices in chain order])], evaluated predecessors)."""
    order = sorted(range(len(anch)), key=lambda t: (anch[t][1] + anch[t][2], anch[t][0] + anch[t][2]))   # stable
    a = [anch[t] for t in order]
    A, f, p, evals = len(a), [t[2] for t in a], [-1] * len(a), 0
    for i in range(A):
        qi, ri, li = a[i]
        for j in range(i - 1, max(0, i - max_pred) - 1, -1):
            qj, rj, lj = a[j]
            dr = ri + li - rj - lj
            if dr > max_gap:
                break
            evals += 1
            dq = qi + li - qj - lj
            if dq <= 0 or dr <= 0 or dq > max_gap:
                continue
            d = abs(dr - dq)
            if d > bandwidth:
                continue
            s = f[j] + min(li, dq, dr) - cost(d)
            if s > f[i]:
                f[i], p[i] = s, j
    used, chains = [False] * A, []
    for i in sorted(range(A), key=lambda i: (-f[i], i)):
        if used[i]:
            continue
        mem, k = [], i
        while k >= 0 and not used[k]:
            used[k] = True
            mem.append(k)
            k = p[k]
        score = f[i] - (f[k] if k >= 0 else 0)
        if score >= min_score and len(mem) >= min_anchors:
            chains.append((score, [order[x] for x in reversed(mem)]))
    return chains, evals


def chain_oracle(groups, **params):
    """The call's expected arrays for groups = [[(q, r, len), ...], ...]."""
    P = dict(DEFAULTS, **{k: v for k, v in params.items() if v is not None})
    out = {k: [] for k in ("score", "n_anchors", "qstart", "qend", "rstart", "rend", "member")}
    coff, moff, base, evals = [0], [0], 0, 0
    for g in groups:
        chains, ev = chain_group(g, **P)
        evals += ev
        for score, mem in chains:
            m = [g[t] for t in mem]
            out["score"].append(score)
            out["n_anchors"].append(len(m))
            out["qstart"].append(min(q for q, r, l in m))
            out["qend"].append(max(q + l for q, r, l in m))
            out["rstart"].append(min(r for q, r, l in m))
            out["rend"].append(max(r + l for q, r, l in m))
            out["member"] += [base + t for t in mem]
            moff.append(len(out["member"]))
        coff.append(len(out["score"]))
        base += len(g)
    kinds = dict(score=np.int32, n_anchors=np.int32, qstart=np.int32, qend=np.int32, rstart=np.int64, rend=np.int64,
                 member=np.int64)
    want = {k: np.array(v, dtype=kinds[k]) for k, v in out.items()}
    want["chain_off"], want["member_off"], want["evals"] = np.array(coff, np.int64), np.array(moff, np.int64), evals
    return want


_ARRAYS = ("chain_off", "score", "n_anchors", "qstart", "qend", "rstart", "rend", "member_off", "member")


def flat(groups):
    off = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int64)
    rows = [a for g in groups for a in g]
    cols = [np.array([a[k] for a in rows], dtype=t) for k, t in ((0, np.int32), (1, np.int64), (2, np.int32))]
    return (off, *cols)


def run(ctx, groups, **params):
    """The device's result for the groups, held against the oracle's."""
    from bwtmi import _lib
    got = _lib.chain_anchors(ctx, *flat(groups), **params)
    want = chain_oracle(groups, **params)
    for k in _ARRAYS:
        assert got[k].dtype == want[k].dtype, (k, got[k].dtype)
        assert got[k].shape == want[k].shape and got[k].tolist() == want[k].tolist(), (k, params)
    assert got["evals"] == want["evals"], params
    return got


def random_group(rng, n, qmax=400, rmax=600, lmin=5, lmax=40):
    return [(rng.randint(0, qmax), rng.randint(0, rmax), rng.randint(lmin, lmax)) for _ in range(n)]


def colinear_group(rng, n, noise=0.2):
    """A dense, mostly colinear group: a diagonal with small indels, some anchors off it."""
    out, q, r = [], 0, 1000
    for _ in range(n):
        q += rng.randint(1, 6)
        r += rng.randint(1, 6)
        if rng.random() < noise:
            out.append((rng.randint(0, 3 * n), 1000 + rng.randint(0, 3 * n), rng.randint(3, 25)))
        else:
            out.append((q, r, rng.randint(3, 25)))
    return out


# ------------------------------------------------------------------ CPU: the oracle itself
def test_oracle_on_a_hand_made_group():
    # A -> B -> C on one diagonal; D branches off B and stops in front of it
    g = [(0, 0, 20), (30, 30, 20), (60, 60, 20), (60, 75, 15)]
    chains, evals = chain_group(g, 200, 50, 16, 10, 1)
    assert chains == [(60, [0, 1, 2]), (53 - 40, [3])] and evals == 6
    assert cost(0) == 0 and cost(1) == 0 and cost(15) == 2 and cost(16) == 3 and cost(500) == 31 + 4


# ------------------------------------------------------------------ GPU
gpu = pytest.mark.gpu


@gpu
def test_group_sizes_in_one_call(gpu_ctx):
    rng = random.Random(11)
    groups = [random_group(rng, n) for n in (0, 1, 2, 63, 64, 65, 200, 0)]
    got = run(gpu_ctx, groups, **dict(SMALL, max_pred=100, min_anchors=1))
    assert got["score"].size > 20 and np.diff(got["chain_off"]).tolist()[0] == 0 and got["n_anchors"].max() > 3
    run(gpu_ctx, groups, **SMALL)
    run(gpu_ctx, groups)            # the defaults


@gpu
def test_many_small_groups(gpu_ctx):
    rng = random.Random(12)
    groups = [random_group(rng, rng.randint(1, 5), 60, 80) for _ in range(300)]
    got = run(gpu_ctx, groups, **dict(SMALL, min_score=20, min_anchors=1))
    assert got["chain_off"].size == 301 and got["score"].size > 300 and (got["n_anchors"] > 1).any()
    one = run(gpu_ctx, groups[150:151], **dict(SMALL, min_score=20, min_anchors=1))
    a, b = got["chain_off"][150:152].tolist()
    assert one["score"].tolist() == got["score"][a:b].tolist()


@gpu
@pytest.mark.parametrize("max_pred", [1, 63, 64, 65, 100])
def test_window_edges(gpu_ctx, max_pred):
    rng = random.Random(max_pred)
    dense = colinear_group(rng, 400)
    # the only predecessor of the last anchor is the first, K anchors that chain with nothing (dq < 0) back:
    # K = max_pred - 1 is the window's last place, K = max_pred is outside it
    edge = []
    for K in (max_pred - 1, max_pred, max_pred + 1, max(0, max_pred - 2)):
        edge.append([(0, 0, 50)] + [(900 - k, 50 + k, 1) for k in range(K)] + [(60, 50 + K + 11, 10)])
    got = run(gpu_ctx, [dense] + edge, max_gap=1000, bandwidth=500, max_pred=max_pred, min_score=1)
    heads = [got["n_anchors"][got["chain_off"][g]] for g in (1, 2, 3, 4)]
    assert heads == [2, 1, 1, 2]
    assert got["n_anchors"][got["chain_off"][0]] > (1 if max_pred == 1 else 20)


@gpu
def test_equal_scores_take_the_nearest(gpu_ctx):
    # P1 and P2 cannot chain (dq = 0); C reaches both with s = 20: P2, the nearer, wins
    p1, p2, c = (7, 7, 13), (10, 26, 10), (50, 66, 10)
    assert 13 + 10 - cost(16) == 10 + 10 - cost(0) == 20
    got = run(gpu_ctx, [[p1, p2, c]], min_score=1)
    assert got["score"].tolist() == [20, 13] and got["member"].tolist() == [1, 2, 0]
    # the same with 70 incompatible anchors between them: P1 is in the second window of 64
    noise = [(900 + k, 20 + k % 15, 1) for k in range(70)]      # (they chain among themselves: f <= 15)
    got = run(gpu_ctx, [[p1] + noise + [p2, c]], min_score=20)
    assert got["member"].tolist()[:2] == [71, 72]
    # a farther predecessor with a higher score still wins across windows
    got = run(gpu_ctx, [[(6, 6, 14)] + noise + [p2, c]], min_score=21)
    assert got["score"].tolist()[0] == 21 and got["member"].tolist()[:2] == [0, 72]


@gpu
def test_equal_f_and_equal_ends(gpu_ctx):
    # isolated anchors with one f: chains in index order, that is by (re, qe), ties in input order
    rng = random.Random(5)
    far = [(rng.randint(0, 5), 1000 * k, 50) for k in rng.sample(range(300), 300)]
    got = run(gpu_ctx, [far, far[:64], far[:65]], max_gap=500, bandwidth=100)
    assert got["score"].tolist() == [50] * 429 and got["member"][:300].tolist() == sorted(range(300), key=lambda t: far[t][1])
    # equal (re, qe) with different starts, and exact duplicates: stability decides the index
    same = [(10, 10, 10), (5, 5, 15), (10, 10, 10), (0, 0, 20), (5, 5, 15)] * 30 + [(40, 40, 10), (40, 40, 10)]
    got = run(gpu_ctx, [same, list(reversed(same))], min_score=1)
    # of the thirty (0, 0, 20) that give (40, 40, 10) the same score the last, the nearest, is taken; the
    # second (40, 40, 10) then stops in front of it
    assert got["n_anchors"].tolist()[:2] == [2, 1] and got["member"].tolist()[:3] == [148, 150, 151]
    assert got["score"].tolist()[:2] == [30, 10]
    rng = random.Random(6)
    run(gpu_ctx, [[(q, r, l) for q, r, l in random_group(rng, 500, 12, 12, 1, 4)]], **dict(SMALL, min_score=3))


@gpu
def test_gap_and_band_limits(gpu_ctx):
    a, G, B = (10, 0, 20), 200, 50
    second = {"gap": (G, G), "gap+1": (G + 1, G + 1), "band": (G, G - B), "band+1": (G, G - B - 1),
              "dq-gap+1": (G + 1, G), "band-r": (G - B, G), "band-r+1": (G - B - 1, G),
              "dq=0": (0, 30), "dq<0": (-5, 30), "dr=0": (30, 0)}
    groups = [[a, (10 + dq, dr, 20)] for dq, dr in second.values()]      # equal lengths: the ends differ by (dq, dr)
    got = run(gpu_ctx, groups, max_gap=G, bandwidth=B, min_score=1)
    chained = [int(got["n_anchors"][got["chain_off"][g]]) == 2 for g in range(len(groups))]
    assert dict(zip(second, chained)) == {"gap": True, "gap+1": False, "band": True, "band+1": False, "dq-gap+1": False,
                                          "band-r": True, "band-r+1": False, "dq=0": False, "dq<0": False, "dr=0": False}
    assert int(got["score"][got["chain_off"][2]]) == 40 - cost(B)


@gpu
def test_coordinate_limits(gpu_ctx):
    top = 1 << 32
    g = [(100, top - 400, 50), (200, top - 300, 50), (300, top - 200, 50), ((1 << 24) - 60, top - 60, 60),
         (0, 0, 30), (40, 40, 30)]
    got = run(gpu_ctx, [g, g[:4]], max_gap=1 << 25, bandwidth=1 << 25, min_score=1)
    assert got["rend"].max() == top and got["qend"].max() == 1 << 24 and got["n_anchors"].max() >= 3
    run(gpu_ctx, [g], max_gap=2147483647, bandwidth=2147483647, max_pred=4096, min_score=1)


@gpu
def test_chain_stops_in_front_of_a_used_anchor(gpu_ctx):
    g = [(0, 0, 20), (30, 30, 20), (60, 60, 20), (60, 75, 15)]
    got = run(gpu_ctx, [g], max_gap=200, bandwidth=50, min_score=10)
    assert got["score"].tolist() == [60, 13] and got["n_anchors"].tolist() == [3, 1]
    assert got["member"].tolist() == [0, 1, 2, 3] and got["member_off"].tolist() == [0, 3, 4]
    assert (got["qstart"].tolist(), got["qend"].tolist()) == ([0, 60], [80, 75])
    assert (got["rstart"].tolist(), got["rend"].tolist()) == ([0, 75], [80, 90])
    # the truncated chain falls to min_score / min_anchors; its marks stay
    assert run(gpu_ctx, [g], max_gap=200, bandwidth=50, min_score=14)["score"].tolist() == [60]
    assert run(gpu_ctx, [g], max_gap=200, bandwidth=50, min_score=10, min_anchors=2)["score"].tolist() == [60]
    assert run(gpu_ctx, [g], max_gap=200, bandwidth=50, min_score=61)["score"].tolist() == []


@gpu
def test_random_groups(gpu_ctx):
    rng = random.Random(7)
    groups = [random_group(rng, rng.randint(1, 28)) for _ in range(200)]
    assert sum(map(len, groups)) <= 3000
    got = run(gpu_ctx, groups, **SMALL)
    assert got["score"].size > 200 and got["n_anchors"].min() >= 2 and got["score"].min() >= 30
    # chains are colinear: both ends strictly increase along the members
    q, r, l = flat(groups)[1:]
    for k in range(got["score"].size):
        m = got["member"][got["member_off"][k]:got["member_off"][k + 1]]
        assert np.all(np.diff(q[m] + l[m]) > 0) and np.all(np.diff(r[m] + l[m]) > 0)
    run(gpu_ctx, groups, **dict(SMALL, min_anchors=1, min_score=1, max_pred=3))
    dense = [colinear_group(rng, n) for n in (700, 130, 1)]
    got = run(gpu_ctx, dense, max_gap=60, bandwidth=20, max_pred=200, min_score=25)
    assert got["n_anchors"].max() > 50
    run(gpu_ctx, dense)


# ------------------------------------------------------------------ arguments, raw C ABI
def _raw(lib, ctx, off, q, r, ln, params=None, null=()):
    from bwtmi._lib import ChainParams
    off = np.asarray(off, np.int64)
    q, r, ln = np.asarray(q, np.int32), np.asarray(r, np.int64), np.asarray(ln, np.int32)
    p = ChainParams()
    for k, v in (params or {}).items():
        if k == "reserved":
            p.reserved[v] = 1
        else:
            setattr(p, k, v)
    ptrs = [C.c_void_p(0xdead) for _ in range(9)]
    counts = [C.c_int64(-7) for _ in range(3)]
    arg = lambda name, a: None if name in null else a.ctypes.data_as(C.c_void_p)      # noqa: E731
    rc = lib.bwtmi_chain_anchors(ctx, arg("off", off), off.size - 1, arg("q", q), arg("r", r), arg("len", ln),
                                 C.byref(p), *[C.byref(x) for x in ptrs], *[C.byref(v) for v in counts])
    return rc, ptrs, [v.value for v in counts]


@gpu
def test_c_abi_reports_argument_errors(gpu_ctx, built_lib):
    ok = ([0, 2], [0, 30], [0, 30], [20, 20])
    bad = [(([0, 2, 1], [0, 30], [0, 30], [20, 20]), {}, ()),          # decreasing offsets
           (([-1, 2], [0, 30, 0], [0, 30, 0], [20, 20, 20]), {}, ()),  # a negative offset
           (([1, 2], [0, 30], [0, 30], [20, 20]), {}, ()),             # does not start at 0
           (([0, 2], [0, 30], [0, 30], [20, 0]), {}, ()),              # len < 1
           (([0, 2], [0, -1], [0, 30], [20, 20]), {}, ()),             # q < 0
           (([0, 2], [0, (1 << 24) - 19], [0, 30], [20, 20]), {}, ()),  # qe > 2^24
           (([0, 2], [0, 30], [0, -30], [20, 20]), {}, ()),            # r < 0
           (([0, 2], [0, 30], [0, (1 << 32) - 19], [20, 20]), {}, ()),  # re > 2^32
           (ok, {}, ("q",)), (ok, {}, ("r",)), (ok, {}, ("len",)), (ok, {}, ("off",)),
           (ok, {"max_pred": 4097}, ()), (ok, {"bandwidth": 5001}, ()), (ok, {"max_gap": 400}, ()),   # default band 500
           (ok, {"max_gap": 10, "bandwidth": 11}, ()),
           (ok, {"reserved": 0}, ()), (ok, {"reserved": 2}, ())]
    for arrays, params, null in bad:
        rc, ptrs, counts = _raw(built_lib, gpu_ctx, *arrays, params=params, null=null)
        assert rc == -1 and built_lib.bwtmi_last_error(), (arrays, params, null)
        assert all(p.value == 0xdead for p in ptrs) and counts == [-7, -7, -7]       # untouched
    # the limits themselves are legal, and so are the largest parameters
    rc, ptrs, counts = _raw(built_lib, gpu_ctx, [0, 2], [0, (1 << 24) - 20], [0, (1 << 32) - 20], [20, 20],
                            params={"max_pred": 4096, "max_gap": 500, "bandwidth": 500})
    assert rc == 0 and counts[:2] == [0, 0] and all(p.value not in (None, 0xdead) for p in ptrs)
    for p in ptrs:
        built_lib.bwtmi_free(p)
    from bwtmi import _lib
    with pytest.raises(ValueError, match="4096"):
        _lib.chain_anchors(gpu_ctx, *flat([[(0, 0, 5)]]), max_pred=5000)
    with pytest.raises(ValueError):
        _lib.chain_anchors(gpu_ctx, *flat([[(0, 0, 0)]]))
    with pytest.raises(TypeError):
        _lib.chain_anchors(gpu_ctx, *flat([[(0, 0, 5)]]), max_gaps=5)


@gpu
def test_no_groups_and_empty_groups(gpu_ctx, built_lib):
    rc, ptrs, counts = _raw(built_lib, gpu_ctx, [0], [], [], [], null=("q", "r", "len"))
    assert rc == 0 and counts == [0, 0, 0] and all(p.value not in (None, 0xdead) for p in ptrs)
    assert C.cast(ptrs[0], C.POINTER(C.c_int64))[0] == 0 and C.cast(ptrs[7], C.POINTER(C.c_int64))[0] == 0
    for p in ptrs:
        built_lib.bwtmi_free(p)
    got = run(gpu_ctx, [])
    assert got["chain_off"].tolist() == [0] and got["member_off"].tolist() == [0]
    got = run(gpu_ctx, [[], [], []])
    assert got["chain_off"].tolist() == [0, 0, 0, 0] and got["score"].size == 0
    got = run(gpu_ctx, [[], [(3, 4, 50)], []])
    assert got["chain_off"].tolist() == [0, 0, 1, 1] and got["member"].tolist() == [0]
