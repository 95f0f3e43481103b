"""bwtmi_select_chains: the device selection of a read's chains against a plain
Python restatement of the contract (include/bwtmi.h) written here: the rank by
(score descending, input index), the sequential parent walk over the list of
primaries, the keep test with its per-group counter, the MAPQ with `//`.  The
four output arrays must be exactly equal, dtypes included, and so must both
counts."""
import ctypes as C
import os
import random

import numpy as np
import pytest

DEFAULTS = dict(mask=50, pri_ratio=80, best_n=5, full=100)
TIGHT = dict(mask=90, pri_ratio=100, best_n=1, full=40)
LOOSE = dict(mask=1, pri_ratio=0, best_n=1000, full=1 << 20)
SETS = (DEFAULTS, TIGHT, LOOSE, dict(mask=100, pri_ratio=33, best_n=0, full=1), dict(mask=37, best_n=2))


# ------------------------------------------------------------------ the oracle
def select_group(rows, mask, pri_ratio, best_n, full):
    """One group's (parent, sub, mapq, keep) for rows = [(score, qstart, qend), ...]."""
    n = len(rows)
    parent, sub, mapq, keep, P, kept = [0] * n, [0] * n, [0] * n, [0] * n, [], 0
    for c in sorted(range(n), key=lambda i: (-rows[i][0], i)):
        sc, cs, ce = rows[c]
        par = None
        for p in P:
            ps, pe = rows[p][1:]
            ov = max(0, min(ce, pe) - max(cs, ps))
            if ov * 100 >= mask * min(ce - cs, pe - ps):
                par = p
                break
        if par is None:
            P.append(c)
            parent[c], keep[c] = c, 1
            continue
        parent[c] = par
        if sub[par] == 0:
            sub[par] = sc
        if sc * 100 >= pri_ratio * rows[par][0] and kept < best_n:
            keep[c], kept = 1, kept + 1
    for p in P:
        s1 = rows[p][0]
        mapq[p] = 60 * (s1 - sub[p]) * min(s1, full) // (s1 * full)
    return parent, sub, mapq, keep


def select_oracle(groups, **params):
    """The call's expected arrays and counts for groups = [[(score, qstart, qend), ...], ...]."""
    P = dict(DEFAULTS, **{k: v for k, v in params.items() if v is not None})
    cols = ([], [], [], [])
    n_primary = 0
    for g in groups:
        got = select_group(g, **P)
        n_primary += sum(1 for i, p in enumerate(got[0]) if p == i)
        for dst, src in zip(cols, got):
            dst += src
    kinds = (np.int32, np.int32, np.uint8, np.uint8)
    want = {k: np.array(v, dtype=t) for k, v, t in zip(("parent", "sub", "mapq", "keep"), cols, kinds)}
    want["n_primary"], want["n_kept"] = n_primary, int(sum(cols[3]))
    return want


def flat(groups):
    off = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int64)
    rows = [r for g in groups for r in g]
    return (off, *[np.array([r[k] for r in rows], dtype=np.int32) for k in range(3)])


def run(ctx, groups, **params):
    """The device's result for the groups, held against the oracle's."""
    from bwtmi import _lib
    got = _lib.select_chains(ctx, *flat(groups), **params)
    want = select_oracle(groups, **params)
    for k in ("parent", "sub", "mapq", "keep"):
        assert got[k].dtype == want[k].dtype, (k, got[k].dtype)
        assert got[k].shape == want[k].shape and got[k].tolist() == want[k].tolist(), (k, params)
    assert (got["n_primary"], got["n_kept"]) == (want["n_primary"], want["n_kept"]), params
    return got


def random_group(rng, n, span=300, smax=200):
    out = []
    for _ in range(n):
        a = rng.randint(0, span)
        out.append((rng.randint(1, smax), a, a + rng.randint(10, 120)))
    return out


# ------------------------------------------------------------------ CPU: the oracle itself
def test_oracle_on_a_hand_made_group():
    # 100 is primary; 90 lies inside it (secondary, kept: 90 >= 80); 60 beside both (primary, unique)
    g = [(90, 10, 90), (100, 0, 100), (60, 200, 260), (70, 0, 100)]
    assert select_group(g, **DEFAULTS) == ([1, 1, 2, 1], [0, 90, 0, 0], [0, 6, 36, 0], [1, 1, 1, 0])
    want = select_oracle([g, []])
    assert (want["n_primary"], want["n_kept"]) == (2, 3) and want["mapq"].dtype == np.uint8


# ------------------------------------------------------------------ GPU
gpu = pytest.mark.gpu


@gpu
def test_no_groups_empty_groups_and_one_chain(gpu_ctx):
    got = run(gpu_ctx, [])
    assert got["parent"].size == 0 and (got["n_primary"], got["n_kept"]) == (0, 0)
    run(gpu_ctx, [[], [], []])
    got = run(gpu_ctx, [[], [(50, 3, 40)], [], [], [(200, 0, 10), (7, 0, 10)], []])
    assert got["parent"].tolist() == [0, 0, 0] and got["mapq"].tolist() == [30, 57, 0]
    got = run(gpu_ctx, [[(100, 5, 6)]])
    assert (got["parent"].tolist(), got["sub"].tolist(), got["mapq"].tolist(), got["keep"].tolist()) == ([0], [0], [60], [1])


@gpu
def test_equal_scores_rank_by_input_index(gpu_ctx):
    got = run(gpu_ctx, [[(70, 0, 100), (70, 0, 100), (70, 0, 100)], [(5, 0, 9), (70, 1, 50), (70, 0, 50)]])
    assert got["parent"].tolist() == [0, 0, 0, 1, 1, 1] and got["sub"].tolist() == [70, 0, 0, 0, 70, 0]
    assert got["mapq"].tolist() == [0] * 6 and got["keep"].tolist() == [1, 1, 1, 0, 1, 1]


@gpu
def test_mask_threshold(gpu_ctx):
    p = (100, 0, 100)
    # intervals of 100 and 60: overlap 30 meets mask 50 exactly, 29 misses it by one base
    got = run(gpu_ctx, [[p, (50, 70, 130)], [p, (50, 71, 131)], [(50, 70, 130), p], [(50, 71, 131), p]])
    assert got["parent"].tolist() == [0, 0, 0, 1, 1, 1, 0, 1]
    # nested inside a primary
    got = run(gpu_ctx, [[p, (50, 20, 40)], [(50, 20, 40), p], [p, (50, 99, 100)], [p, (50, 100, 101)]])
    assert got["parent"].tolist() == [0, 0, 1, 1, 0, 0, 0, 1]
    # 40 % of itself on each of two primaries: overlap is never summed
    got = run(gpu_ctx, [[p, (90, 120, 220), (50, 60, 160)]])
    assert got["parent"].tolist() == [0, 1, 2] and got["mapq"].tolist() == [60, 54, 30]
    # under two primaries: the first in rank order, not the larger overlap (55 against 65)
    got = run(gpu_ctx, [[(90, 100, 200), p, (50, 45, 165)], [p, (90, 100, 200), (50, 45, 165)]])
    assert got["parent"].tolist() == [0, 1, 1, 0, 1, 0] and got["sub"].tolist() == [0, 50, 0, 50, 0, 0]
    for mask in (1, 29, 30, 31, 100):
        run(gpu_ctx, [[p, (50, 70, 170)], [p, (50, 0, 100)], [p, (50, 1, 101)], [p, (99, 99, 100)]], mask=mask)


@gpu
def test_pri_ratio_threshold(gpu_ctx):
    p = (100, 0, 100)
    got = run(gpu_ctx, [[p, (80, 0, 100)], [p, (79, 0, 100)], [(199, 0, 9), (160, 0, 9), (159, 0, 9)]])
    assert got["keep"].tolist() == [1, 1, 1, 0, 1, 1, 0] and got["sub"].tolist() == [80, 0, 79, 0, 160, 0, 0]
    got = run(gpu_ctx, [[p, (100, 0, 100), (99, 0, 100)], [p, (1, 0, 100)]], pri_ratio=100)
    assert got["keep"].tolist() == [1, 1, 0, 1, 0]
    got = run(gpu_ctx, [[p, (1, 0, 100)]], pri_ratio=0)
    assert got["keep"].tolist() == [1, 1]


@gpu
def test_best_n_counts_per_group_in_rank_order(gpu_ctx):
    # two primaries; the secondaries 90 (of the first), 85 (of the second), 84 (of the first) in rank order
    g = [(100, 0, 100), (84, 0, 100), (95, 200, 300), (85, 200, 300), (90, 0, 100)]
    want = {0: [1, 0, 1, 0, 0], 1: [1, 0, 1, 0, 1], 2: [1, 0, 1, 1, 1], 3: [1, 1, 1, 1, 1]}
    for best_n, keep in want.items():
        got = run(gpu_ctx, [g, [], g], best_n=best_n)
        assert got["keep"].tolist() == keep * 2 and got["n_kept"] == 2 * sum(keep), best_n
        assert got["parent"].tolist() == [0, 0, 2, 2, 0] * 2 and got["sub"].tolist() == [90, 0, 85, 0, 0] * 2


@gpu
def test_mapq_full_above_and_below_the_score(gpu_ctx):
    got = run(gpu_ctx, [[(50, 0, 9)], [(100, 0, 9)], [(200, 0, 9)], [(200, 0, 9), (50, 0, 9)], [(30, 0, 9), (10, 0, 9)]])
    assert got["mapq"].tolist() == [30, 60, 60, 45, 0, 12, 0]
    got = run(gpu_ctx, [[(50, 0, 9)], [(1 << 30, 0, 1 << 28), ((1 << 30) - 1, 0, 1 << 28)], [(1 << 30, 0, 1)]], full=1 << 20)
    assert got["mapq"].tolist() == [0, 0, 0, 60]
    got = run(gpu_ctx, [[(50, 0, 9)], [(3, 0, 9), (1, 0, 9)]], full=1)
    assert got["mapq"].tolist() == [60, 40, 0]


@gpu
def test_group_sizes_and_parameter_sets(gpu_ctx):
    rng = random.Random(21)
    groups = [random_group(rng, n) for n in (1, 63, 64, 65, 130, 0, 2)]
    for params in SETS:
        got = run(gpu_ctx, groups, **params)
    assert got["parent"].size == 325
    # many primaries in groups at the window's edges: narrow intervals that touch but do not overlap
    groups = [[(rng.randint(1, 50), 10 * k, 10 * k + 10) for k in rng.sample(range(n), n)] for n in (63, 64, 65, 130)]
    got = run(gpu_ctx, groups)
    assert got["n_primary"] == 322 and got["keep"].all()
    # the same intervals twice: every second chain finds its parent in window 0, 1 or 2
    got = run(gpu_ctx, [g + [(s, a, b) for s, a, b in reversed(g)] for g in groups], pri_ratio=0, best_n=1000)
    assert got["n_primary"] == 322 and got["n_kept"] == 644


@gpu
def test_many_primaries_cross_the_list_windows(gpu_ctx):
    # 1,500 chains, mostly disjoint 8-base intervals: about 1,000 primaries, so the list leaves its first window
    # and the on-chip part of it; the later chains repeat an earlier interval and find their parents at every depth
    rng = random.Random(22)
    first = [(rng.randint(1, 1000), 10 * k, 10 * k + 8) for k in range(1000)]
    again = [(rng.randint(1, 1000), 10 * k + rng.randint(0, 2), 10 * k + 8) for k in rng.sample(range(1000), 500)]
    g = first + again
    rng.shuffle(g)
    got = run(gpu_ctx, [g[:7], g, g[:70]])
    assert got["n_primary"] > 1000 and np.count_nonzero(got["sub"]) > 300
    run(gpu_ctx, [g], **LOOSE)
    run(gpu_ctx, [g, g], **TIGHT)


@gpu
def test_one_primary_and_299_secondaries(gpu_ctx):
    rng = random.Random(23)
    g = [(rng.randint(1, 500), rng.randint(0, 20), rng.randint(80, 100)) for _ in range(300)]
    got = run(gpu_ctx, [g], pri_ratio=10, best_n=1000)
    top = max(range(300), key=lambda i: (g[i][0], -i))
    assert got["n_primary"] == 1 and set(got["parent"].tolist()) == {top} and got["n_kept"] > 100
    assert run(gpu_ctx, [g])["n_kept"] == 6


@gpu
def test_random_groups(gpu_ctx):
    rng = random.Random(24)
    groups = [random_group(rng, rng.randint(0, 40)) for _ in range(200)]
    for params in SETS:
        got = run(gpu_ctx, groups, **params)
    got = run(gpu_ctx, groups)
    assert 200 < got["n_primary"] < got["n_kept"] < got["parent"].size
    one = run(gpu_ctx, groups[77:78])
    a = sum(len(g) for g in groups[:77])
    assert one["parent"].tolist() == got["parent"][a:a + len(groups[77])].tolist()


@gpu
def test_merged_chains_of_real_reads(gpu_ctx, golden_dir):
    from bwtmi import BWTCore, merge_groups, select_chains
    from test_map_cli import _contigs
    contigs = _contigs(os.path.join(golden_dir, "inputs", "synth_small.fa"))
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    seq, last = contigs[0][1], contigs[-1][1]
    cut = seq[20:140]
    sub = cut[:30] + ("A" if cut[30] != "A" else "C") + cut[31:75] + ("G" if cut[75] != "G" else "T") + cut[76:]
    reads = [cut, sub, sub.encode().translate(comp)[::-1].decode(), cut[:50] + cut[58:], last[-60:], seq[300:360] + last[:60],
             "GATTACAGATTACAGATTACAGATTACA"]
    results = []
    for _, cseq in contigs:
        core = BWTCore(cseq.encode() + b"$", build_kmer=False)
        results.append(core.map_batch(reads, 12, True, False, 50, None, max_gap=400, bandwidth=60, min_score=20))
        core.clear()
    m = merge_groups(results)
    assert m["score"].size == sum(r.score.size for r in results) > len(reads) - 2
    groups = [[(int(m["score"][k]), int(m["qstart"][k]), int(m["qend"][k])) for k in range(a, b)]
              for a, b in zip(m["chain_off"][:-1].tolist(), m["chain_off"][1:].tolist())]
    for params in (DEFAULTS, LOOSE):
        got = run(gpu_ctx, groups, **params)
        sels = select_chains(results, gpu_ctx, **params)
        assert sum(int(s.primary.sum()) for s in sels) == got["n_primary"] == sels[0].n_primary
        assert sum(int(s.keep.sum()) for s in sels) == got["n_kept"] == sels[-1].n_kept
        for i, s in enumerate(sels):
            rows = np.flatnonzero(m["origin"][:, 0] == i)
            assert s.mapq.tolist() == got["mapq"][rows].tolist() and s.sub.tolist() == got["sub"][rows].tolist()
            assert s.mapq.dtype == np.uint8 and s.primary.dtype == bool and s.parent_chain.dtype == np.int64
    assert got["n_primary"] >= len(reads) - 1      # every read but the absent one has a placement


# ------------------------------------------------------------------ arguments
def _raw(lib, ctx, off, score, qs, qe, params=None, null=(), ng=None):
    from bwtmi._lib import SelectParams
    off = np.asarray(off, np.int64)
    score, qs, qe = (np.asarray(a, np.int32) for a in (score, qs, qe))
    p = SelectParams(-1, -1, -1, -1)
    for k, v in (params or {}).items():
        if k == "reserved":
            p.reserved[v] = 1
        else:
            setattr(p, k, v)
    ptrs = [C.c_void_p(0xdead) for _ in range(4)]
    counts = [C.c_int64(-7) for _ in range(2)]
    arg = lambda name, a: None if name in null else a.ctypes.data_as(C.c_void_p)      # noqa: E731
    rc = lib.bwtmi_select_chains(ctx, arg("off", off), off.size - 1 if ng is None else ng, arg("score", score),
                                 arg("qstart", qs), arg("qend", qe), None if params is None else C.byref(p),
                                 *[C.byref(x) for x in ptrs], *[C.byref(v) for v in counts])
    return rc, ptrs, [v.value for v in counts]


@gpu
def test_argument_errors(gpu_ctx, built_lib):
    from bwtmi import _lib
    ok = ([0, 2], [50, 40], [0, 10], [30, 60])
    bad = [(([0, 2, 1], [50], [0], [30]), {}, "chain_off"),               # decreasing offsets
           (([1, 2], [50, 40], [0, 10], [30, 60]), {}, "chain_off"),       # does not start at 0
           (([0, 2], [50, 40], [0, -1], [30, 60]), {}, "qstart"),
           (([0, 2], [50, 40], [0, 60], [30, 60]), {}, "qend"),            # qend <= qstart
           (([0, 2], [50, 40], [0, 10], [30, (1 << 28) + 1]), {}, "qend"),
           (([0, 2], [50, 0], [0, 10], [30, 60]), {}, "score"),
           (([0, 2], [50, (1 << 30) + 1], [0, 10], [30, 60]), {}, "score"),
           (ok, {"mask": 0}, "mask"), (ok, {"mask": 101}, "mask"), (ok, {"pri_ratio": 101}, "pri_ratio"),
           (ok, {"full": 0}, "full"), (ok, {"full": (1 << 20) + 1}, "full")]
    for arrays, params, name in bad:
        with pytest.raises(ValueError, match=name) as e:
            _lib.select_chains(gpu_ctx, *arrays, **params)
        assert "outputs were written" not in str(e.value), (arrays, params)
        # the contract's state after BWTMI_E_ARG: every output pointer NULL, every count 0
        rc, ptrs, counts = _raw(built_lib, gpu_ctx, *arrays, params=params)
        assert rc == -1 and name in built_lib.bwtmi_last_error().decode(), (arrays, params)
        assert all(p.value is None for p in ptrs) and counts == [0, 0]
    for k in range(4):
        with pytest.raises(ValueError, match="reserved"):
            _lib.select_chains(gpu_ctx, *ok, reserved=[0] * k + [1])
    rc, ptrs, counts = _raw(built_lib, gpu_ctx, *ok, ng=-1)
    assert rc == -1 and b"ng" in built_lib.bwtmi_last_error() and counts == [0, 0] and not any(p.value for p in ptrs)
    for name in ("off", "score", "qstart", "qend"):
        rc, ptrs, counts = _raw(built_lib, gpu_ctx, *ok, null=(name,))
        assert rc == -1 and {"off": b"chain_off"}.get(name, name.encode()) in built_lib.bwtmi_last_error()
        assert counts == [0, 0] and not any(p.value for p in ptrs)
    with pytest.raises(ValueError, match="best_n"):
        _lib.select_chains(gpu_ctx, *ok, best_n=-2)
    # the limits themselves are legal; params = NULL is all defaults; no chains still gives four arrays
    run(gpu_ctx, [[(1 << 30, 0, 1 << 28), (1, (1 << 28) - 1, 1 << 28)]], mask=100, pri_ratio=100, best_n=0, full=1 << 20)
    run(gpu_ctx, [[(1 << 30, 0, 1 << 28), (1, (1 << 28) - 1, 1 << 28)]], mask=1, pri_ratio=0, full=1)
    rc, ptrs, counts = _raw(built_lib, gpu_ctx, *ok)
    assert rc == 0 and counts == [1, 2] and all(p.value for p in ptrs)
    assert C.cast(ptrs[0], C.POINTER(C.c_int32))[1] == 0 and C.cast(ptrs[2], C.POINTER(C.c_uint8))[0] == 6
    for p in ptrs:
        built_lib.bwtmi_free(p)
    rc, ptrs, counts = _raw(built_lib, gpu_ctx, [0, 0], [], [], [], null=("score", "qstart", "qend"))
    assert rc == 0 and counts == [0, 0] and all(p.value not in (None, 0xdead) for p in ptrs)
    for p in ptrs:
        built_lib.bwtmi_free(p)
    # a good call after the refused ones still gives the right answer
    rng = random.Random(25)
    run(gpu_ctx, [random_group(rng, 30), random_group(rng, 3)])
