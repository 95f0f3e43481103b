"""Device timing of the north_star library kernels off the CLI path (VERDICT r2
#7): Kasai LCP (k_isa, k_kasai; bwt.py:56-95, 2108-2116), the LCP plateau scan
(k_plateau_*; 2118-2145, 2500-2560), the Hamming seed-and-extend table
(k_extend; 2027-2095, 2697-2805 -- the reference skips it above 1 Mbp),
Tier 1 (k_t1_flags; 1426-1538), Tier 3 anchoring (k_t3_windows; 2828-3036) and
the simple period scan (k_simple_extend; 2177-2498), on seeded synthetic
contigs of the given sizes.  Per call: wall ms and every kernel's HIP-event
time, launches and algorithmic bytes (KLAUNCH models) -> GB/s.  Then the
batched locate (k_loc_seed2, k_loc_verify, the hit sort, k_loc_unpack) on a 10
Mbp contig with 10,000 patterns, against the per-pattern route (locate_runs).

usage: python tools/lib_kernels.py [--locate-only] OUT.json [bp ...]   (default 1e6 1e7)"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "bwt-algorithm_amd")]

import numpy as np  # noqa: E402


def _kern(ks):
    return {k: dict(ms=round(v[0], 4), launches=v[1], alg_bytes=v[2],
                    gbs=round(v[2] / (v[0] / 1e3) / 1e9, 1) if v[0] > 0 and v[2] > 0 else None)
            for k, v in sorted(ks.items(), key=lambda kv: -kv[1][0])}


def locate_runs(ctx, n=10_000_000, npat=10_000, m=24, reps=5):
    """BWTCore.locate_batch on a seeded synthetic contig: `npat` patterns of `m`
    bp cut from the text, each with up to k random substitutions, half of them
    reverse-complemented; k = 0, 1, 2 on both strands.  And, for k = 0 on one
    strand only, the route that existed before: the Python loop over
    BWTCore.locate_positions on the same index, suffix-array download included.
    Wall times are taken with the kernel statistics off (`reps` repeats after a
    warm call; min and every repeat), the per-kernel times in one more call."""
    from bwtmi import BWTCore, _lib, synth
    seq = synth.generate_contig(n, 500 + n % 97, 0.02)
    T = np.frombuffer(seq, dtype=np.uint8)
    core = BWTCore(seq + b"$", build_kmer=False)
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    runs = []

    def patterns(k):
        r = np.random.default_rng(7000 + k)
        pats = []
        for i, st in enumerate(r.integers(0, n - m, npat).tolist()):
            q = T[st:st + m].copy()
            for j in r.choice(m, size=int(r.integers(0, k + 1)), replace=False).tolist():
                q[j] = r.choice([c for c in b"ACGT" if c != q[j]])
            p = q.tobytes()
            pats.append((p.translate(comp)[::-1] if i % 2 else p).decode())
        return pats

    def timed(fn):
        fn()   # warm (slots, code objects)
        walls = []
        for _ in range(reps):
            t0 = time.perf_counter()
            got = fn()
            walls.append(round((time.perf_counter() - t0) * 1e3, 3))
        return got, walls

    for k, both in ((0, False), (0, True), (1, True), (2, True)):
        pats = patterns(k)
        call = lambda: core.locate_batch(pats, max_mismatches=k, both_strands=both)   # noqa: E731
        got, walls = timed(call)
        _lib.kernel_stats(ctx, enable=True, reset=True)
        call()
        ks = _lib.kernel_stats(ctx, enable=False, reset=True)
        run = dict(bp=n, call="locate", k=k, both_strands=both, patterns=npat, pattern_bp=m, wall_ms=min(walls),
                   wall_ms_repeats=walls, hits=int(got.positions.size), candidates=int(got.candidates),
                   kernels=_kern(ks))
        if k == 0 and not both:
            # the per-pattern route on the same index (fresh host state: the SA comes down again)
            def loop():
                core._sa = None
                return [core.locate_positions(p) for p in pats]
            t0 = time.perf_counter()
            want = loop()
            loop_ms = [round((time.perf_counter() - t0) * 1e3, 3)]
            t0 = time.perf_counter()
            loop()
            loop_ms.append(round((time.perf_counter() - t0) * 1e3, 3))
            assert [got[i][0].tolist() for i in range(npat)] == want, "batched locate differs from locate_positions"
            run["per_pattern_route_ms"] = min(loop_ms)
            run["per_pattern_route_ms_repeats"] = loop_ms
            run["speedup_vs_per_pattern_route"] = round(min(loop_ms) / min(walls), 1)
        runs.append(run)
        print(json.dumps(run), flush=True)
    core.clear()
    return runs


def main():
    args = sys.argv[1:]
    locate_only = "--locate-only" in args
    args = [a for a in args if a != "--locate-only"]
    out = args[0]
    sizes = [int(float(x)) for x in args[1:]] or [999_000, 10_000_000]
    from bwtmi import BWTCore, _lib, synth
    from bwtmi.tiers import Tier1STRFinder, Tier2LCPFinder, Tier3LongReadFinder
    ctx = _lib.ctx(0)
    res = dict(host=_lib.host_info(), runs=[])
    for n in ([] if locate_only else sizes):
        seq = synth.generate_contig(n, 500 + n % 97, 0.02)
        text = seq + b"$"
        r = np.random.default_rng(n % 1000)
        reads = [seq[a:a + 5000].decode() for a in r.integers(0, n - 5000, 64).tolist()]
        core = BWTCore(text)
        f = Tier2LCPFinder(core)
        calls = [("lcp", lambda: core.lcp_array()),
                 ("lcp_plateaus", lambda: f._detect_lcp_plateaus(None, "c")),
                 ("tier1", lambda: Tier1STRFinder(np.frombuffer(text, dtype=np.uint8), 9).find_strs("c")),
                 ("tier3", lambda: Tier3LongReadFinder(core).find_very_long_repeats(reads, "c"))]
        if n < 1_000_000:   # bwt.py:2048: the reference returns [] above 1 Mbp (text incl. '$')
            calls.append(("short_imperfect", lambda: f.find_short_imperfect_repeats("c", set())))
            calls.append(("long_repeats", lambda: f.find_long_repeats("c", set())))
        for name, fn in calls:
            fn()   # warm (slots, code objects)
            _lib.kernel_stats(ctx, enable=True, reset=True)
            t0 = time.perf_counter()
            got = fn()
            wall = (time.perf_counter() - t0) * 1e3
            ks = _lib.kernel_stats(ctx, enable=False, reset=True)
            res["runs"].append(dict(bp=n, call=name, wall_ms=round(wall, 3), records=len(got), kernels=_kern(ks)))
            print(json.dumps(res["runs"][-1]), flush=True)
        core.clear()
    res["runs"] += locate_runs(ctx)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
