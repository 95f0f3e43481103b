"""Device timing of the batched SMEM search (BWTCore.smem_batch) on
the set-up of tools/lib_kernels.py locate_runs: a seeded 10 Mbp synthetic
contig, 10,000 reads of 150 bp cut from it with 3 substitutions, half of them
reverse-complemented, min_len 19, both strands.  Recorded: the wall time of the
call (min of 5 after a warm call, kernel statistics off), every kernel's
HIP-event time from one more call, `work`, the SMEM and position counts, the
rank kernel's rate in steps per ns -- and the route that existed before, in
the same run on the same index: each read's substrings through one
backward_search_batch call, the SMEM rule on the host, locate_positions per
seed, for as many reads as finish in --route-seconds; equal results asserted.

    python tools/smem_bench.py OUT.json [--route-seconds S] [--tree DIR]

(--tree: the package of another checkout, as below; the run carries a digest
of the call's arrays, so that two trees can be held against each other.)

With --untouched: only the searches this feature does not touch (k_bsearch2 /
k_bsearch over the 145,338 motifs, locate_batch at k = 0 and k = 2), from the
package under --tree (default: this tree), so that two trees can be run
alternately; prints one JSON line with the kernel times and a digest of the
results.

    python tools/smem_bench.py --untouched [--tree DIR]

With --long: the long-read entry (BWTCore.smem_long_batch) on the
same contig, one index built with its reverse index.  Three records: (1) the
workload above through smem_batch and smem_long_batch in turn, equal digests
asserted, each entry's wall time (min of 5, the two alternating) and kernel
times; (2) 1,000 reads of 10 kbp cut from the contig with 1 % substitutions,
half reverse-complemented, min_len 19, both strands, through smem_long_batch
(smem_batch refuses them): wall time, the walk kernel's time, `steps`, `work`;
(3) the wall time of the index build with and without the reverse index.

    python tools/smem_bench.py --long OUT.json [--long-reads N] [--long-bp M]"""
import argparse
import hashlib
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _kern(ks):
    return {k: dict(ms=round(v[0], 4), launches=v[1], alg_bytes=v[2])
            for k, v in sorted(ks.items(), key=lambda kv: -kv[1][0])}


def _contig(n):
    from bwtmi import synth
    return synth.generate_contig(n, 500 + n % 97, 0.02)


def make_reads(seq, nreads, m, nsub, seed=9000):
    T = np.frombuffer(seq, dtype=np.uint8)
    r = np.random.default_rng(seed)
    reads = []
    for i, st in enumerate(r.integers(0, len(seq) - m, nreads).tolist()):
        q = T[st:st + m].copy()
        for j in r.choice(m, size=nsub, replace=False).tolist():
            q[j] = r.choice([c for c in b"ACGT" if c != q[j]])
        p = q.tobytes()
        reads.append(p.translate(COMP)[::-1] if i % 2 else p)
    return reads


def substring_route(core, read, min_len, max_occ):
    """The SMEMs of one read on both strands with the calls that existed before
    smem_batch: (qstart, qend, strand, count, positions) rows by (strand, qstart)."""
    rows, m = [], len(read)
    for strand, Q in enumerate((read, read.translate(COMP)[::-1])):
        if strand and Q == read:
            break
        s = Q.decode()
        subs = [s[a:e] for e in range(1, m + 1) for a in range(e)]
        iv = core.backward_search_batch(subs)
        ok = iv[:, 0] >= 0
        ell, at = np.zeros(m + 2, dtype=np.int64), 0
        for e in range(1, m + 1):
            hit = np.flatnonzero(ok[at:at + e])          # starts a = 0 .. e - 1: the first that occurs
            ell[e] = e - hit[0] if hit.size else 0
            at += e
        mine = []
        for e in range(1, m + 1):
            if ell[e] >= min_len and (e == m or ell[e + 1] <= ell[e]):
                a = e - int(ell[e])
                pos = core.locate_positions(s[a:e])
                mine.append((m - e, m - a, 1, len(pos), pos) if strand else (a, e, 0, len(pos), pos))
        rows += sorted(mine)
    return [r[:4] + ((r[4] if r[3] <= max_occ else []),) for r in rows]


def smem_runs(ctx, n, nreads, m, nsub, min_len, route_seconds, reps=5):
    from bwtmi import BWTCore, _lib
    seq = _contig(n)
    core = BWTCore(seq + b"$", build_kmer=False)
    reads = make_reads(seq, nreads, m, nsub)
    call = lambda: core.smem_batch(reads, min_len=min_len, both_strands=True)   # noqa: E731
    call()   # warm (slots, code objects)
    walls = []
    for _ in range(reps):
        t0 = time.perf_counter()
        got = call()
        walls.append(round((time.perf_counter() - t0) * 1e3, 3))
    _lib.kernel_stats(ctx, enable=True, reset=True)
    call()
    ks = _lib.kernel_stats(ctx, enable=False, reset=True)
    rank = "k_smem_ms2" if "k_smem_ms2" in ks else "k_smem_ms"
    run = dict(bp=n, call="smem", reads=nreads, read_bp=m, substitutions=nsub, min_len=min_len, both_strands=True,
               wall_ms=min(walls), wall_ms_repeats=walls, work=int(got.work), smems=int(got.qstart.size),
               positions=int(got.positions.size), positions_total=int(got.positions_total),
               lanes=2 * nreads * m, rank_kernel=rank, rank_kernel_ms=round(ks[rank][0], 4),
               rank_steps_per_ns=round(got.work / (ks[rank][0] * 1e6), 2),
               wall_us_per_read=round(min(walls) * 1e3 / nreads, 3), kernels=_kern(ks),
               results_sha256=hashlib.sha256(b"".join(
                   np.ascontiguousarray(a).tobytes() for a in (got.offsets, got.qstart, got.qend, got.strand, got.count,
                                                               got.pos_offsets, got.positions))).hexdigest()[:16])
    # the route that existed before, on the same index (fresh host state: the SA comes down again)
    core._sa = None
    t0, done = time.perf_counter(), 0
    while done < nreads and (done == 0 or time.perf_counter() - t0 < route_seconds):
        want = substring_route(core, reads[done], min_len, 1024)
        qs, qe, st, cnt, pos = got[done]
        mine = [(int(a), int(b), int(c), int(d), p.tolist()) for a, b, c, d, p in zip(qs, qe, st, cnt, pos)]
        assert mine == want, f"smem_batch differs from the substring route on read {done}"
        done += 1
    route = time.perf_counter() - t0
    run.update(route_reads=done, route_s=round(route, 3), route_ms_per_read=round(route * 1e3 / done, 3),
               speedup_vs_substring_route=round(route * 1e3 / done / (min(walls) / nreads), 1))
    core.clear()
    return run


def _digest(got):
    return hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in (
        got.offsets, got.qstart, got.qend, got.strand, got.count, got.pos_offsets, got.positions))).hexdigest()[:16]


def _timed(ctx, calls, reps=5):
    """name -> (walls ms, kernel statistics of one more call, last result); the
    calls alternate inside every repeat, after one warm call each."""
    from bwtmi import _lib
    out = {name: [[], None, None] for name in calls}
    for name, call in calls.items():
        call()
    for _ in range(reps):
        for name, call in calls.items():
            t0 = time.perf_counter()
            out[name][2] = call()
            out[name][0].append(round((time.perf_counter() - t0) * 1e3, 3))
    for name, call in calls.items():
        _lib.kernel_stats(ctx, enable=True, reset=True)
        call()
        out[name][1] = _lib.kernel_stats(ctx, enable=False, reset=True)
    return out


def _entry_record(walls, ks, got, rank):
    return dict(wall_ms=min(walls), wall_ms_repeats=walls, rank_kernel=rank, rank_kernel_ms=round(ks[rank][0], 4),
                kernels_ms=round(sum(v[0] for v in ks.values()), 4), work=int(got.work), steps=int(got.steps),
                smems=int(got.qstart.size), positions=int(got.positions.size), results_sha256=_digest(got),
                kernels=_kern(ks))


def long_runs(ctx, n, nreads, long_reads, long_bp):
    from bwtmi import BWTCore
    seq = _contig(n)
    text = seq + b"$"
    # (3) the build, with and without the reverse index, alternating
    builds = {"forward_only": [], "with_reverse": []}
    for rep in range(4):
        for name, flag in (("forward_only", False), ("with_reverse", True)):
            t0 = time.perf_counter()
            core = BWTCore(text, build_kmer=False, reverse_index=flag)
            if rep:      # (the first pair sizes the context's scratch)
                builds[name].append(round((time.perf_counter() - t0) * 1e3, 2))
            core.clear()
    build = dict(bp=n, build_kmer=False, wall_ms_forward_only=min(builds["forward_only"]),
                 wall_ms_with_reverse=min(builds["with_reverse"]), repeats=builds,
                 ratio=round(min(builds["with_reverse"]) / min(builds["forward_only"]), 3))
    core = BWTCore(text, build_kmer=False, reverse_index=True)
    # (1) the short reads through both entries
    reads = make_reads(seq, nreads, 150, 3)
    t = _timed(ctx, {"smem_batch": lambda: core.smem_batch(reads, min_len=19, both_strands=True),
                     "smem_long_batch": lambda: core.smem_long_batch(reads, min_len=19, both_strands=True)})
    short = _entry_record(*t["smem_batch"], "k_smem_ms2")
    long_ = _entry_record(*t["smem_long_batch"], "k_smem_walk2")
    assert short["results_sha256"] == long_["results_sha256"] and short["work"] == long_["work"]
    both = dict(bp=n, reads=nreads, read_bp=150, substitutions=3, min_len=19, both_strands=True,
                smem_batch=short, smem_long_batch=long_,
                wall_ratio_long_over_short=round(long_["wall_ms"] / short["wall_ms"], 3),
                kernels_ratio_long_over_short=round(long_["kernels_ms"] / short["kernels_ms"], 3),
                rank_kernel_ratio_long_over_short=round(long_["rank_kernel_ms"] / short["rank_kernel_ms"], 3))
    # (2) long reads: the long entry alone
    lreads = make_reads(seq, long_reads, long_bp, long_bp // 100, seed=9100)
    t = _timed(ctx, {"smem_long_batch": lambda: core.smem_long_batch(lreads, min_len=19, both_strands=True)}, reps=3)
    rec = _entry_record(*t["smem_long_batch"], "k_smem_walk2")
    rec.update(bp=n, reads=long_reads, read_bp=long_bp, substitutions=long_bp // 100, min_len=19, both_strands=True,
               lanes=2 * long_reads * long_bp, steps_per_work=round(rec["steps"] / rec["work"], 4),
               steps_per_query_byte=round(rec["steps"] / (2 * long_reads * long_bp), 3),
               walk_steps_per_ns=round(rec["steps"] / (rec["rank_kernel_ms"] * 1e6), 3),
               smem_batch="refuses queries past 1024 bytes: no comparison exists")
    core.clear()
    return dict(short_reads_both_entries=both, long_reads=rec, index_build=build)


def untouched(ctx, n=10_000_000):
    """The existing searches, from whichever tree `bwtmi` was imported from."""
    from bwtmi import BWTCore, MotifUtils, _lib
    seq = _contig(n)
    core = BWTCore(seq + b"$", build_kmer=False)
    motifs = [mo for k in range(1, 11) for mo in MotifUtils.enumerate_motifs(k)]
    blob, off = core.pack_patterns(motifs)
    out, h = {}, hashlib.sha256()
    for name, fm_bytes in (("k_bsearch2", 0), ("k_bsearch", 1)):
        with _lib.knobs(FM_BYTES=fm_bytes):
            core.backward_search_packed(blob, off)
            _lib.kernel_stats(ctx, enable=True, reset=True)
            for _ in range(5):
                iv = core.backward_search_packed(blob, off)
            ks = _lib.kernel_stats(ctx, enable=False, reset=True)
        out[name + "_us"] = round(ks[name][0] * 1e3 / ks[name][1], 2)
        h.update(iv.tobytes())
    T = np.frombuffer(seq, dtype=np.uint8)
    for k in (0, 2):
        r = np.random.default_rng(7000 + k)
        pats = []
        for i, st in enumerate(r.integers(0, n - 24, 10_000).tolist()):
            q = T[st:st + 24].copy()
            for j in r.choice(24, size=int(r.integers(0, k + 1)), replace=False).tolist():
                q[j] = r.choice([c for c in b"ACGT" if c != q[j]])
            p = q.tobytes()
            pats.append((p.translate(COMP)[::-1] if i % 2 else p).decode())
        call = lambda: core.locate_batch(pats, max_mismatches=k, both_strands=True)   # noqa: E731
        call()
        walls = []
        for _ in range(5):
            t0 = time.perf_counter()
            got = call()
            walls.append((time.perf_counter() - t0) * 1e3)
        _lib.kernel_stats(ctx, enable=True, reset=True)
        call()
        ks = _lib.kernel_stats(ctx, enable=False, reset=True)
        out[f"locate_k{k}_wall_ms"] = round(min(walls), 3)
        out[f"locate_k{k}_kernels_ms"] = round(sum(v[0] for v in ks.values()), 4)
        out[f"locate_k{k}_seed_ms"] = round(ks["k_loc_seed2"][0], 4)
        out[f"locate_k{k}_kernels"] = {name: round(v[0], 4) for name, v in sorted(ks.items())}
        for a in (got.offsets, got.positions, got.mismatches, got.strand):
            h.update(a.tobytes())
    out["results_sha256"] = h.hexdigest()[:16]
    core.clear()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--route-seconds", type=float, default=60.0)
    ap.add_argument("--untouched", action="store_true")
    ap.add_argument("--long", action="store_true")
    ap.add_argument("--long-reads", type=int, default=1000)
    ap.add_argument("--long-bp", type=int, default=10_000)
    ap.add_argument("--tree", default=REPO)
    ap.add_argument("--bp", type=int, default=10_000_000)
    ap.add_argument("--reads", type=int, default=10_000)
    a = ap.parse_args()
    sys.path[:0] = [REPO, os.path.join(os.path.abspath(a.tree), "bwt-algorithm_amd")]
    from bwtmi import _lib
    ctx = _lib.ctx(0)
    if a.untouched:
        print(json.dumps(dict(tree=os.path.abspath(a.tree), lib=_lib.source_hash()[:12], **untouched(ctx, a.bp))),
              flush=True)
        return
    if a.long:
        runs = long_runs(ctx, a.bp, a.reads, a.long_reads, a.long_bp)
        print(json.dumps(runs), flush=True)
        with open(a.out, "w") as fh:
            json.dump(dict(host=_lib.host_info(), **runs), fh, indent=1)
        return
    run = smem_runs(ctx, a.bp, a.reads, 150, 3, 19, a.route_seconds)
    print(json.dumps(run), flush=True)
    with open(a.out, "w") as fh:
        json.dump(dict(host=_lib.host_info(), runs=[run]), fh, indent=1)


if __name__ == "__main__":
    main()
