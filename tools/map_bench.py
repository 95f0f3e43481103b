"""Device timing of batched read mapping (BWTCore.map_batch) on the
two workloads of tools/smem_bench.py, on the same seeded 10 Mbp synthetic
contig and one index built with its reverse index: (short) 10,000 reads of
150 bp with 3 substitutions, (long) 1,000 reads of 10 kbp with 1 %
substitutions through the long entry; half of the reads reverse-complemented,
min_len 19, both strands, default chain parameters.  Recorded per workload:
the wall time of the call (min of 5 after a warm call, kernel statistics off),
every kernel's HIP-event time from one more call (chain_upload is the
re-upload of the seeds as anchors, timed on the stream like a kernel), the
anchors, chains and the DP's evaluated predecessors, the wall time of the SMEM
entry alone on the same reads -- and the route that existed before, in the
same run on the same index: that SMEM entry, then the chain rules on the host
in plain Python, for as many reads as finish in --route-seconds; equal results
asserted read by read.

    python tools/map_bench.py OUT.json [--route-seconds S] [--bp N] [--reads N] [--long-reads N] [--long-bp M]
"""
import argparse
import hashlib
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "tools"), os.path.join(REPO, "bwt-algorithm_amd")]

import numpy as np  # noqa: E402
from smem_bench import _contig, _kern, make_reads  # noqa: E402

MAX_GAP, BANDWIDTH, MAX_PRED, MIN_SCORE, MIN_ANCHORS = 5000, 500, 1024, 40, 1


def _cost(d):
    return 0 if d == 0 else (d >> 4) + (d.bit_length() >> 1)


def host_chains(anch):
    """The contract of include/bwtmi.h on one group's anchors (q, r, len), in
    plain Python: [(score, [anchors in chain order])] in extraction order."""
    a = sorted(anch, key=lambda t: (t[1] + t[2], t[0] + t[2]))
    A, f, p = len(a), [t[2] for t in a], [-1] * len(a)
    for i in range(A):
        qi, ri, li = a[i]
        for j in range(i - 1, max(0, i - MAX_PRED) - 1, -1):
            qj, rj, lj = a[j]
            dr = ri + li - rj - lj
            if dr > MAX_GAP:
                break
            dq = qi + li - qj - lj
            if dq <= 0 or dr <= 0 or dq > MAX_GAP:
                continue
            d = abs(dr - dq)
            if d > BANDWIDTH:
                continue
            s = f[j] + min(li, dq, dr) - _cost(d)
            if s > f[i]:
                f[i], p[i] = s, j
    used, out = [False] * A, []
    for i in sorted(range(A), key=lambda i: (-f[i], i)):
        if used[i]:
            continue
        mem, k = [], i
        while k >= 0 and not used[k]:
            used[k] = True
            mem.append(k)
            k = p[k]
        score = f[i] - (f[k] if k >= 0 else 0)
        if score >= MIN_SCORE and len(mem) >= MIN_ANCHORS:
            out.append((score, [a[x] for x in reversed(mem)]))
    return out


def host_route(sm, i, m):
    """Read i's chains from the SMEM result `sm`: rows (strand, score, members in
    the original read's coordinates), by strand, then extraction order."""
    qs, qe, st, cnt, pos = sm[i]
    rows = []
    for strand in (0, 1):
        anch = [((m - int(e)) if strand else int(s), int(p), int(e - s))
                for s, e, t, ps in zip(qs, qe, st, pos) if t == strand for p in ps.tolist()]
        for score, mem in host_chains(anch):
            rows.append((strand, score, [((m - q - l) if strand else q, r, l) for q, r, l in mem]))
    return rows


def _digest(got):
    return hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in (
        got.offsets, got.strand, got.score, got.n_anchors, got.qstart, got.qend, got.rstart, got.rend,
        got.member_offsets, got.member_q, got.member_r, got.member_len))).hexdigest()[:16]


def _walls(call, reps):
    call()   # warm (slots, code objects)
    walls, got = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        got = call()
        walls.append(round((time.perf_counter() - t0) * 1e3, 3))
    return walls, got


def run(ctx, core, reads, long, route_seconds, reps=5):
    from bwtmi import _lib
    seed = core.smem_long_batch if long else core.smem_batch
    smem_walls, sm = _walls(lambda: seed(reads, min_len=19, both_strands=True), reps)
    call = lambda: core.map_batch(reads, min_len=19, both_strands=True, long=long)   # noqa: E731
    walls, got = _walls(call, reps)
    _lib.kernel_stats(ctx, enable=True, reset=True)
    call()
    ks = _lib.kernel_stats(ctx, enable=False, reset=True)
    chain_ms = sum(v[0] for k, v in ks.items() if k.startswith("k_chain"))
    upload_ms = ks.get("chain_upload", (0.0,))[0]
    all_ms = sum(v[0] for v in ks.values())
    rec = dict(reads=len(reads), read_bp=len(reads[0]), long_entry=long, min_len=19, both_strands=True,
               chain_params=dict(max_gap=MAX_GAP, bandwidth=BANDWIDTH, max_pred=MAX_PRED, min_score=MIN_SCORE,
                                 min_anchors=MIN_ANCHORS),
               wall_ms=min(walls), wall_ms_repeats=walls, smem_entry_wall_ms=min(smem_walls),
               smem_entry_wall_ms_repeats=smem_walls, wall_ms_over_smem_entry=round(min(walls) - min(smem_walls), 3),
               anchors=int(got.anchors), chains=int(got.score.size), members=int(got.member_q.size),
               skipped_smems=int(got.skipped_smems), dp_evaluated_predecessors=int(got.evals),
               dp_ms=round(ks["k_chain_dp"][0], 4),
               dp_evals_per_ns=round(got.evals / (ks["k_chain_dp"][0] * 1e6), 4),
               chain_kernels_ms=round(chain_ms, 4), chain_upload_ms=round(upload_ms, 4),
               chain_upload_share_of_wall=round(upload_ms / min(walls), 4), all_timed_ms=round(all_ms, 4),
               kernels=_kern(ks), results_sha256=_digest(got))
    # the route that existed before: the SMEM entry (timed above), then the chain rules on the host
    t0, done = time.perf_counter(), 0
    while done < len(reads) and (done == 0 or time.perf_counter() - t0 < route_seconds):
        want = host_route(sm, done, len(reads[done]))
        strand, score, n, qs, qe, rs, re, mem = got[done]
        mine = [(int(s), int(c), [tuple(row) for row in m.tolist()]) for s, c, m in zip(strand, score, mem)]
        assert mine == want, f"map_batch differs from the host route on read {done}"
        done += 1
    host = time.perf_counter() - t0
    route_ms_per_read = min(smem_walls) / len(reads) + host * 1e3 / done
    rec.update(route="the SMEM entry, then the chain rules in plain Python (no numpy in the DP)", route_reads=done,
               route_host_chain_s=round(host, 3), route_ms_per_read=round(route_ms_per_read, 4),
               speedup_vs_host_route=round(route_ms_per_read / (min(walls) / len(reads)), 2))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--route-seconds", type=float, default=30.0)
    ap.add_argument("--bp", type=int, default=10_000_000)
    ap.add_argument("--reads", type=int, default=10_000)
    ap.add_argument("--long-reads", type=int, default=1000)
    ap.add_argument("--long-bp", type=int, default=10_000)
    a = ap.parse_args()
    from bwtmi import BWTCore, _lib
    ctx = _lib.ctx(0)
    seq = _contig(a.bp)
    core = BWTCore(seq + b"$", build_kmer=False, reverse_index=True)
    runs = dict(bp=a.bp,
                short_reads=run(ctx, core, make_reads(seq, a.reads, 150, 3), False, a.route_seconds),
                long_reads=run(ctx, core, make_reads(seq, a.long_reads, a.long_bp, a.long_bp // 100, seed=9100), True,
                               a.route_seconds, reps=3))
    core.clear()
    print(json.dumps(runs), flush=True)
    with open(a.out, "w") as fh:
        json.dump(dict(host=_lib.host_info(), **runs), fh, indent=1)


if __name__ == "__main__":
    main()
