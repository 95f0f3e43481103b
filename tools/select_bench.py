"""Device timing of the chain selection (bwtmi.select_chains) on the
three workloads of tools/align_bench.py: the same seeded 10 Mbp
contig, one index with its reverse index, (short) 10,000 reads of 150 bp,
(long) 1,000 reads of 10 kbp through the long entry, (tract) the long reads
with 75 bases cut out of the middle; min_len 19, both strands, default chain,
selection and alignment parameters.  Recorded per workload:
  (a) the wall time of select_chains on the MapResult (min of the repeats after
      a warm call, every repeat listed, kernel statistics off) and the
      k_select_* and select_upload HIP-event times from one more call;
  (b) the counts: chains, primaries, kept;
  (c) align_chains and align_chains(extend=True) wall on all chains against the
      kept chains of the same MapResult (MapResult.take), with cells_total and
      ext_rows of both;
  (d) the route users had: the contract in plain Python on the same chains, its
      wall time, and its results asserted equal to the device's for every read.

    python tools/select_bench.py OUT.json [--bp N] [--reads N] [--long-reads N] [--long-bp M]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "tools"), os.path.join(REPO, "bwt-algorithm_amd")]

import numpy as np  # noqa: E402

from align_bench import _walls, align_digest, extend_digest, map_digest, workloads  # noqa: E402


def select_python(chain_off, score, qstart, qend, mask=50, pri_ratio=80, best_n=5, full=100):
    """The contract of bwtmi_select_chains (include/bwtmi.h) in plain Python."""
    n = len(score)
    parent, sub, mapq, keep = [0] * n, [0] * n, [0] * n, [0] * n
    for a, b in zip(chain_off[:-1], chain_off[1:]):
        P, kept = [], 0
        for c in sorted(range(a, b), key=lambda i: (-score[i], i)):
            par = None
            for p in P:
                ov = max(0, min(qend[c], qend[p]) - max(qstart[c], qstart[p]))
                if ov * 100 >= mask * min(qend[c] - qstart[c], qend[p] - qstart[p]):
                    par = p
                    break
            if par is None:
                P.append(c)
                parent[c], keep[c] = c - a, 1
                continue
            parent[c] = par - a
            if sub[par] == 0:
                sub[par] = score[c]
            if score[c] * 100 >= pri_ratio * score[par] and kept < best_n:
                keep[c], kept = 1, kept + 1
        for p in P:
            mapq[p] = 60 * (score[p] - sub[p]) * min(score[p], full) // (score[p] * full)
    return parent, sub, mapq, keep


def run(ctx, core, reads, long, reps):
    from bwtmi import _lib, select_chains
    from smem_bench import _kern
    res = core.map_batch(reads, min_len=19, both_strands=True, long=long)
    walls, (sel,) = _walls(lambda: select_chains(res, ctx), reps)
    _lib.kernel_stats(ctx, enable=True, reset=True)
    select_chains(res, ctx)
    ks = _lib.kernel_stats(ctx, enable=False, reset=True)
    # (d) the plain-Python route on the same rows
    rows = [np.asarray(a).tolist() for a in (res.offsets, res.score, res.qstart, res.qend)]
    t0 = time.perf_counter()
    parent, sub, mapq, keep = select_python(*rows)
    py_ms = round((time.perf_counter() - t0) * 1e3, 3)
    raw = _lib.select_chains(ctx, res.offsets, res.score, res.qstart, res.qend)
    for q in range(len(res)):
        a, b = int(res.offsets[q]), int(res.offsets[q + 1])
        for name, want in (("parent", parent), ("sub", sub), ("mapq", mapq), ("keep", keep)):
            assert raw[name][a:b].tolist() == want[a:b], (name, q)
    assert sel.keep.tolist() == [bool(v) for v in keep] and sel.mapq.tolist() == mapq
    # (c) alignment of all chains against the kept ones
    kept = res.take(sel.keep)
    out = {}
    for tag, r in (("all", res), ("kept", kept)):
        aw, aln = _walls(lambda: core.align_chains(reads, r), reps)
        ew, ext = _walls(lambda: core.align_chains(reads, r, extend=True), reps)
        out[tag] = dict(chains=int(r.strand.size), members=int(r.member_q.size),
                        align_wall_ms=min(aw), align_wall_ms_repeats=aw, cells_total=int(aln.cells_total),
                        extend_wall_ms=min(ew), extend_wall_ms_repeats=ew, extend_cells_total=int(ext.cells_total),
                        ext_rows=int(ext.ext_rows), align_sha256=align_digest(aln), extend_sha256=extend_digest(ext))
    sel_ms = sum(v[0] for k, v in ks.items() if k.startswith("k_select"))
    return dict(reads=len(reads), read_bp=len(reads[0]), long_entry=long, mask=50, pri_ratio=80, best_n=5, full=100,
                chains=int(res.strand.size), chains_per_read=round(res.strand.size / max(len(reads), 1), 2),
                primaries=int(sel.n_primary), kept=int(sel.n_kept), mapq60=int((sel.mapq == 60).sum()),
                mapq0_primaries=int(((sel.mapq == 0) & sel.primary).sum()),
                select_wall_ms=min(walls), select_wall_ms_repeats=walls, select_kernels_ms=round(sel_ms, 4),
                select_upload_ms=round(ks.get("select_upload", (0.0,))[0], 4),
                select_all_timed_ms=round(sum(v[0] for v in ks.values()), 4), kernels=_kern(ks),
                python_wall_ms=py_ms, python_equal=True, map_sha256=map_digest(res), align=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--bp", type=int, default=10_000_000)
    ap.add_argument("--reads", type=int, default=10_000)
    ap.add_argument("--long-reads", type=int, default=1000)
    ap.add_argument("--long-bp", type=int, default=10_000)
    a = ap.parse_args()
    from bwtmi import BWTCore, _lib
    from smem_bench import _contig
    ctx = _lib.ctx(0)
    seq = _contig(a.bp)
    core = BWTCore(seq + b"$", build_kmer=False, reverse_index=True)
    short, long = workloads(seq, a.reads, a.long_reads, a.long_bp)
    mid = a.long_bp // 2
    tract = [r[:mid] + r[mid + 75:] for r in long]
    runs = dict(bp=a.bp, short_reads=run(ctx, core, short, False, 5), long_reads=run(ctx, core, long, True, 3),
                tract_reads=run(ctx, core, tract, True, 3))
    core.clear()
    print(json.dumps(runs), flush=True)
    with open(a.out, "w") as fh:
        json.dump(dict(host=_lib.host_info(), **runs), fh, indent=1)


if __name__ == "__main__":
    main()
