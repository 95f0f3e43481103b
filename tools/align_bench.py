"""Device timing of base-level alignment (BWTCore.align_chains) on
the two workloads of tools/map_bench.py, on the same seeded 10 Mbp synthetic
contig and one index built with its reverse index: (short) 10,000 reads of
150 bp with 3 substitutions, (long) 1,000 reads of 10 kbp with 1 %
substitutions through the long entry; half of the reads reverse-complemented,
min_len 19, both strands, default chain and alignment parameters -- and, since
substitutions alone leave almost every gap 1 x 1, (tract) the long reads again
with 75 bases cut out of the middle of each, which puts one gap of about
0..20 x 75..95 into every read's chain.  Recorded per workload: the wall time of
map_batch alone and of map_batch followed by align_chains (min of the repeats
after a warm call, every repeat listed, kernel statistics off), every kernel's
HIP-event time from one more pair of calls (align_upload is the chains' way back
up, timed on the stream like a kernel), the gaps by class, cells_total, and
digests of both results.

    python tools/align_bench.py OUT.json [--extend] [--bp N] [--reads N] [--long-reads N] [--long-bp M]

With --extend: every workload also through align_chains(extend=True)
on the same chains -- its wall time, the new kernels' times, ext_rows, the
extensions' cells, a digest, and the share of the reads whose first chain's
alignment spans the whole read, without and with extension.

With --untouched: only map_batch and the plain align_chains on the first two
workloads, from the package under --tree (default: this tree), so that two
trees can be run alternately; prints one JSON line with the wall times and the
result digests.

    python tools/align_bench.py --untouched [--tree DIR]
"""
import argparse
import hashlib
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "tools")]

import numpy as np  # noqa: E402


def _sha(arrays):
    return hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)).hexdigest()[:16]


def map_digest(got):   # tools/map_bench.py's
    return _sha((got.offsets, got.strand, got.score, got.n_anchors, got.qstart, got.qend, got.rstart, got.rend,
                 got.member_offsets, got.member_q, got.member_r, got.member_len))


def align_digest(got):
    return _sha((got.cigar_offsets, got.cigar, got.nm, got.n_eq, got.cols, got.qstart, got.qend, got.rstart, got.rend))


def _walls(call, reps):
    call()   # warm (slots, code objects)
    walls, got = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        got = call()
        walls.append(round((time.perf_counter() - t0) * 1e3, 3))
    return walls, got


def extend_digest(got):
    return _sha((got.cigar_offsets, got.cigar, got.nm, got.n_eq, got.cols, got.qstart, got.qend, got.rstart, got.rend,
                 got.head_score, got.tail_score))


def whole_read_share(reads, res, aln):
    """the share of the reads whose first chain's alignment spans the whole read"""
    first, has = res.offsets[:-1], res.offsets[1:] > res.offsets[:-1]
    qlen = np.array([len(r) for r in reads])
    k = first[has]
    return round(float(((aln.qstart[k] == 0) & (aln.qend[k] == qlen[has])).sum()) / max(len(reads), 1), 4)


def run_extend(ctx, core, reads, res, aln, reps):
    """align_chains(extend=True) on the chains `res`, next to the plain result `aln`"""
    from bwtmi import _lib
    from smem_bench import _kern
    walls, ext = _walls(lambda: core.align_chains(reads, res, extend=True), reps)
    _lib.kernel_stats(ctx, enable=True, reset=True)
    core.align_chains(reads, res, extend=True)
    ks = _lib.kernel_stats(ctx, enable=False, reset=True)
    return dict(ext_band=32, match=1, mismatch=3, gap=3, xdrop=30,
                extend_wall_ms=min(walls), extend_wall_ms_repeats=walls, ext_rows=int(ext.ext_rows),
                extension_cells=int(ext.cells_total - aln.cells_total), cells_total=int(ext.cells_total),
                cigar_operations=int(ext.cigar.size), nm_total=int(ext.nm.sum()), columns_total=int(ext.cols.sum()),
                heads_extended=int((ext.head_score > 0).sum()), tails_extended=int((ext.tail_score > 0).sum()),
                whole_read_share_plain=whole_read_share(reads, res, aln),
                whole_read_share_extended=whole_read_share(reads, res, ext),
                extend_kernels_ms=round(sum(v[0] for k, v in ks.items() if k.startswith("k_extend")), 4),
                all_timed_ms=round(sum(v[0] for v in ks.values()), 4), kernels=_kern(ks),
                extend_sha256=extend_digest(ext))


def run(ctx, core, reads, long, reps, extend=False):
    from bwtmi import _lib
    from smem_bench import _kern
    mapper = lambda: core.map_batch(reads, min_len=19, both_strands=True, long=long)   # noqa: E731
    both = lambda: (lambda res: (res, core.align_chains(reads, res)))(mapper())        # noqa: E731
    map_walls, res = _walls(mapper, reps)
    both_walls, (res2, aln) = _walls(both, reps)
    align_walls, _ = _walls(lambda: core.align_chains(reads, res), reps)
    assert map_digest(res) == map_digest(res2)
    _lib.kernel_stats(ctx, enable=True, reset=True)
    core.align_chains(reads, res)
    ks = _lib.kernel_stats(ctx, enable=False, reset=True)
    kern_ms = sum(v[0] for k, v in ks.items() if k.startswith("k_align"))
    ngap = sum(aln.gaps)
    more = dict(extend=run_extend(ctx, core, reads, res, aln, reps)) if extend else {}
    return dict(reads=len(reads), read_bp=len(reads[0]), long_entry=long, min_len=19, both_strands=True, band=32,
                map_wall_ms=min(map_walls), map_wall_ms_repeats=map_walls,
                map_then_align_wall_ms=min(both_walls), map_then_align_wall_ms_repeats=both_walls,
                align_wall_ms=min(align_walls), align_wall_ms_repeats=align_walls,
                chains=int(res.strand.size), members=int(res.member_q.size), gaps=ngap,
                gaps_trivial=aln.gaps[0], gaps_small=aln.gaps[1], gaps_wave=aln.gaps[2],
                cells_total=int(aln.cells_total), cigar_operations=int(aln.cigar.size),
                nm_total=int(aln.nm.sum()), columns_total=int(aln.cols.sum()),
                align_kernels_ms=round(kern_ms, 4), align_upload_ms=round(ks.get("align_upload", (0.0,))[0], 4),
                align_all_timed_ms=round(sum(v[0] for v in ks.values()), 4), kernels=_kern(ks),
                map_sha256=map_digest(res), align_sha256=align_digest(aln), **more)


def workloads(seq, reads, long_reads, long_bp):
    from smem_bench import make_reads
    short = make_reads(seq, reads, 150, 3)
    long = make_reads(seq, long_reads, long_bp, long_bp // 100, seed=9100)
    return short, long


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--untouched", action="store_true")
    ap.add_argument("--extend", action="store_true")
    ap.add_argument("--tree", default=REPO)
    ap.add_argument("--bp", type=int, default=10_000_000)
    ap.add_argument("--reads", type=int, default=10_000)
    ap.add_argument("--long-reads", type=int, default=1000)
    ap.add_argument("--long-bp", type=int, default=10_000)
    a = ap.parse_args()
    sys.path[:0] = [os.path.join(os.path.abspath(a.tree), "bwt-algorithm_amd")]
    from bwtmi import BWTCore, _lib
    from smem_bench import _contig
    ctx = _lib.ctx(0)
    seq = _contig(a.bp)
    core = BWTCore(seq + b"$", build_kmer=False, reverse_index=True)
    short, long = workloads(seq, a.reads, a.long_reads, a.long_bp)
    if a.untouched:
        out = dict(tree=os.path.abspath(a.tree), lib=_lib.source_hash()[:12])
        for name, reads, lng, reps in (("short", short, False, 5), ("long", long, True, 3)):
            walls, res = _walls(lambda: core.map_batch(reads, min_len=19, both_strands=True, long=lng), reps)
            awalls, aln = _walls(lambda: core.align_chains(reads, res), reps)
            out[name] = dict(map_wall_ms=min(walls), map_wall_ms_repeats=walls, map_sha256=map_digest(res),
                             align_wall_ms=min(awalls), align_wall_ms_repeats=awalls, align_sha256=align_digest(aln))
        core.clear()
        print(json.dumps(out), flush=True)
        return
    if not a.out:
        ap.error("OUT.json is required")
    mid = a.long_bp // 2
    tract = [r[:mid] + r[mid + 75:] for r in long]
    runs = dict(bp=a.bp, short_reads=run(ctx, core, short, False, 5, a.extend),
                long_reads=run(ctx, core, long, True, 3, a.extend), tract_reads=run(ctx, core, tract, True, 3, a.extend))
    core.clear()
    print(json.dumps(runs), flush=True)
    with open(a.out, "w") as fh:
        json.dump(dict(host=_lib.host_info(), **runs), fh, indent=1)


if __name__ == "__main__":
    main()
