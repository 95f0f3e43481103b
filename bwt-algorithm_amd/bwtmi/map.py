"""`map.py` command line: where reads lie in a genome, and how much longer or
shorter they are there -- the SMEM seeds of `seeds.py` chained on the device,
one PAF row per chain.

    python map.py IN.fa QUERIES [-l MIN_LEN] [--both-strands] [--long] [--max-occ N] [--max-gap N]
                  [--bandwidth N] [--min-score N] [--min-anchors N] [--cigar [--align-band N]]
                  [--extend [--xdrop N] [--ext-band N]]
                  [--select [--mask-level PCT] [--pri-ratio PCT] [--best-n N] [--mapq-full F]] -o OUT.paf

QUERIES is in the pattern-file format of `locate.py` (`SEQ` or `NAME<TAB>SEQ`
per line).  One FM index per contig (seq + '$', built on the device, released
before the next; with `--long` also its reverse index, for reads up to
1,048,576 bp instead of 1024), one BWTCore.map_batch per contig.  Rows are
ordered by contig, then query order in the file, then the result's order
(strand, then the chainer's: best chain first).  The 12 PAF columns are
`qname qlen qstart qend strand tname tlen tstart tend nmatch alen 255`: tlen is
the contig's length without the '$', nmatch = len_0 + the sum of min(len_i, dq,
dr) along the chain (the bases its anchors cover, overlaps counted once), alen
= max(qend - qstart, tend - tstart).  Tags: `s1:i:` the chain's score, `cm:i:`
its anchors, `dl:i:` = (last qe - first qe) - (last re - first re) over the
chain's anchors in the searched string's coordinates: positive when the read
is longer than the reference there -- through both flanks of a tandem repeat,
the tract's length difference.  Chains are per contig: each contig has its own
index.  With `--cigar` every chain is also aligned base by base on the device
(BWTCore.align_chains: a banded DP per gap between anchors, `--align-band` its
W, default 32): columns 3, 4, 8 and 9 become the aligned span (first anchor to
last), column 10 the bases in `=`, column 11 the alignment's columns, and the
row gains `NM:i:` and `cg:Z:` (with `=` and `X`; on strand `-` in the reverse
complement's order) after `dl:i:`.  With `--extend` (implies `--cigar`) every
alignment is also extended past its outer anchors towards the read's ends, a
scored banded DP with X-drop (`--xdrop`, default 30; `--ext-band`, default 32):
the same columns and tags, with the extended span, matches, columns, `NM:i:`
and `cg:Z:`.  With `--select` (implied by any of its four options) the chains
of a read over all contigs and both strands are judged together on the device
(bwtmi.select_chains; include/bwtmi.h, bwtmi_select_chains, states the rule): a
chain that overlaps a better chain of the read by `--mask-level` percent
(default 50) of the shorter of the two is secondary to it, the others are
primary; a secondary is written when its score reaches `--pri-ratio` percent
(default 80) of its primary's, `--best-n` (default 5) per read at most.  Column
12 becomes the mapping quality, 0..60 for a primary (60 when no secondary
competes and its score reaches `--mapq-full`, default 100) and 0 for a
secondary, and the row gains `tp:A:P` or `tp:A:S` after `dl:i:`.  Every contig
is mapped first; the selection runs once; then `--cigar` / `--extend` align
the kept chains only (a FASTA of one contig keeps its index meanwhile; with
more, the index of a contig with a kept chain is built again).  Not in the
reference: `bwt.py` stays the drop-in, this tool stands next to it.
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import List, Optional, Sequence

from .locate import parse_patterns


def map_rows(chrom: str, tlen: int, names: Sequence[str], qlens: Sequence[int], res, aln=None, sel=None) -> List[str]:
    """PAF rows of one contig's chains (`res`: the arrays of a MapResult), in
    the result's order: query order, then strand, then the chainer's order.
    `aln` (the AlignResult of the same chains): the rows carry the alignment's
    span, matches, columns, NM:i: and cg:Z: (the module's text says how).
    `sel` (the Selection of the same chains): column 12 is the chain's mapq and
    tp:A:P or tp:A:S follows dl:i:."""
    off = [int(v) for v in res.offsets]
    mo = [int(v) for v in res.member_offsets]
    rows = []
    for q in range(len(off) - 1):
        m = int(qlens[q])
        for k in range(off[q], off[q + 1]):
            rev = bool(int(res.strand[k]))
            a, b = mo[k], mo[k + 1]
            ln = [int(v) for v in res.member_len[a:b]]
            # ends in the searched string's coordinates (revcomp(Q) on strand '-')
            qe = [(m - int(v)) if rev else int(v) + l for v, l in zip(res.member_q[a:b], ln)]
            re = [int(v) + l for v, l in zip(res.member_r[a:b], ln)]
            nmatch = ln[0] + sum(min(ln[i], qe[i] - qe[i - 1], re[i] - re[i - 1]) for i in range(1, b - a))
            dl = (qe[-1] - qe[0]) - (re[-1] - re[0])
            tags = f"s1:i:{int(res.score[k])}\tcm:i:{int(res.n_anchors[k])}\tdl:i:{dl}"
            mapq = 255
            if sel is not None:
                mapq = int(sel.mapq[k])
                tags += f"\ttp:A:{'P' if sel.primary[k] else 'S'}"
            if aln is None:
                qs, qend, ts, te = int(res.qstart[k]), int(res.qend[k]), int(res.rstart[k]), int(res.rend[k])
                alen = max(qend - qs, te - ts)
            else:
                qs, qend, ts, te = int(aln.qstart[k]), int(aln.qend[k]), int(aln.rstart[k]), int(aln.rend[k])
                nmatch, alen = int(aln.n_eq[k]), int(aln.cols[k])
                tags += f"\tNM:i:{int(aln.nm[k])}\tcg:Z:{aln.cigar_string(k)}"
            rows.append(f"{names[q]}\t{m}\t{qs}\t{qend}\t{'-' if rev else '+'}\t{chrom}\t{tlen}\t{ts}\t{te}\t{nmatch}\t"
                        f"{alen}\t{mapq}\t{tags}\n")
    return rows


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Map reads to a genome: chained SMEM seeds as PAF (MI355X-native FM index)")
    p.add_argument("reference", help="Reference genome FASTA file")
    p.add_argument("queries", help="Query file: one SEQ or NAME<TAB>SEQ per line ('#' comments), up to 1024 bp each "
                                   "(1,048,576 with --long)")
    p.add_argument("-l", "--min-len", type=int, default=19, help="Shortest SMEM used as a seed (default: 19)")
    p.add_argument("--both-strands", action="store_true", help="Also map the reverse complement")
    p.add_argument("--long", action="store_true",
                   help="Long reads: build each contig's reverse index too and lift the 1024 bp limit to 1,048,576 bp")
    p.add_argument("--max-occ", type=int, default=1024,
                   help="Seeds with more occurrences than this give no anchors (default: 1024)")
    p.add_argument("--max-gap", type=int, default=None, help="Longest gap between chained anchors (default: 5000)")
    p.add_argument("--bandwidth", type=int, default=None,
                   help="Largest difference between the query and reference gaps (default: 500)")
    p.add_argument("--min-score", type=int, default=None, help="Lowest chain score reported (default: 40)")
    p.add_argument("--min-anchors", type=int, default=None, help="Fewest anchors of a reported chain (default: 1)")
    p.add_argument("--cigar", action="store_true",
                   help="Align every chain base by base on the device: aligned span, matches, columns, NM:i: and cg:Z:")
    p.add_argument("--align-band", type=int, default=None,
                   help="With --cigar: the band W of the DP between anchors (default: 32, at most 1024)")
    p.add_argument("--extend", action="store_true",
                   help="Extend every alignment past its outer anchors towards the read's ends (implies --cigar)")
    p.add_argument("--xdrop", type=int, default=None,
                   help="With --extend: stop once a row's best score lies this far below the best (default: 30)")
    p.add_argument("--ext-band", type=int, default=None,
                   help="With --extend: the band of the extension DP (default: 32, at most 1024)")
    p.add_argument("--select", action="store_true",
                   help="Judge each read's chains over all contigs together: primary / secondary (tp:A:), mapping quality "
                        "in column 12, weak secondaries dropped")
    p.add_argument("--mask-level", type=int, default=None,
                   help="With --select: a chain overlapping a better one by this percentage of the shorter is secondary "
                        "(default: 50)")
    p.add_argument("--pri-ratio", type=int, default=None,
                   help="With --select: a secondary is written when its score reaches this percentage of its primary's "
                        "(default: 80)")
    p.add_argument("--best-n", type=int, default=None,
                   help="With --select: at most this many secondaries per read (default: 5; 0: primaries only)")
    p.add_argument("--mapq-full", type=int, default=None,
                   help="With --select: the score at which a primary without a competitor earns mapping quality 60 "
                        "(default: 100)")
    p.add_argument("-o", "--output", required=True, help="Output PAF file")
    return p


def main(argv: Optional[List[str]] = None) -> int:
    a = build_parser().parse_args(argv)
    tmp = a.output + ".tmp"
    try:
        with open(a.queries) as fh:
            pats = parse_patterns(fh)
        from .core import BWTCore
        from .records import Job
        names, seqs = [n for n, _ in pats], [s for _, s in pats]
        qlens = [len(s.encode("utf-8")) for s in seqs]
        job = Job()
        job.load_fasta(a.reference, 0)
        params = dict(mask=a.mask_level, pri_ratio=a.pri_ratio, best_n=a.best_n, full=a.mapq_full)
        select = a.select or any(v is not None for v in params.values())

        def index(seq):
            return BWTCore(seq + b"$", build_kmer=False, reverse_index=a.long)

        def chains(core):
            return core.map_batch(seqs, a.min_len, a.both_strands, a.long, a.max_occ, None, max_gap=a.max_gap,
                                  bandwidth=a.bandwidth, min_score=a.min_score, min_anchors=a.min_anchors)

        def align(core, res):
            if a.extend:
                return core.align_chains(seqs, res, band=a.align_band, extend=True, ext_band=a.ext_band, xdrop=a.xdrop)
            return core.align_chains(seqs, res, band=a.align_band) if a.cigar else None

        ncontig = job.contig_count()
        with open(tmp, "w") as out:
            if not select:
                for cid in range(ncontig):
                    chrom = job.contig_info(cid)[0]
                    seq = job.contig_seq(cid)
                    core = index(seq)
                    try:
                        res = chains(core)
                        aln = align(core, res)
                    finally:
                        core.clear()
                    out.writelines(map_rows(chrom, len(seq), names, qlens, res, aln))
            else:
                from .select import select_chains
                kept_core = None   # a FASTA of one contig keeps its index between the passes
                try:
                    results = []
                    for cid in range(ncontig):       # pass 1: every contig's chains, held on the host
                        core = index(job.contig_seq(cid))
                        try:
                            results.append(chains(core))
                        finally:
                            if ncontig == 1:
                                kept_core = core
                            else:
                                core.clear()
                    sels = select_chains(results, **params) if results else []
                    for cid in range(ncontig):       # pass 2: the kept chains, aligned when asked for
                        chrom = job.contig_info(cid)[0]
                        seq = job.contig_seq(cid)
                        keep = sels[cid].keep
                        res, sel, aln = results[cid].take(keep), sels[cid].take(keep), None
                        if (a.cigar or a.extend) and res.strand.size:
                            core = kept_core if kept_core is not None else index(seq)
                            try:
                                aln = align(core, res)
                            finally:
                                if kept_core is None:
                                    core.clear()
                        out.writelines(map_rows(chrom, len(seq), names, qlens, res, aln, sel))
                finally:
                    if kept_core is not None:
                        kept_core.clear()
        os.replace(tmp, a.output)
    except (ValueError, RuntimeError, OSError) as e:   # a bad query or parameter, a tripped cap, an unreadable file
        if os.path.exists(tmp):
            os.remove(tmp)
        print(f"map: {e}", file=sys.stderr)
        return 1
    return 0
