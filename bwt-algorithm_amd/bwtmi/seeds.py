"""`seeds.py` command line: the super-maximal exact matches (SMEMs) of reads
against a genome, with where they occur -- the seeds a read mapper, an STR
genotyper or a contamination screen starts from.

    python seeds.py IN.fa QUERIES [-l MIN_LEN] [--both-strands] [--long] [--max-occ N] [--max-positions N] -o OUT.tsv

QUERIES is in the pattern-file format of `locate.py` (`SEQ` or `NAME<TAB>SEQ`
per line).  One FM index per contig (seq + '$', built on the device, released
before the next), one BWTCore.smem_batch per contig; one row per SMEM per
contig, `query qstart qend strand chrom count positions`, ordered by contig,
then query order in the file, then (strand, qstart).  `positions` is
comma-joined, or `*` when count > max-occ.  Maximality is per contig: each
contig has its own index, so a match that could be extended on another contig
is still reported on the one where it cannot.  Queries are at most 1024 bp;
with `--long`, 1,048,576 bp: each contig's index is then built with its reverse
index (about twice the build time) and searched by BWTCore.smem_long_batch,
with the same rows in the same order.  Not in the reference: `bwt.py` stays
the drop-in, this tool stands next to it.
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import List, Optional

from .locate import parse_patterns


def smem_rows(chrom: str, names: List[str], res, max_occ: int) -> List[str]:
    """TSV rows of one contig's SMEMs (`res`: the arrays of a SmemResult), in
    the result's order: query order, then (strand, qstart)."""
    off = [int(v) for v in res.offsets]
    po = [int(v) for v in res.pos_offsets]
    pos = [int(v) for v in res.positions]
    rows = []
    for q in range(len(off) - 1):
        for i in range(off[q], off[q + 1]):
            cnt = int(res.count[i])
            where = "*" if cnt > max_occ else ",".join(str(p) for p in pos[po[i]:po[i + 1]])
            rows.append(f"{names[q]}\t{int(res.qstart[i])}\t{int(res.qend[i])}\t{'-' if int(res.strand[i]) else '+'}\t"
                        f"{chrom}\t{cnt}\t{where}\n")
    return rows


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(
        description="Super-maximal exact matches of reads against a genome (MI355X-native FM index)")
    p.add_argument("reference", help="Reference genome FASTA file")
    p.add_argument("queries", help="Query file: one SEQ or NAME<TAB>SEQ per line ('#' comments), up to 1024 bp each "
                                   "(1,048,576 with --long)")
    p.add_argument("-l", "--min-len", type=int, default=19, help="Shortest SMEM reported (default: 19)")
    p.add_argument("--both-strands", action="store_true", help="Also search the reverse complement")
    p.add_argument("--long", action="store_true",
                   help="Long reads: build each contig's reverse index too and lift the 1024 bp limit to 1,048,576 bp")
    p.add_argument("--max-occ", type=int, default=1024,
                   help="List the positions of an SMEM with at most this many occurrences, else '*' (default: 1024)")
    p.add_argument("--max-positions", type=int, default=None,
                   help="Fail a contig's search above this many listed positions (default: 2^27)")
    p.add_argument("-o", "--output", required=True, help="Output TSV file")
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
        job = Job()
        job.load_fasta(a.reference, 0)
        with open(tmp, "w") as out:
            for cid in range(job.contig_count()):
                chrom = job.contig_info(cid)[0]
                core = BWTCore(job.contig_seq(cid) + b"$", build_kmer=False, reverse_index=a.long)
                try:
                    search = core.smem_long_batch if a.long else core.smem_batch
                    res = search(seqs, a.min_len, a.both_strands, a.max_occ, a.max_positions)
                finally:
                    core.clear()
                out.writelines(smem_rows(chrom, names, res, a.max_occ))
        os.replace(tmp, a.output)
    except (ValueError, RuntimeError, OSError) as e:   # a bad query, a tripped cap, an unreadable file
        if os.path.exists(tmp):
            os.remove(tmp)
        print(f"seeds: {e}", file=sys.stderr)
        return 1
    return 0
