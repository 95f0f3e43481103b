"""`locate.py` command line: where on a genome do these flanks, primers or
motifs occur, allowing a few substitutions, on either strand.

    python locate.py IN.fa PATTERNS [-k K] [--both-strands] [--max-candidates N] -o OUT.bed

One FM index per contig (seq + '$', built on the device, released before the
next), one BWTCore.locate_batch per contig; BED6 rows
`chrom start end name mismatches strand`.  Not in the reference: `bwt.py`
stays the drop-in, this tool stands next to it.
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import Iterable, List, Optional, Tuple

import numpy as np


def parse_patterns(lines: Iterable[str]) -> List[Tuple[str, str]]:
    """(name, sequence) of every pattern line: `SEQ` or `NAME<TAB>SEQ`; '#'
    lines and blank lines are skipped, sequences upper-cased (the loader
    upper-cases the genome), the name defaults to the sequence."""
    out = []
    for no, line in enumerate(lines, 1):
        line = line.rstrip("\r\n")
        if not line.strip() or line.lstrip().startswith("#"):
            continue
        cols = line.split("\t")
        if len(cols) == 1:
            seq = cols[0].strip().upper()
            name = seq
        elif len(cols) == 2:
            name, seq = cols[0].strip(), cols[1].strip().upper()
        else:
            raise ValueError(f"pattern line {no}: expected SEQ or NAME<TAB>SEQ, got {len(cols)} columns")
        if not name or not seq or any(ch.isspace() for ch in seq):
            raise ValueError(f"pattern line {no}: empty name or sequence, or white space inside the sequence")
        out.append((name, seq))
    return out


def bed_rows(chrom: str, names: List[str], lengths: List[int], offsets, positions, mismatches, strand) -> List[str]:
    """BED6 rows of one contig's hits (the arrays of a LocateResult): by start,
    then pattern order in the file, then '+' before '-'."""
    offsets = np.asarray(offsets, dtype=np.int64)
    pos = np.asarray(positions, dtype=np.int64)
    pid = np.repeat(np.arange(offsets.size - 1, dtype=np.int64), np.diff(offsets))
    st = np.asarray(strand, dtype=np.int64)
    order = np.lexsort((st, pid, pos))
    mm = np.asarray(mismatches, dtype=np.int64)
    return [f"{chrom}\t{pos[i]}\t{pos[i] + lengths[pid[i]]}\t{names[pid[i]]}\t{mm[i]}\t{'-' if st[i] else '+'}\n"
            for i in order.tolist()]


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(
        description="Locate patterns on a genome with up to 3 substitutions (MI355X-native FM index)")
    p.add_argument("reference", help="Reference genome FASTA file")
    p.add_argument("patterns", help="Pattern file: one SEQ or NAME<TAB>SEQ per line ('#' comments)")
    p.add_argument("-k", "--max-mismatches", type=int, default=0, help="Substitutions allowed, 0..3 (default: 0)")
    p.add_argument("--both-strands", action="store_true", help="Also search the reverse complement")
    p.add_argument("--max-candidates", type=int, default=None,
                   help="Fail a contig's search above this many seed occurrences (default: 2^27)")
    p.add_argument("-o", "--output", required=True, help="Output BED6 file")
    return p


def main(argv: Optional[List[str]] = None) -> int:
    a = build_parser().parse_args(argv)
    tmp = a.output + ".tmp"
    try:
        with open(a.patterns) as fh:
            pats = parse_patterns(fh)
        from .core import BWTCore
        from .records import Job
        names, seqs = [n for n, _ in pats], [s for _, s in pats]
        lengths = [len(s.encode("utf-8")) for s in seqs]
        job = Job()
        job.load_fasta(a.reference, 0)
        with open(tmp, "w") as out:
            for cid in range(job.contig_count()):
                chrom = job.contig_info(cid)[0]
                core = BWTCore(job.contig_seq(cid) + b"$", build_kmer=False)
                try:
                    res = core.locate_batch(seqs, a.max_mismatches, a.both_strands, a.max_candidates)
                finally:
                    core.clear()
                out.writelines(bed_rows(chrom, names, lengths, res.offsets, res.positions, res.mismatches,
                                        res.strand))
        os.replace(tmp, a.output)
    except (ValueError, RuntimeError, OSError) as e:   # a bad pattern, a tripped cap, an unreadable file
        if os.path.exists(tmp):
            os.remove(tmp)
        print(f"locate: {e}", file=sys.stderr)
        return 1
    return 0
