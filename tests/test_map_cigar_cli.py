"""`bwt-algorithm_amd/map.py --cigar`: the PAF rows with an alignment (no
device) and the new flags, and the tool end to end on the golden FASTA of two
contigs against rows built from BWTCore.map_batch plus BWTCore.align_chains."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bwt-algorithm_amd")


def _ops(text):
    """'45=6I44=' -> uint32 operations"""
    out, n = [], ""
    for ch in text:
        if ch.isdigit():
            n += ch
        else:
            out.append(int(n) << 4 | {"I": 1, "D": 2, "=": 7, "X": 8}[ch])
            n = ""
    return out


def _aln(cigars, nm, n_eq, qstart, qend, rstart, rend):
    from bwtmi.core import AlignResult
    ops = [_ops(c) for c in cigars]
    off = np.concatenate([[0], np.cumsum([len(o) for o in ops])]).astype(np.int64)
    return AlignResult(off, np.array([v for o in ops for v in o], np.uint32), np.array(nm, np.int32),
                       np.array(n_eq, np.int32), np.array(nm, np.int32) + np.array(n_eq, np.int32),
                       np.array(qstart, np.int32), np.array(qend, np.int32), np.array(rstart, np.int64),
                       np.array(rend, np.int64))


# ------------------------------------------------------------------ CPU
def test_map_rows_with_an_alignment():
    from bwtmi.map import map_rows
    # query 0 (100 bp): a '+' chain of two anchors with 6 bases more in the read, a '-' chain of two anchors
    # with 9 fewer whose span is narrower than the chain's; query 1: none; query 2 (30 bp): one anchor
    res = SimpleNamespace(
        offsets=np.array([0, 2, 2, 3]), strand=np.array([0, 1, 0], np.uint8), score=np.array([88, 55, 30], np.int32),
        n_anchors=np.array([2, 2, 1], np.int32), qstart=np.array([5, 10, 0], np.int32),
        qend=np.array([100, 80, 30], np.int32), rstart=np.array([1000, 195, 400]), rend=np.array([1089, 279, 430]),
        member_offsets=np.array([0, 2, 4, 5]), member_q=np.array([5, 56, 50, 10, 0], np.int32),
        member_r=np.array([1000, 1045, 200, 249, 400]), member_len=np.array([45, 44, 30, 30, 30], np.int32))
    aln = _aln(["45=6I44=", "30=9D10X30=", "30="], [6, 19, 0], [89, 60, 30], [5, 10, 0], [100, 80, 30],
               [1000, 200, 400], [1089, 279, 430])
    assert aln.cigar_string(1) == "30=9D10X30=" and len(aln) == 3 and aln.cols.tolist() == [95, 79, 30]
    rows = map_rows("chr1", 5000, ["r0", "r1", "r2"], [100, 77, 30], res, aln)
    assert rows == [
        "r0\t100\t5\t100\t+\tchr1\t5000\t1000\t1089\t89\t95\t255\ts1:i:88\tcm:i:2\tdl:i:6\tNM:i:6\tcg:Z:45=6I44=\n",
        "r0\t100\t10\t80\t-\tchr1\t5000\t200\t279\t60\t79\t255\ts1:i:55\tcm:i:2\tdl:i:-9\tNM:i:19\tcg:Z:30=9D10X30=\n",
        "r2\t30\t0\t30\t+\tchr1\t5000\t400\t430\t30\t30\t255\ts1:i:30\tcm:i:1\tdl:i:0\tNM:i:0\tcg:Z:30=\n"]
    # without the alignment (five arguments, or None) the rows are the chains' own
    plain = map_rows("chr1", 5000, ["r0", "r1", "r2"], [100, 77, 30], res)
    assert plain == map_rows("chr1", 5000, ["r0", "r1", "r2"], [100, 77, 30], res, None)
    assert plain[1] == "r0\t100\t10\t80\t-\tchr1\t5000\t195\t279\t60\t84\t255\ts1:i:55\tcm:i:2\tdl:i:-9\n"
    assert [r.split("\t")[:2] + r.split("\t")[4:7] + r.rstrip("\n").split("\t")[12:15] for r in plain] == \
        [r.split("\t")[:2] + r.split("\t")[4:7] + r.split("\t")[12:15] for r in rows]
    empty = SimpleNamespace(offsets=np.array([0, 0]), strand=np.zeros(0, np.uint8), score=np.zeros(0, np.int32),
                            n_anchors=np.zeros(0, np.int32), qstart=np.zeros(0, np.int32), qend=np.zeros(0, np.int32),
                            rstart=np.zeros(0, np.int64), rend=np.zeros(0, np.int64), member_offsets=np.array([0]),
                            member_q=np.zeros(0, np.int32), member_r=np.zeros(0, np.int64),
                            member_len=np.zeros(0, np.int32))
    assert map_rows("c", 10, ["r0"], [4], empty, _aln([], [], [], [], [], [], [])) == []


def test_map_parser_cigar_flags():
    from bwtmi import map as mapcli
    a = mapcli.build_parser().parse_args(["in.fa", "reads.txt", "-o", "out.paf"])
    assert (a.cigar, a.align_band) == (False, None)
    a = mapcli.build_parser().parse_args(["in.fa", "reads.txt", "--cigar", "-o", "o"])
    assert (a.cigar, a.align_band, a.min_len, a.max_occ) == (True, None, 19, 1024)
    a = mapcli.build_parser().parse_args(["in.fa", "reads.txt", "--cigar", "--align-band", "8", "--long", "-o", "o"])
    assert (a.cigar, a.align_band, a.long) == (True, 8, True)
    with pytest.raises(SystemExit):
        mapcli.build_parser().parse_args(["in.fa", "reads.txt", "--align-band", "x", "-o", "o"])


# ------------------------------------------------------------------ GPU
def _contigs(fasta):
    contigs = []
    with open(fasta) as f:
        for line in f:
            line = line.strip()
            if line.startswith(">"):
                contigs.append([line[1:].split()[0], ""])
            elif line:
                contigs[-1][1] += line.upper()
    return contigs


@pytest.mark.gpu
def test_map_cli_with_cigar(gpu_ctx, golden_dir, tmp_path):
    from bwtmi import BWTCore
    from bwtmi.map import map_rows
    fasta = os.path.join(golden_dir, "inputs", "synth_small.fa")
    contigs = _contigs(fasta)
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    seq = contigs[0][1]
    cut = seq[20:140]
    sub = cut[:30] + ("A" if cut[30] != "A" else "C") + cut[31:75] + ("G" if cut[75] != "G" else "T") + cut[76:]
    gone = cut[:50] + cut[58:]                                    # 8 bases missing from the read
    more = cut[:60] + "ACGTTGCA" + cut[60:]                       # 8 bases more in the read
    reads = [("cut", cut), ("sub", sub), ("rc", sub.encode().translate(comp)[::-1].decode()), ("gone", gone),
             ("more", more), ("tail", contigs[-1][1][-60:]), ("absent", "GATTACAGATTACAGATTACAGATTACA")]
    qf = tmp_path / "reads.txt"
    qf.write_text("".join(f"{n}\t{s}\n" for n, s in reads))
    tool = os.path.join(PKG, "map.py")
    args = ["-l", "12", "--both-strands", "--max-occ", "50", "--max-gap", "400", "--bandwidth", "60", "--min-score", "20"]
    names, seqs = [n for n, _ in reads], [s for _, s in reads]
    want = {None: [], 32: [], 2: []}
    for chrom, cseq in contigs:
        core = BWTCore(cseq.encode() + b"$", build_kmer=False)
        res = core.map_batch(seqs, 12, True, False, 50, None, max_gap=400, bandwidth=60, min_score=20)
        want[None] += map_rows(chrom, len(cseq), names, [len(s) for s in seqs], res)
        for band in (32, 2):
            aln = core.align_chains(seqs, res, band=band)
            want[band] += map_rows(chrom, len(cseq), names, [len(s) for s in seqs], res, aln)
    first = contigs[0][0]
    head = f"\t+\t{first}\t{len(seq)}\t20\t140\t"
    text = "".join(want[32])
    assert f"cut\t120\t0\t120{head}120\t120\t255\ts1:i:120\tcm:i:1\tdl:i:0\tNM:i:0\tcg:Z:120=\n" in text
    assert any(r.startswith(f"sub\t120\t0\t120{head}118\t120\t255\t") and r.endswith("\tNM:i:2\tcg:Z:30=1X44=1X44=\n")
               for r in want[32])
    assert any(r.startswith("rc\t120\t0\t120\t-\t") and r.endswith("\tNM:i:2\tcg:Z:30=1X44=1X44=\n") for r in want[32])
    gone_row = next(r for r in want[32] if r.startswith(f"gone\t112\t0\t112{head}112\t120\t255\t"))
    assert "\tdl:i:-8\tNM:i:8\tcg:Z:" in gone_row and "8D" in gone_row
    more_row = next(r for r in want[32] if r.startswith(f"more\t128\t0\t128{head}120\t128\t255\t"))
    assert "\tdl:i:8\tNM:i:8\tcg:Z:" in more_row and "8I" in more_row
    assert all(len(r.split("\t")) == 17 for r in want[32]) and len(want[32]) == len(want[None])
    for flags, rows in ((["--cigar"], want[32]), (["--cigar", "--align-band", "2"], want[2]), ([], want[None])):
        out = tmp_path / "map.paf"
        r = subprocess.run([sys.executable, tool, fasta, str(qf), *args, *flags, "-o", str(out)], capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert out.read_bytes() == "".join(rows).encode(), flags
    # a band the library refuses: its message, a failing exit, no file
    out2 = tmp_path / "bad.paf"
    r = subprocess.run([sys.executable, tool, fasta, str(qf), *args, "--cigar", "--align-band", "2000", "-o", str(out2)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "band" in r.stderr and not out2.exists() and not os.path.exists(str(out2) + ".tmp")
