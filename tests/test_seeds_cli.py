"""`bwt-algorithm_amd/seeds.py`: the row formatter and the argument parser (no
device), and the tool end to end on the golden synthetic FASTA against the
brute-force SMEM oracle of tests/test_gpu_smem.py, one index per contig."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bwt-algorithm_amd")


# ------------------------------------------------------------------ CPU
def test_smem_rows_format_and_order():
    from bwtmi.seeds import smem_rows
    # query 0: [2,30)+ at 7 and 90, [10,40)- too frequent; query 1: none; query 2: [0,12)+ at 0
    res = SimpleNamespace(offsets=np.array([0, 2, 2, 3]), qstart=np.array([2, 10, 0], np.int32),
                          qend=np.array([30, 40, 12], np.int32), strand=np.array([0, 1, 0], np.uint8),
                          count=np.array([2, 5000, 1]), pos_offsets=np.array([0, 2, 2, 3]),
                          positions=np.array([7, 90, 0]))
    assert smem_rows("chr1", ["r0", "r1", "r2"], res, 1024) == ["r0\t2\t30\t+\tchr1\t2\t7,90\n",
                                                               "r0\t10\t40\t-\tchr1\t5000\t*\n",
                                                               "r2\t0\t12\t+\tchr1\t1\t0\n"]
    empty = SimpleNamespace(offsets=np.array([0, 0]), qstart=np.zeros(0, np.int32), qend=np.zeros(0, np.int32),
                            strand=np.zeros(0, np.uint8), count=np.zeros(0, np.int64), pos_offsets=np.array([0]),
                            positions=np.zeros(0, np.int64))
    assert smem_rows("c", ["r0"], empty, 1024) == []


def test_seeds_parser():
    from bwtmi import locate, seeds
    assert seeds.parse_patterns is locate.parse_patterns          # the one pattern-file parser
    a = seeds.build_parser().parse_args(["in.fa", "reads.txt", "-o", "out.tsv"])
    assert (a.reference, a.queries, a.output) == ("in.fa", "reads.txt", "out.tsv")
    assert (a.min_len, a.both_strands, a.max_occ, a.max_positions) == (19, False, 1024, None)
    a = seeds.build_parser().parse_args(["in.fa", "reads.txt", "-l", "12", "--both-strands", "--max-occ", "3",
                                         "--max-positions", "99", "-o", "o"])
    assert (a.min_len, a.both_strands, a.max_occ, a.max_positions) == (12, True, 3, 99)
    with pytest.raises(SystemExit):
        seeds.build_parser().parse_args(["in.fa", "reads.txt"])   # no output


def test_seeds_reports_unreadable_input(tmp_path, capsys):
    from bwtmi import seeds
    out = tmp_path / "o.tsv"
    assert seeds.main([str(tmp_path / "none.fa"), str(tmp_path / "none.txt"), "-o", str(out)]) == 1
    assert "seeds:" in capsys.readouterr().err and not out.exists() and not os.path.exists(str(out) + ".tmp")
    bad = tmp_path / "bad.txt"
    bad.write_text("a\tACGT\textra\n")
    assert seeds.main([str(tmp_path / "none.fa"), str(bad), "-o", str(out)]) == 1
    assert "pattern line 1" in capsys.readouterr().err


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


def _expected_tsv(contigs, reads, min_len, both, max_occ):
    from test_gpu_smem import Oracle
    rows = []
    for chrom, seq in contigs:
        orc = Oracle(seq.encode() + b"$")
        for name, read in reads:
            for s, e, strand, occ in orc.query(read.encode(), min_len, both)[0]:
                where = "*" if len(occ) > max_occ else ",".join(map(str, occ))
                rows.append(f"{name}\t{s}\t{e}\t{'-' if strand else '+'}\t{chrom}\t{len(occ)}\t{where}\n")
    return "".join(rows)


@pytest.mark.gpu
def test_seeds_cli_end_to_end(gpu_ctx, golden_dir, tmp_path):
    fasta = os.path.join(golden_dir, "inputs", "synthetic_test.fa")
    contigs = _contigs(fasta)
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    seq = contigs[0][1]
    cut = seq[20:80]
    sub = cut[:20] + ("A" if cut[20] != "A" else "C") + cut[21:45] + ("G" if cut[45] != "G" else "T") + cut[46:]
    last = contigs[-1][1]
    reads = [("cut", cut), ("sub", sub), ("rc", sub.encode().translate(comp)[::-1].decode()),
             ("ca-run", "CACACACA"), ("ATGCATGCATGCATGC", "ATGCATGCATGCATGC"), ("agc", "TAGCAGCT"),
             ("tail", last[-30:]), ("gap", "GTCNNNNTTNNNNNNNNNNNN"), ("absent", "GATTACAGATTACAGATTACAGATTACA"),
             ("short", "ACGTAC")]
    qf = tmp_path / "reads.txt"
    qf.write_text("# reads\n\n" + "".join((f"{s.lower()}\n" if n == s else f"{n}\t{s}\n") for n, s in reads))
    tool = os.path.join(PKG, "seeds.py")
    out = tmp_path / "seeds.tsv"
    r = subprocess.run([sys.executable, tool, fasta, str(qf), "-l", "4", "--both-strands", "--max-occ", "3",
                        "-o", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want = _expected_tsv(contigs, reads, 4, True, 3)
    assert want.count("\n") > 10 and "\t-\t" in want and "\t*\n" in want and "cut\t0\t60\t+\t" in want
    assert any(line.split("\t")[5] not in ("0", "1") and not line.endswith("*\n") for line in want.splitlines(True))
    assert out.read_bytes() == want.encode()
    assert not os.path.exists(str(out) + ".tmp")
    # a tripped cap: the library's message, a failing exit, no file
    out2 = tmp_path / "capped.tsv"
    r = subprocess.run([sys.executable, tool, fasta, str(qf), "-l", "4", "--max-positions", "1", "-o", str(out2)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "positions" in r.stderr and "max_positions = 1" in r.stderr
    assert not out2.exists() and not os.path.exists(str(out2) + ".tmp")
