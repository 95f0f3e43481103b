"""`bwt-algorithm_amd/seeds.py --long`: a read past 1024 bp through the tool end
to end on a two-contig FASTA, against the brute-force SMEM oracle of
tests/test_gpu_smem.py; without --long the same read is refused."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_seeds_cli import PKG, _contigs, _expected_tsv


def test_long_flag_parses():
    from bwtmi import seeds
    a = seeds.build_parser().parse_args(["in.fa", "reads.txt", "--long", "-o", "o"])
    assert a.long is True and (a.min_len, a.both_strands, a.max_occ) == (19, False, 1024)
    assert seeds.build_parser().parse_args(["in.fa", "reads.txt", "-o", "o"]).long is False


@pytest.mark.gpu
def test_seeds_long_cli_end_to_end(gpu_ctx, tmp_path):
    from test_gpu_smem import _mutate, _random_dna, revcomp
    rng = np.random.default_rng(1500)
    a = _random_dna(rng, 4000)
    a[2600:3400] = _mutate(rng, a[300:1100], 5)                 # a near-copy inside contig 1
    b = _random_dna(rng, 2500)
    b[500:1400] = _mutate(rng, np.frombuffer(revcomp(a[200:1100].tobytes()), dtype=np.uint8), 4)   # and a '-' one in contig 2
    fasta = tmp_path / "two.fa"
    with open(fasta, "w") as fh:
        for name, seq in (("ctgA", a), ("ctgB", b)):
            s = seq.tobytes().decode()
            fh.write(f">{name} test\n" + "".join(s[i:i + 70] + "\n" for i in range(0, len(s), 70)))
    contigs = _contigs(str(fasta))
    assert [(n, len(s)) for n, s in contigs] == [("ctgA", 4000), ("ctgB", 2500)]
    read = _mutate(rng, a[100:1600], 6).tobytes().decode()      # 1,500 bp over the source of both copies
    reads = [("long", read), ("short", read[700:760])]
    qf = tmp_path / "reads.txt"
    qf.write_text("".join(f"{n}\t{s}\n" for n, s in reads))
    tool = os.path.join(PKG, "seeds.py")
    out = tmp_path / "seeds.tsv"
    r = subprocess.run([sys.executable, tool, str(fasta), str(qf), "--long", "--both-strands", "-o", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want = _expected_tsv(contigs, reads, 19, True, 1024)
    rows = [line.split("\t") for line in want.splitlines()]
    assert {(row[3], row[4]) for row in rows if row[0] == "long"} >= {("+", "ctgA"), ("-", "ctgB")}
    assert max(int(row[2]) - int(row[1]) for row in rows) > 150 and len(rows) > 8
    assert out.read_bytes() == want.encode()
    assert not os.path.exists(str(out) + ".tmp")
    # without --long: the 1024 bp limit, a failing exit, no file
    out2 = tmp_path / "refused.tsv"
    r = subprocess.run([sys.executable, tool, str(fasta), str(qf), "--both-strands", "-o", str(out2)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "1024" in r.stderr
    assert not out2.exists() and not os.path.exists(str(out2) + ".tmp")
