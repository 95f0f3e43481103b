"""The writers' pass from records to bytes (render.cpp): chunks of consecutive
records of one fold unit are walked for compounds as if the walk arrived at
their first index, ordered and formatted on their own, and a chunk the true
walk enters elsewhere is walked again from there.  BWTMI_RENDER_CHUNK sets the
records per chunk, so an edge can fall anywhere: between the two members of a
compound pair, inside a 3-mer split, ahead of a k-mer piece, inside a run of
equal starts.  Every case asserts the text equal, byte for byte, to the text
of one chunk and to the oracle's writers, in all five formats.
"""
import random

import pytest

import oracle
from oracle import post

FORMATS = ("strfinder", "bed", "vcf", "trf_table", "trf_dat")
CHUNKS = (1, 2, 3, 7, 0)       # 0: the default rule
ONE_CHUNK = 1 << 40
TRIM = 30


def crafted_contig():
    """Compound pairs, chains of three, 3-mer splits and k-mer pieces between
    stretches of random text."""
    r = random.Random(7)

    def background(n):
        return "".join(r.choice("ACGT") for _ in range(n))

    blocks = ("AC" * 8 + "GG" + "AG" * 8,
              "AC" * 8 + "T" + "AG" * 8 + "C" + "TC" * 8,
              "CAG" * 12 + "CAA" * 12,
              "CAG" * 12 + "T" + "GTT" * 5,
              ("ACACACACACAGAGAGAGAG" + "T") * 4,
              "A" * 9 + "AT" * 6)
    parts = []
    for _ in range(6):
        for b in blocks:
            parts.append(background(r.randint(40, 90)))
            parts.append(b)
    parts.append(background(200))
    return "".join(parts).encode()


def _job(contigs, threads):
    """contigs: (name, full, trim); hits from the oracle's strict scan."""
    from bwtmi.records import Job
    j = Job(min_copies=3, show_progress=True, threads=threads)
    for i, (name, seq, trim) in enumerate(contigs):
        j.add_contig(name, seq, trim, trim)
        j.add_hits(i, oracle.strict_scan(seq[trim:len(seq) - trim], 1, 1000, 0, 3))
    j.postprocess()
    return j


def _oracle_texts(contigs):
    seqs = {n: s[t:len(s) - t].decode() for n, s, t in contigs}
    full = {n: s.decode() for n, s, t in contigs}
    p = post.Pipeline(seqs, full, {n: t for n, s, t in contigs}, 3)
    recs = p.run([r for n, s in seqs.items()
                  for r in post.worker_records(n, s, oracle.strict_scan(s.encode(), 1, 1000, 0, 3))])
    return {fmt: post.render(p, recs, fmt).encode() for fmt in FORMATS}


def _same_at_every_chunk_size(jobs, want=None, chunks=CHUNKS):
    """jobs: {threads: job}.  Returns the one-chunk texts."""
    from bwtmi import _lib
    with _lib.knobs(RENDER_CHUNK=ONE_CHUNK):
        one = {fmt: next(iter(jobs.values())).render(fmt) for fmt in FORMATS}
    for fmt in FORMATS:
        if want is not None:
            assert one[fmt] == want[fmt], fmt
        for threads, j in jobs.items():
            for ch in chunks:
                with _lib.knobs(RENDER_CHUNK=ch):
                    assert j.render(fmt) == one[fmt], (fmt, threads, ch)
    return one


def test_crafted_contig_every_chunk_edge(built_lib, tmp_path):
    from bwtmi import _lib
    seq = crafted_contig()
    contigs = [("chr1", seq, TRIM)]
    jobs = {t: _job(contigs, t) for t in (1, 4)}
    one = _same_at_every_chunk_size(jobs, _oracle_texts(contigs))
    rows = one["strfinder"].decode().splitlines()[1:]
    compound = [r for r in rows if "]n+[" in r]
    # pairs, chains of three (a pair and a single), 3-mer splits and k-mer pieces are all there
    assert (len(seq), jobs[1].count(), len(rows), len(compound)) == (4437, 78, 61, 29)
    for motif in ("[AC]n+[AG]n", "[CAG]n+[CAA]n", "[CAG]n+[TGT]n", "[A]n+[AT]n", "[CT]n", "[TGT]n"):
        assert any(r.split("\t")[2] == motif for r in rows), motif
    # the file writers take the same pass (parts written behind the formatting)
    for ch in (1, 3):
        with _lib.knobs(RENDER_CHUNK=ch):
            for fmt in ("strfinder", "vcf"):
                out = tmp_path / f"o{ch}.{fmt}"
                jobs[4].write(fmt, str(out))
                assert out.read_bytes() == one[fmt], (fmt, ch)


def test_walk_again_is_reported(built_lib, capfd):
    """BWTMI_STATS=1: with one record per chunk every pair's second member is a
    chunk the walk steps over or enters late; with one chunk nothing is walked again."""
    import re
    from bwtmi import _lib
    j = _job([("chr1", crafted_contig(), TRIM)], 4)
    capfd.readouterr()
    with _lib.knobs(RENDER_CHUNK=1, STATS=1):
        j.render("strfinder")
    m = re.search(r"walked again from inside: (\d+) chunks, (\d+) rows", capfd.readouterr().err)
    assert m and int(m.group(1)) >= 20
    with _lib.knobs(RENDER_CHUNK=ONE_CHUNK, STATS=1):
        j.render("strfinder")
    assert "walked again from inside: 0 chunks, 0 rows" in capfd.readouterr().err


def _handmade(seq):
    """Records handed in: (start, end, motif, copies).  None carries an actual
    sequence, so the rows are built from the motifs."""
    recs = []

    def add(start, motif, copies, end=None):
        recs.append((start, end if end is not None else start + len(motif) * copies, motif, float(copies)))

    # equal starts with different ends, ends out of order, several runs in a row
    for s in (100, 140, 141):
        add(s, "AC", 9)
        add(s, "ACAC", 3)
        add(s, "A", 7)
        add(s, "ACACAC", 5)
    # a pairable couple, and a 12-base motif over 26 of its 32 bases (>= 80 %: no pair)
    add(300, "AC", 8)
    add(316, "AG", 8)
    add(290, "ACGTACGTACGG", 3, end=326)
    # the same with 25 of 32 bases (just under 80 %: a pair)
    add(500, "AC", 8)
    add(516, "AG", 8)
    add(490, "ACGTACGTACGG", 3, end=525)
    # couples and a chain of three, so that some edge falls between two members
    for k in range(7):
        s = 700 + 100 * k
        add(s, "TC", 6)
        add(s + 12 + (k % 5), "GA", 6)
        if k % 2:
            add(s + 30, "CT", 7)
    recs.sort(key=lambda r: r[0])
    return recs


def _as_records(recs, name, cls, **extra):
    return [cls(chrom=name, start=s, end=e, motif=m, copies=c, length=e - s, tier=2, confidence=0.9,
                n_copies_evaluated=int(c), percent_matches=97.0, score=40, **extra) for s, e, m, c in recs]


@pytest.mark.parametrize("order", ["by_start", "reversed"])
def test_handmade_records_equal_starts_and_long_motifs(built_lib, order):
    """Through set_records: runs of equal start on both sides of every edge, a
    long motif covering 80 % and just under 80 % of a couple, couples across an
    edge.  Reversed, the records are not one sorted run and the unit is one chunk."""
    from bwtmi.records import Job, TandemRepeat
    r = random.Random(11)
    seq = "".join(r.choice("ACGT") for _ in range(1600))
    recs = _handmade(seq)
    if order == "reversed":
        recs = recs[::-1]
    p = post.Pipeline({"c": seq[TRIM:-TRIM]}, {"c": seq}, {"c": TRIM}, 3)
    want = {fmt: post.render(p, _as_records(recs, "c", post.Rec), fmt).encode() for fmt in FORMATS}
    jobs = {}
    for t in (1, 4):
        j = Job(min_copies=3, show_progress=True, threads=t)
        j.add_contig("c", seq.encode(), TRIM, TRIM)
        j.set_records(_as_records(recs, "c", TandemRepeat), {"c": seq})
        jobs[t] = j
    one = _same_at_every_chunk_size(jobs, want)
    rows = one["strfinder"].decode().splitlines()[1:]
    assert not any(r.split("\t")[1] == "c:301-332" for r in rows)       # covered: two rows
    assert any(r.split("\t")[1] == "c:501-532" for r in rows)           # not covered: the pair
    bed = [tuple(map(int, ln.split("\t")[1:3])) for ln in one["bed"].decode().splitlines()[2:]]
    assert bed == sorted(bed) and len({s for s, e in bed}) < len(bed)


def test_imperfect_contig_and_a_unit_of_three_contigs(built_lib, tmp_path):
    """Records with variations and consensus motifs (2 % substitutions), and
    chr01 / CHR1 / chr1 in one fold unit with two trim offsets: their rows
    interleave, so that unit is one chunk whatever the switch says."""
    from bwtmi import synth
    from bwtmi.records import Job
    from test_fold_cuts import write_colliding_fasta
    contigs = [("c8", synth.generate_contig(200_000, 8, 0.02), TRIM)]
    jobs = {t: _job(contigs, t) for t in (1, 4)}
    one = _same_at_every_chunk_size(jobs, _oracle_texts(contigs))
    assert one["strfinder"].count(b"\n") > 500 and b";" in one["strfinder"]
    fa = str(tmp_path / "u.fa")
    write_colliding_fasta(fa)
    jobs = {}
    for t in (1, 4):
        j = Job(min_copies=3, show_progress=True, threads=t)
        j.load_fasta(fa, TRIM)
        for cid in range(j.contig_count()):
            _, fl, tl, tr = j.contig_info(cid)
            j.add_hits(cid, oracle.strict_scan(j.contig_seq(cid)[tl:fl - tr], 1, 1000, 0, 3))
        j.postprocess()
        jobs[t] = j
    _same_at_every_chunk_size(jobs, {fmt: post.run_file(fa, fmt).encode() for fmt in FORMATS})


@pytest.mark.gpu
def test_device_path_matches_host_path_at_every_chunk_size(gpu_ctx, tmp_path):
    """load -> scan -> postprocess -> write on the device, at three chunk sizes,
    against the host path over the oracle's hits."""
    from bwtmi import _lib, synth
    from bwtmi.records import Job
    for k, seq in enumerate((synth.generate_contig(200_000, 8, 0.02), crafted_contig())):
        host = _job([("c", seq, TRIM)], 4)
        with _lib.knobs(RENDER_CHUNK=ONE_CHUNK):
            want = {fmt: host.render(fmt) for fmt in ("strfinder", "trf_dat")}
        fa = str(tmp_path / f"d{k}.fa")
        with open(fa, "wb") as f:
            f.write(b">c\n" + b"\n".join(seq[i:i + 70] for i in range(0, len(seq), 70)) + b"\n")
        j = Job(min_copies=3, show_progress=True)
        j.load_fasta(fa, TRIM)
        j.scan(_lib.ctx())
        j.postprocess()
        for ch in (1, 5, 0):
            with _lib.knobs(RENDER_CHUNK=ch):
                for fmt, text in want.items():
                    out = tmp_path / f"d{k}_{ch}.{fmt}"
                    j.write(fmt, str(out))
                    assert out.read_bytes() == text, (k, ch, fmt)
