"""The fold, refine, collapse and filter in one pass over cut segments (CPU).

Every fold unit takes post.cpp's fold_cuts.  A unit of one contig whose input
records are all strict hits is folded segment by segment between verified cuts
(BWTMI_FOLD_CUTS=1, the default); with BWTMI_FOLD_CUTS=0 no cut is used and the
unit is one segment, the reference's serial fold -- which is also what a unit
of several contigs gets whatever the switch.  Every case asserts that the
rendered text is the same, byte for byte.  BWTMI_FOLD_CHUNK sets the records
per task: at 1, 2 and 8 cuts and task edges fall everywhere and some tasks own
nothing.
"""
import ctypes
import json
import os

import pytest

import oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CHUNKS = (1, 2, 8, 64, 0)      # 0: the default rule


def _render(seq, hits, min_copies, threads, trim=30):
    from bwtmi.records import Job
    j = Job(min_copies=min_copies, show_progress=True, threads=threads)
    j.add_contig("chr1", seq, trim, trim)
    j.add_hits(0, hits)
    j.postprocess()
    return j.render("strfinder")


def _hits(seq, min_copies, trim=30):
    return oracle.strict_scan(seq[trim:len(seq) - trim], 1, 1000, 0, min_copies)


def _same_on_both_paths(seq, min_copies=3, threads=(4,), chunks=CHUNKS, trim=30):
    from bwtmi import _lib
    hits = _hits(seq, min_copies, trim)
    with _lib.knobs(FOLD_CUTS=0):
        want = _render(seq, hits, min_copies, 4, trim)
    for t in threads:
        for ch in chunks:
            with _lib.knobs(FOLD_CUTS=1, FOLD_CHUNK=ch):
                got = _render(seq, hits, min_copies, t, trim)
            assert got == want, (min_copies, t, ch)
    return want, len(hits)


@pytest.mark.parametrize("rate", [0.0, 0.02])
@pytest.mark.parametrize("min_copies", [1, 2, 3, 4, 7])
def test_synthetic_contigs_every_min_copies(built_lib, min_copies, rate):
    from bwtmi import synth
    seq = synth.generate_contig(60_000 + 20_000 * min_copies, 40 + min_copies, rate)
    want, n = _same_on_both_paths(seq, min_copies, threads=(1, 2, 8))
    assert n > 100 and want.count(b"\n") > 10


def test_gap_profile_contig(built_lib):
    """Assembly gaps (N runs, IUPAC codes): long chains of one-base merges."""
    from bwtmi import synth
    seq = synth.generate_contig(200_000, 3, 0.0, gaps="n2")
    assert seq.count(b"N") > 100
    _same_on_both_paths(seq, 3, threads=(1, 8))


def test_the_pass_reports_its_stages_and_verifies_its_cuts(built_lib, capfd):
    """BWTMI_STATS=1: the stage line (it names merge and collapse)
    counts hits, verified cuts and the bits that did not verify.  A cut is used
    only after it is verified on the records themselves, so a bit that the reach
    bound gets wrong changes nothing: with 2 % substitutions some bits do fail
    (the walk's last copy may end past its limit) and the text is still the same."""
    import re
    from bwtmi import _lib, synth
    seq = synth.generate_contig(200_000, 8, 0.02)
    hits = _hits(seq, 3)
    capfd.readouterr()
    with _lib.knobs(FOLD_CUTS=1, STATS=1):
        got = _render(seq, hits, 3, 4)
    err = capfd.readouterr().err
    assert "merge" in err and "collapse" in err and "one pass" in err, err[-600:]
    m = re.search(r"(\d+) hits, (\d+) cuts \((\d+) bits unverified", err)
    assert m and 1000 < int(m.group(1)) <= len(hits), err[-600:]     # (the host screen ran first)
    assert int(m.group(2)) > int(m.group(1)) // 10 and 1 <= int(m.group(3)) < 10, err[-600:]
    with _lib.knobs(FOLD_CUTS=0, STATS=1):
        want = _render(seq, hits, 3, 4)
    err = capfd.readouterr().err
    assert "one pass" in err and "repair" not in err, err[-600:]
    assert "hits, 1 cuts (0 bits unverified, 0 tasks folded again)" in err, err[-600:]
    assert got == want
    # every task edge on an unverified bit's neighbourhood: chunks of 1 record
    with _lib.knobs(FOLD_CUTS=1, FOLD_CHUNK=1, STATS=1):
        assert _render(seq, hits, 3, 4) == want
    m = re.search(r"(\d+) tasks folded again", capfd.readouterr().err)
    assert m and int(m.group(1)) >= 1


def _pad(core, seed=0):
    """core between two stretches without tandem repeats (a de Bruijn-like walk)."""
    import numpy as np
    r = np.random.default_rng(100 + seed)
    flank = bytes(r.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 400))
    return flank + core + flank[::-1]


CRAFTED = {
    # the short run absorbs the long one
    "short_run_absorbs_long": b"AAAGAAAAAAAA",
    "two_runs_touching": b"AAATTTT",
    # a one-base run overlapped by a dinucleotide array
    "run_under_dinucleotide": b"AAACACACACACAC",
    # two arrays with a shared start: (AC)n is also (ACAC)n's unit, and a longer unit array starts with it
    "shared_start": b"ACGACGACGACGACGACGTTACGACGTTACGACGTTACGACGTT",
    # a record that ends exactly M + 1 before the next start (no cut), and one M + 2 before it (a cut)
    "gap_m_plus_1": b"CAGCAGCAGCAGCAG" + b"TGAT" + b"CAGCAGCAGCAGCAG",
    "gap_m_plus_2": b"CAGCAGCAGCAGCAG" + b"TGATC" + b"CAGCAGCAGCAGCAG",
    "gap_1_plus_1": b"AAAAAAAA" + b"CG" + b"AAAAAAAA",
    "gap_1_plus_2": b"AAAAAAAA" + b"CGT" + b"AAAAAAAA",
}


@pytest.mark.parametrize("name", sorted(CRAFTED))
@pytest.mark.parametrize("min_copies", [2, 3])
def test_crafted_texts(built_lib, name, min_copies):
    for trim, seq in ((0, CRAFTED[name]), (0, _pad(CRAFTED[name])), (0, CRAFTED[name] * 3)):
        _same_on_both_paths(seq, min_copies, threads=(1, 4), trim=trim)


def test_both_sides_of_the_cut_test(built_lib):
    """Hits handed in directly: the second starts M + 1 (no cut: the merge test
    must see it) and M + 2 (a cut) after the reach of the first, for a one-base
    and a three-base unit; and the same with the ends alone M + 1 / M + 2 apart."""
    import numpy as np
    from bwtmi import _lib
    from bwtmi.records import Job
    for unit, m in ((b"A", 1), (b"CAG", 3)):
        for mc in (2, 3):
            a = unit * 8
            ext = 2 * max(3 * m, 4 * (min(10, m // 2) if m >= 4 else 1))
            for gap in (m, m + 1, m + 2, ext + m + 1, ext + m + 2, ext + m + 3):
                filler = (b"GTTGCATCGGATCCTAGT" * 8)[:gap]
                seq = b"TGCATG" + a + filler + a + b"GTACCT"
                s1, s2 = 6, 6 + len(a) + gap
                # rows (start, end, unit_len, prim_len, copies)
                hits = np.array([[s1, s1 + len(a), m, m, 8], [s2, s2 + len(a), m, m, 8]], dtype=np.int64)
                out = []
                for cuts in (0, 1):
                    with _lib.knobs(FOLD_CUTS=cuts, FOLD_CHUNK=1):
                        j = Job(min_copies=mc, show_progress=True, threads=2)
                        j.add_contig("c", seq, 0, 0)
                        j.add_hits(0, hits)
                        j.postprocess()
                        out.append(j.render("strfinder"))
                assert out[0] == out[1], (unit, mc, gap)


def test_long_n_run_chain_without_a_cut(built_lib):
    """An N run of 50 kbp: a hit per unit length, about 1000 of them, chain-merging
    into one record with no cut inside -- one task folds through many nominal chunks."""
    from bwtmi import synth
    base = synth.generate_contig(30_000, 12, 0.0)
    seq = base[:15_000] + b"N" * 50_000 + base[15_000:]
    want, n = _same_on_both_paths(seq, 3, threads=(1, 8), chunks=(1, 8, 64, 0))
    assert n > 900


def test_homopolymer_long_golden_inputs(built_lib):
    """The texts of tests/golden/homopolymer_long.json (runs of 1 kbp - 200 kbp of
    one base between short flanks) through the new path."""
    with open(os.path.join(GOLDEN, "homopolymer_long.json")) as f:
        cases = json.load(f)["cases"]
    texts = sorted({c["left"] + c["base"] * c["run"] + c["right"] for c in cases}, key=len)
    assert len(texts) >= 3 and len(texts[-1]) >= 200_000
    for t in texts:
        _same_on_both_paths(t.encode(), 3, threads=(4,), chunks=(1, 64, 0), trim=0)


@pytest.mark.parametrize("task", [0, 3, -2])
def test_injected_task_failure_comes_back_as_an_error(built_lib, task):
    """BWTMI_FAIL_MERGE_CHUNK throws inside task k of the one pass (-2: the last
    task): the error comes back through the C ABI and the next run is clean."""
    from bwtmi import _lib, synth
    seq = synth.generate_contig(300_000, 4, 0.02)
    hits = _hits(seq, 3)
    assert len(hits) // 2048 + 1 > 3        # the default rule gives more than four tasks
    with _lib.knobs(FOLD_CUTS=1):
        want = _render(seq, hits, 3, 4)
        with _lib.knobs(FAIL_MERGE_CHUNK=task):
            with pytest.raises(_lib.BwtmiError, match="injected failure"):
                _render(seq, hits, 3, 4)
        assert _render(seq, hits, 3, 4) == want
    with _lib.knobs(FOLD_CUTS=0):
        assert _render(seq, hits, 3, 4) == want


# chr01 / CHR1 / chr1 share a natural sort key: one fold unit of three contigs.
# chr1 is 54 bp, at most twice the trim, so its trim offset is 0 and the others'
# is 30; chr2 is a unit of its own.
COLLIDING = ("chr01", "CHR1", "chr1")


def write_colliding_fasta(path):
    from bwtmi import synth
    a = synth.generate_contig(24_000, 71, 0.03).decode()
    b = synth.generate_contig(14_000, 72, 0.0).decode()
    c = "TG" + "CAG" * 9 + "ACACACACACAC" + "AAAAAAAAAT" + "GTC"
    assert len(c) == 54
    with open(path, "w") as f:
        for name, s in (("chr01", a), ("chr2", b[:9000]), ("CHR1", b), ("chr1", c)):
            f.write(f">{name}\n")
            for i in range(0, len(s), 60):
                f.write(s[i:i + 60] + "\n")


@pytest.fixture(scope="module")
def colliding(tmp_path_factory, built_lib):
    """The FASTA and the reference post-processing's bed and vcf text for it."""
    from oracle import post
    fa = str(tmp_path_factory.mktemp("unit") / "colliding.fa")
    write_colliding_fasta(fa)
    return fa, {fmt: post.run_file(fa, fmt) for fmt in ("bed", "vcf")}


def _colliding_job(fa, threads):
    from bwtmi import _lib
    from test_host import _native_job
    j = _native_job(fa, dict(fmt="bed", mc=3, trim=30, tier2=True))
    j.params.threads = threads
    _lib.check(_lib.lib().bwtmi_job_set_params(j.h, ctypes.byref(j.params)))
    return j


def test_unit_of_three_contigs_with_two_trim_offsets(colliding):
    """Fold and refine in the trimmed frame, each record to its own contig's full
    frame, then order, collapse and filter -- in the one segment such a unit is."""
    from bwtmi import _lib
    fa, want = colliding
    rows = want["bed"].splitlines()
    for name in COLLIDING:
        assert sum(r.startswith(name + "\t") for r in rows) >= 1, name
    for cuts in (0, 1):
        for chunk in (0, 1, 8):
            for threads in (1, 4):
                with _lib.knobs(FOLD_CUTS=cuts, FOLD_CHUNK=chunk):
                    j = _colliding_job(fa, threads)
                    j.postprocess()
                    for fmt in ("bed", "vcf"):
                        assert j.render(fmt).decode() == want[fmt], (cuts, chunk, threads, fmt)


@pytest.mark.parametrize("task", [0, -2])
def test_injected_task_failure_in_a_unit_of_several_contigs(colliding, task):
    from bwtmi import _lib
    fa, want = colliding
    with _lib.knobs(FAIL_MERGE_CHUNK=task):
        j = _colliding_job(fa, 4)
        with pytest.raises(_lib.BwtmiError, match="injected failure"):
            j.postprocess()
    j = _colliding_job(fa, 4)
    j.postprocess()
    assert j.render("bed").decode() == want["bed"]
