#!/usr/bin/env python3
"""Generate the committed golden vectors from the REFERENCE itself.

Runs only in the build container, where /root/reference (wyim-pgl/bwt-algorithm
@ 2025-11-14, pure Python) is importable; the GPU box never sees it.  Nothing
here is product code.  Outputs land in tests/golden/ as small data files:

  fixtures      reference CLI (`bwt.py IN.fa --jobs -1 ...`) on the reference's
                own FASTA fixtures + crafted edge files + seeded small synthetic
                contigs -> expected output files (*.out) and expected_cli.json
  rawhits       Tier2LCPFinder.find_long_unit_repeats_strict raw hit lists
  index         BWTCore arrays (SA, BWT, C, Occ, sampled SA, 8-mer hash),
                Kasai LCP, backward_search / locate / get_kmer_positions
  index_rates   BWTCore at other sample rates (1 .. n + 1, 2048) and on alphabets
                of up to 94 symbols: Occ checkpoints, sampled SA, backward_search
  motif         MotifUtils known answers
  library       library finders off the CLI path: short imperfect repeats
                (FM seeds + Hamming seed-and-extend), LCP plateaus, Tier 1
  tier3         Tier3LongReadFinder on seeded contigs + long reads (library
                call) and the CLI with --tier3 --long-reads (FASTA and FASTQ
                reads, four formats, parallel and sequential modes)
  edge          reference CLI on crafted edge inputs (natural-key collisions,
                CRLF / CR line ends, '$' in sequences, 0-64 bp contigs,
                non-ASCII text) -> expected_edge.json
  simple        Tier2LCPFinder.find_long_repeats (_find_repeats_simple) on
                small seeded / crafted / edge contigs (each well inside the
                reference's 30 s wall-clock stop)
  hybrid        reference post-processing with the strict scan (and the
                O(k^2) nested-suppression loop) swapped for the oracle's
                restatements -> full-size output SHA-256; the
                swap is validated against the pure reference on every fixture
                by `fixtures --check-hybrid`.  Inputs with assembly gaps
                (N runs) also swap align_repeat_region's one-base case for
                its closed form, checked against the reference function on
                20000 random cases before the run.
"""
from __future__ import annotations

import argparse
import contextlib
import hashlib
import io
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
REF = "/root/reference"
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "bwt-algorithm_amd"))

FIXTURE_FASTAS = ["synthetic_test.fa", "test.fa", "test1.fa", "test2.fa", "test_all_12.fa",
                  "test_long_motif.fa", "test_repeat.fa", "test_seq1.fa", "test_simple.fasta",
                  "test_synthetic.fasta"]
FORMATS = ["strfinder", "bed", "vcf", "trf_table", "trf_dat"]


def ref_module():
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import bwt as ref  # noqa: E402  (the reference, build container only)
    return ref


def sha(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def run_ref_cli(ref, args, cwd):
    old = os.getcwd(), sys.argv
    try:
        os.chdir(cwd)
        sys.argv = ["bwt.py"] + list(args)
        with contextlib.redirect_stdout(io.StringIO()):
            ref.main()
    finally:
        os.chdir(old[0])
        sys.argv = old[1]


# --------------------------------------------------------------------- inputs
EDGE_FA = """>chr10 some description
ACGTTGCAAGTCAGTCAGTCAGTCGGATCCNNNNNNNNNNNNNNNNNNNNACGTAGCTAGCTACGATCG
acgtacgtacgtacgtTTAGGCATCGATCGAaaaaaaaaaaGCGCGCGCATCRYRYRYRYRYRYGATTACA

GATCGATCGTAGCTAGCTAGGGCCCAGCAGCAGCAGCAGCAGCAGCAGCAGCAGCAGCAGCTGCTGCTGCTG
CTGCTGCTGACGATCGATTTTTTTTTTTTTTGACTAGCATCGATCGATTAGACAGACAGACAGACAGACAGA
>chr2
GGATCCGATCGATGCATCGATCGGCATGCATCGATCGGGAAGGAAGGAAGGAAGGAAGGAAGGCTAGCTAGCAT
CGATCGATGCATGCAACACACACACACACACATGTGTGTGTGTGTGTATCGATCGATCGGCTAGCTAGCTAGG
ATCGATCGTACGATCGTAGCTAGCATGCATCAGCAGCAGCAGCAGCAGCAGCAGCAGCAGCAGCAGTTGTTGTT
GTTGTTGTTGATCGATCGTACGTAGCTAGCTAGCATCGATGCATCGACTGCATGCAAAAAAAAAAAAAAAAACG
>Chr1
ACGTACGTTTTTTTTTGGGGGGGGATATATATATATCGCGCG
>chr3
TGCATGCAGGTCAGTCAGTCAGTCAGTCAGTCAGTCAGTCGGTCAGTCAGTTAGTCAGTCAGTCAGTCCATCAT
GCATCGATCGATCGGCTAGCTAGCTAGCTCATCATCATCATCATCATCATCATCATCATCATCATCATCTGCTG
CTGCTGCTGCTGCTGCTGAGAGAGAGAGAGAGAGCGATCGATTGCATGCACCGCCGCCGCCGCCGATCGATCGA
"""


def write_inputs(dst):
    from bwtmi import synth
    os.makedirs(dst, exist_ok=True)
    for fa in FIXTURE_FASTAS:
        shutil.copy(os.path.join(REF, fa), os.path.join(dst, fa))
    with open(os.path.join(dst, "edge_mixed.fa"), "w") as f:
        f.write(EDGE_FA)
    synth.write_fasta(os.path.join(dst, "synth_small.fa"), [3000, 2200], 0.0, first_index=101)
    synth.write_fasta(os.path.join(dst, "synth_imperfect.fa"), [3000, 2600], 0.05, first_index=201)
    synth.write_fasta(os.path.join(dst, "synth_imperfect2.fa"), [4000], 0.02, first_index=301)


CLI_CASES = []   # (name, input, args)
for fa in FIXTURE_FASTAS:
    CLI_CASES.append((f"{fa}.strfinder", fa, []))
for fmt in FORMATS[1:]:
    CLI_CASES.append((f"synthetic_test.fa.{fmt}", "synthetic_test.fa", ["--format", fmt]))
CLI_CASES += [
    ("synthetic_test.fa.tier1", "synthetic_test.fa", ["--tier1", "--max-motif-len", "6"]),
    ("synthetic_test.fa.nomm", "synthetic_test.fa", ["--no-mismatches"]),
    ("test2.fa.mc4", "test2.fa", ["--min-copies", "4"]),
    ("edge_mixed.fa.strfinder", "edge_mixed.fa", []),
    ("edge_mixed.fa.bed", "edge_mixed.fa", ["--format", "bed"]),
    ("edge_mixed.fa.trim0", "edge_mixed.fa", ["--flank-trim", "0"]),
    ("edge_mixed.fa.trim7.vcf", "edge_mixed.fa", ["--flank-trim", "7", "--format", "vcf"]),
    ("synth_small.fa.strfinder", "synth_small.fa", []),
    ("synth_small.fa.mc2", "synth_small.fa", ["--min-copies", "2"]),
    ("synth_small.fa.mc5.bed", "synth_small.fa", ["--min-copies", "5", "--format", "bed"]),
    ("synth_imperfect.fa.strfinder", "synth_imperfect.fa", []),
    ("synth_imperfect.fa.trf_table", "synth_imperfect.fa", ["--format", "trf_table"]),
    ("synth_imperfect.fa.trf_dat", "synth_imperfect.fa", ["--format", "trf_dat"]),
    ("synth_imperfect.fa.vcf", "synth_imperfect.fa", ["--format", "vcf"]),
    ("synth_imperfect2.fa.strfinder", "synth_imperfect2.fa", []),
    ("synth_imperfect2.fa.bed", "synth_imperfect2.fa", ["--format", "bed"]),
    ("test_all_12.fa.trf_table", "test_all_12.fa", ["--format", "trf_table"]),
    ("test2.fa.vcf", "test2.fa", ["--format", "vcf"]),
]


# --------------------------------------------------------------- hybrid swap
class _StubCore:
    """Index stand-in for the hybrid oracle: the CLI path consumes only
    text_arr from BWTCore (bwt.py:1910); every other array is built and
    discarded, so the hybrid skips the build."""

    def __init__(self, text, sa_sample_rate=32, occ_sample_rate=128):
        self.text = text
        self.n = len(text)
        self.text_arr = np.frombuffer(text.encode("utf-8"), dtype=np.uint8)

    def clear(self):
        self.text_arr = np.array([], dtype=np.uint8)


def _homopolymer_align(ref):
    """align_repeat_region (bwt.py:998-1102) for a one-base template and the
    default indel band, in closed form: a window whose first base differs from
    the template has the deletion end j = 0 among its best alignments (cost 1,
    tied with the substitution, first j wins), so _align_unit_to_window fails
    there and the walk stops; the consensus never changes.  The result is the
    run of the template base from `start` up to the walk's limit (bwt.py:1033).
    Validated against the reference function by `_check_homopolymer_align`
    before every use; it makes assembly gaps (N runs of up to 1 Mbp, each
    merged ~1000 times) tractable for the hybrid oracle."""
    orig = ref.MotifUtils.align_repeat_region

    def fast(sequence, start, end, motif_template, mismatch_fraction=0.1, max_indel=None, min_copies=3):
        if len(motif_template) != 1 or max_indel is not None or len(sequence) == 0:
            return orig(sequence, start, end, motif_template, mismatch_fraction, max_indel, min_copies)
        n = len(sequence)
        start = max(0, start)
        end = min(n, end if end > start else n)
        limit = min(n, max(end, start + min_copies) + 4)
        b = motif_template
        pos = start
        while pos < limit:   # run of b, stepping by long slices
            step = min(limit - pos, 4096)
            chunk = sequence[pos:pos + step]
            k = len(chunk) - len(chunk.lstrip(b))
            pos += k
            if k < step:
                break
        copies = pos - start
        if copies < min_copies or copies <= 0:
            return None
        return ref.RepeatAlignmentSummary(consensus=b, motif_len=1, copies=copies, consumed_length=copies,
                                          mismatch_rate=0.0, max_errors_per_copy=0, variations=[],
                                          copy_sequences=[b] * copies, total_insertions=0, total_deletions=0,
                                          error_counts=[0] * copies)
    return orig, fast


def _check_homopolymer_align(ref, orig, fast, cases=20000):
    """The closed form equals the reference function on random one-base
    cases: runs of the template base inside random ACGTNRY text, any start /
    end (including past the run, at the text's end and end <= start), the
    callers' min_copies and mismatch fractions."""
    rng = np.random.default_rng(0x4F11)
    alpha = "ACGTNRY"
    for i in range(cases):
        n = int(rng.integers(1, 120))
        seq = [alpha[j] for j in rng.integers(0, len(alpha), n)]
        b = alpha[int(rng.integers(0, len(alpha)))]
        for _ in range(int(rng.integers(0, 4))):
            a = int(rng.integers(0, n))
            seq[a:a + int(rng.integers(1, 40))] = [b] * int(rng.integers(1, 40))
        seq = "".join(seq)[:n] or b
        n = len(seq)
        start = int(rng.integers(-2, n + 2))
        end = int(rng.integers(-2, n + 6))
        mc = int(rng.choice([1, 2, 3, 5]))
        frac = float(rng.choice([0.1, 0.05, 0.2]))
        tmpl = b if rng.random() < 0.8 else seq[min(max(start, 0), n - 1)]
        want = orig(seq, start, end, tmpl, mismatch_fraction=frac, min_copies=mc)
        got = fast(seq, start, end, tmpl, mismatch_fraction=frac, min_copies=mc)
        if want != got:
            raise SystemExit(f"homopolymer closed form differs from the reference on case {i}: "
                             f"{seq!r} {start} {end} {tmpl!r} {frac} {mc}: {want} vs {got}")


def _long_homopolymer_cases():
    """Long one-base cases (verdict r4 #2): runs of 1 kbp - 200 kbp of the
    template base inside ACGTNRY text, the walk starting before, at and inside
    the run, its requested end inside, at and past the run (and end <= start),
    every caller's arguments: _recompute_repeat's two attempts (bwt.py:3535-
    3551: mismatch_fraction 0.1, min_copies max(1, min_copies) then 1) and
    the variation scan (bwt.py:1277: 0.1, min_copies 1), min_copies 3 and 5 of
    the CLI's --min-copies, and mismatch fractions 0.05 / 0.2."""
    rng = np.random.default_rng(0x10C6)
    alpha = "ACGTNRY"
    cases = []
    for run in (1_000, 4_999, 20_000, 75_000, 200_000):
        for b in ("N", "A", "T"):
            left = "".join(alpha[j] for j in rng.integers(0, len(alpha), int(rng.integers(0, 300))))
            right = "".join(alpha[j] for j in rng.integers(0, len(alpha), int(rng.integers(0, 300))))
            left = left.rstrip(b)
            right = right.lstrip(b)
            seq = left + b * run + right
            r0, r1 = len(left), len(left) + run
            starts = [max(0, r0 - 7), r0, r0 + int(rng.integers(1, run))]
            for st in starts:
                ends = [st, st - 3, min(len(seq), st + int(rng.integers(1, 40))), r1 - int(rng.integers(0, 5)), r1,
                        min(len(seq) + 10, r1 + int(rng.integers(1, 50)))]
                for en in ends:
                    mc = int(rng.choice([1, 2, 3, 5]))
                    frac = float(rng.choice([0.1, 0.1, 0.05, 0.2]))
                    cases.append(dict(left=left, base=b, run=run, right=right, start=st, end=en, min_copies=mc,
                                      mismatch_fraction=frac))
    return cases


def _check_homopolymer_align_long(ref, orig, fast):
    """The closed form against the reference function on _long_homopolymer_cases."""
    for i, c in enumerate(_long_homopolymer_cases()):
        seq = c["left"] + c["base"] * c["run"] + c["right"]
        want = orig(seq, c["start"], c["end"], c["base"], mismatch_fraction=c["mismatch_fraction"],
                    min_copies=c["min_copies"])
        got = fast(seq, c["start"], c["end"], c["base"], mismatch_fraction=c["mismatch_fraction"],
                   min_copies=c["min_copies"])
        if want != got:
            raise SystemExit(f"homopolymer closed form differs from the reference on long case {i}: "
                             f"{ {k: v for k, v in c.items() if k not in ('left', 'right')} }")


def install_hybrid(ref, stub_index=True, restate_nested=True, homopolymer=False):
    import oracle
    from oracle import post

    def fast_strict(self, chromosome, min_unit_len=20, max_unit_len=120, max_mismatch=2,
                    min_copies=3):
        t = self.bwt.text_arr
        hits = oracle.strict_scan(t, min_unit_len, max_unit_len, max_mismatch, min_copies)
        out = []
        for s, e, L, p, c in hits.tolist():
            motif = bytes(t[s:s + p]).decode("ascii", errors="replace")
            pm, pi, sc, comp, ent, act = ref.MotifUtils.calculate_trf_statistics(t, s, e, motif, c, 0.0)
            out.append(ref.TandemRepeat(
                chrom=chromosome, start=s, end=e, motif=motif, copies=float(c), length=e - s,
                tier=2, confidence=0.95, consensus_motif=motif, mismatch_rate=0.0,
                max_mismatches_per_copy=0 if pm >= 99.9 else max_mismatch, n_copies_evaluated=c,
                strand="+", percent_matches=pm, percent_indels=pi, score=sc, composition=comp,
                entropy=ent, actual_sequence=act, variations=None))
        return out

    ref.Tier2LCPFinder.find_long_unit_repeats_strict = fast_strict
    if stub_index:
        ref.BWTCore = _StubCore
    if restate_nested:
        def nested(self, repeats, overlap_threshold=0.5):
            return post.Pipeline({}, {}, {}).suppress_nested(repeats, overlap_threshold)
        ref.TandemRepeatFinder._suppress_nested_short_calls = nested
    if homopolymer:
        orig, fast = _homopolymer_align(ref)
        _check_homopolymer_align(ref, orig, fast)
        _check_homopolymer_align_long(ref, orig, fast)
        ref.MotifUtils.align_repeat_region = staticmethod(fast)


# ------------------------------------------------------------------ commands
def cmd_fixtures(a):
    ref = ref_module()
    inp = os.path.join(HERE, "inputs")
    write_inputs(inp)
    out_dir = os.path.join(HERE, "cli")
    os.makedirs(out_dir, exist_ok=True)
    manifest = {}
    work = tempfile.mkdtemp()
    for name, fa, args in CLI_CASES:
        t0 = time.time()
        dst = os.path.join(out_dir, name + ".out")
        shutil.copy(os.path.join(inp, fa), os.path.join(work, fa))
        run_ref_cli(ref, [fa, "-o", "out.tab", "--jobs", "-1"] + args, work)
        shutil.copy(os.path.join(work, "out.tab"), dst)
        manifest[name] = dict(input=fa, args=args, sha256=sha(dst))
        print(f"{name}: {time.time() - t0:.1f}s {manifest[name]['sha256'][:12]}", flush=True)
    with open(os.path.join(HERE, "expected_cli.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    if a.check_hybrid:
        install_hybrid(ref, stub_index=True, restate_nested=True)
        bad = 0
        for name, fa, args in CLI_CASES:
            run_ref_cli(ref, [fa, "-o", "hy.tab", "--jobs", "-1"] + args, work)
            ok = sha(os.path.join(work, "hy.tab")) == manifest[name]["sha256"]
            bad += not ok
            print(f"hybrid {name}: {'OK' if ok else 'MISMATCH'}", flush=True)
        if bad:
            raise SystemExit(f"hybrid oracle disagrees with reference on {bad} case(s)")


def _contigs_of(ref, path, flank=30):
    f = ref.TandemRepeatFinder(path, flank_trim=flank)
    return f.load_reference()


def cmd_rawhits(a):
    ref = ref_module()
    inp = os.path.join(HERE, "inputs")
    res = {}
    for fa in ["synthetic_test.fa", "test.fa", "test2.fa", "test_all_12.fa", "test_long_motif.fa",
               "edge_mixed.fa", "synth_small.fa", "synth_imperfect.fa"]:
        seqs = _contigs_of(ref, os.path.join(inp, fa))
        for chrom, seq in seqs.items():
            core = ref.BWTCore(seq + "$", 32)
            for mc in ([3, 2, 4] if fa == "synth_small.fa" else [3]):
                U = max(120, min(len(seq) // mc, 1000))
                t2 = ref.Tier2LCPFinder(core, min_period=1)
                hits = t2.find_long_unit_repeats_strict(chrom, min_unit_len=1, max_unit_len=U,
                                                        max_mismatch=0, min_copies=mc)
                res[f"{fa}|{chrom}|mc{mc}"] = dict(
                    seq=seq, U=U, min_copies=mc,
                    hits=[[h.start, h.end, h.motif, int(h.copies)] for h in hits])
            print(fa, chrom, len(seq), flush=True)
    # a mismatch-tolerant call of the same function (library use, bwt.py:1941)
    seqs = _contigs_of(ref, os.path.join(inp, "synth_imperfect.fa"))
    chrom, seq = next(iter(seqs.items()))
    core = ref.BWTCore(seq + "$", 32)
    hits = ref.Tier2LCPFinder(core).find_long_unit_repeats_strict(chrom, 4, 40, 2, 3)
    res["synth_imperfect.fa|mm2"] = dict(seq=seq, U=40, min_unit=4, max_mismatch=2, min_copies=3,
                                         hits=[[h.start, h.end, h.motif, int(h.copies)] for h in hits])
    with open(os.path.join(HERE, "rawhits.json"), "w") as f:
        json.dump(res, f)


def cmd_index(a):
    ref = ref_module()
    from bwtmi import synth
    inp = os.path.join(HERE, "inputs")
    texts = {}
    for fa in ["test2.fa", "edge_mixed.fa"]:
        for chrom, seq in _contigs_of(ref, os.path.join(inp, fa)).items():
            texts[f"{fa}|{chrom}"] = seq
    texts["synth10k"] = synth.generate_contig(10000, 7).decode()
    texts["lower_mixed"] = "acgtNNACGTacgtRYKMacgtacgtTTTTTTTTtttt$$ACGT"[:40]
    texts["tiny"] = "A"
    texts["empty"] = ""
    rng = np.random.default_rng(5)
    pats = ["", "A", "C", "G", "T", "N", "$", "X", "AC", "ACG", "ACGT", "TTTT", "GATC",
            "CAGCAG", "NNNN", "acgt", "AAAAAAAAA"]
    for k in range(1, 11):
        for _ in range(4):
            pats.append("".join(rng.choice(list("ACGT"), k)))
    arrays = {}
    meta = {}
    for name, seq in texts.items():
        text = seq + "$"
        core = ref.BWTCore(text, 32)
        key = name.replace("|", "__").replace(".", "_")
        arrays[key + "__text"] = np.frombuffer(text.encode(), dtype=np.uint8)
        arrays[key + "__sa"] = np.asarray(core.suffix_array, dtype=np.int32)
        arrays[key + "__bwt"] = np.asarray(core.bwt_arr, dtype=np.uint8)
        arrays[key + "__lcp"] = np.asarray(ref.Tier2LCPFinder(core)._compute_lcp_array(), dtype=np.int32)
        occ = {str(c): v.tolist() for c, v in core.occ_checkpoints.items()}
        kh = {str(c): v for c, v in core.kmer_hash.items()}
        bs = {p: list(core.backward_search(p)) for p in pats}
        loc = {p: core.locate_positions(p) for p in pats if p}
        kp = {p: core.get_kmer_positions(p) for p in ["ACGT", "A", "CAG", "GATCGATC", "AC", "TTTTTTTT"]}
        meta[key] = dict(name=name, C={str(ord(c)): v for c, v in core.char_counts.items()},
                         totals={str(ord(c)): v for c, v in core.char_totals.items()},
                         occ=occ, sampled={str(k): int(v) for k, v in core.sampled_sa.items()},
                         kmer_hash=kh, backward=bs, locate=loc, kmer_positions=kp)
    np.savez_compressed(os.path.join(HERE, "index_arrays.npz"), **arrays)
    with open(os.path.join(HERE, "index_meta.json"), "w") as f:
        json.dump(meta, f)


RATE_NS = [1, 2, 15, 16, 17, 127, 128, 129, 300]          # text lengths, sentinel included
_PRINTABLE = bytes(c for c in range(0x21, 0x7F) if c != ord("$")).decode()   # 93 symbols
RATE_ALPHABETS = ["ACGT", "ACGTN", "ACGTNRYKM", _PRINTABLE[:15], _PRINTABLE[:16], _PRINTABLE[:17],
                  _PRINTABLE[:40], _PRINTABLE]


def rate_pairs(n):
    """(sa_sample_rate, occ_sample_rate) of the index_rates grid for a text of n bytes."""
    return [(1, 1), (7, 16), (32, 48), (33, 100), (1000, 1024), (n, n), (n + 1, n + 1), (2, 2048), (31, 7)]


def cmd_index_rates(a):
    """BWTCore(text, sa_sample_rate, occ_sample_rate) of the reference at rates
    other than 32 / 128 and on alphabets of up to 94 symbols ->
    index_rates.json.  Per text (RATE_NS x RATE_ALPHABETS, random symbols with
    one planted run, + '$'): the text, the byte codes present, a few patterns,
    and per case a row [sa, occ, occ_len, sampled_len] of rate_pairs with the
    reference's two lengths.  The numbers themselves -- per case, in this
    order: the Occ checkpoint row of every byte code of the text (ascending),
    the sampled SA values (keys 0, sa, 2 sa, ... checked here), (sp, ep) of
    every pattern -- are one little-endian int16 stream per text (every value
    is in -1 .. 300), zlib-compressed and base64-encoded ("stream"), which
    keeps 648 cases under 100 KB.  SA and BWT do not depend on the rates and
    are not stored.  tests/test_oracle.py reads the file."""
    import base64
    import zlib
    ref = ref_module()
    out = {}
    ncases = 0
    for ai, alpha in enumerate(RATE_ALPHABETS):
        for n in RATE_NS:
            rng = np.random.default_rng(1000 * ai + n)
            body = [alpha[j] for j in rng.integers(0, len(alpha), n - 1)]
            if n >= 17:
                p = int(rng.integers(0, n - 9))
                body[p:p + 8] = [body[p]] * 8
            body = "".join(body)[:n - 1]
            text = body + "$"
            assert len(text) == n and text.isascii()
            pats = ["", "$", " ", text[:1], text[:1] * 2, text[:2], text[-3:], text[n // 2:n // 2 + 3],
                    body[-1:] + body[:1]]
            pats = list(dict.fromkeys(pats))
            stream, cases, codes = [], [], None
            for sa, occ in rate_pairs(n):
                core = ref.BWTCore(text, sa, occ)
                cp = {int(c): np.asarray(v).tolist() for c, v in core.occ_checkpoints.items()}
                if codes is None:
                    codes = sorted(cp)
                assert sorted(cp) == codes == sorted(set(text.encode()))
                lens = {len(v) for v in cp.values()}
                assert len(lens) == 1
                for c in codes:
                    stream += cp[c]
                samp = {int(k): int(v) for k, v in core.sampled_sa.items()}
                assert list(samp) == list(range(0, n, sa)), (n, sa)
                stream += list(samp.values())
                for p in pats:
                    stream += [int(x) for x in core.backward_search(p)]
                cases.append([sa, occ, lens.pop(), len(samp)])
                ncases += 1
            assert min(stream) >= -1 and max(stream) <= 300
            blob = zlib.compress(np.asarray(stream, dtype="<i2").tobytes(), 9)
            out[f"a{ai}_n{n}"] = dict(text=text, patterns=pats, cases=cases, values=len(stream),
                                      stream=base64.b64encode(blob).decode())
    path = os.path.join(HERE, "index_rates.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(ncases, "cases", os.path.getsize(path), "bytes")


def cmd_motif(a):
    ref = ref_module()
    M = ref.MotifUtils
    words = ["ATCG", "CGAT", "AAAA", "ATAT", "GCGGCG", "TGCTGATCGTAGCTAGCTGA", "CAG", "A", "",
             "NNAC", "ACGTN", "TTAGGG", "GATCGATC", "RYRY"]
    out = dict(
        canonical={w: M.get_canonical_motif(w) for w in words},
        stranded={w: list(M.get_canonical_motif_stranded(w)) for w in words},
        revcomp={w: M.reverse_complement(w) for w in words},
        entropy={w: float(M.calculate_entropy(w)) for w in words},
        primitive={w: M.is_primitive_motif(w) for w in words},
        period={w: M.smallest_period_str(w) for w in words},
        hamming=[[s1, s2, M.hamming_distance(s1, s2)] for s1, s2 in
                 [("ATCG", "ATGG"), ("ATCG", "GGGG"), ("AAAA", "TTTT"), ("AC", "ACG")]],
        edit=[[s1, s2, M.edit_distance(s1, s2)] for s1, s2 in
              [("ACGT", "AGT"), ("", "AC"), ("CAGCAG", "CAGAG"), ("ATCG", "TACG")]],
        consensus=[[seqs, list(M.build_consensus_motif(seqs))] for seqs in
                   [["ATCG", "ATCG", "ATGG"], ["AAA", "AAT", "ATT"], ["CG"]]],
        composition={w: M.calculate_composition(w) for w in words},
        score=[[l, mm, M.calculate_trf_score("A", 3, mm, l)] for l, mm in
               [(10, 0.0), (35, 0.1), (100, 0.333), (7, 0.9)]],
        enumerate={k: len(list(M.enumerate_motifs(k))) for k in range(1, 7)},
    )
    aligns = []
    cases = [("ACGTTACGTACGTAACGTACGT", 0, 22, "ACGT"),
             ("CAGCAGCAGCAAGCAGCAGTCAGCAG", 0, 26, "CAG"),
             ("TCATCGGTCATCGGTCATCGGTCATCGGTCAACGGTCATCGGGTCATCGG", 0, 50, "TCATCGG"),
             ("AAAAAAAAAA", 0, 10, "AA"), ("GATTACA", 2, 1, "TTA")]
    for seq, s, e, m in cases:
        for mc in (1, 3):
            r = M.align_repeat_region(seq, s, e, m, min_copies=mc)
            aligns.append([seq, s, e, m, mc, None if r is None else dict(
                consensus=r.consensus, copies=r.copies, consumed=r.consumed_length,
                mismatch_rate=r.mismatch_rate, max_err=r.max_errors_per_copy,
                variations=r.variations, ins=r.total_insertions, dele=r.total_deletions)])
    out["align"] = aligns
    with open(os.path.join(HERE, "motif_known.json"), "w") as f:
        json.dump(out, f, indent=1)


def _rec_json(r):
    import dataclasses
    d = dataclasses.asdict(r)
    for k, v in list(d.items()):
        if isinstance(v, np.generic):
            d[k] = v.item()
    return d


def _crafted_short(seed: int, n_segments: int = 30) -> bytes:
    """Random spacers + short imperfect arrays (units 2-9 bp, 3-13 copies,
    transition-only substitutions at 4 %), most preceded by 'A' * (8 - k): the
    reference's k-mer lookup for k < 8 returns positions of that padded
    8-mer, so these arrays actually get seeded."""
    r = np.random.default_rng(seed)
    B = b"ACGT"
    trans = {ord("A"): ord("G"), ord("G"): ord("A"), ord("C"): ord("T"), ord("T"): ord("C")}
    out = bytearray()
    for _ in range(n_segments):
        out += bytes(B[i] for i in r.integers(0, 4, int(r.integers(10, 60))))
        k = int(r.choice([2, 3, 4, 5, 6, 7, 8, 9]))
        if r.random() < 0.6 and k < 8:
            out += b"A" * (8 - k)
        unit = bytes(B[i] for i in r.integers(0, 4, k))
        arr = bytearray(unit * int(r.integers(3, 14)))
        for q in range(len(arr)):
            if r.random() < 0.04:
                arr[q] = trans[arr[q]]
        out += arr
    return bytes(out)


def cmd_library(a):
    """Library finders that are not on the CLI path (SURVEY.md §8(a) A2-9, A2-10,
    §8(f) #2): Tier2LCPFinder.find_short_imperfect_repeats (FM seeds + Hamming
    seed-and-extend + majority vote), Tier2LCPFinder._detect_lcp_plateaus over
    the Kasai LCP, Tier1STRFinder.find_strs -> library.json."""
    ref = ref_module()
    from bwtmi import synth
    cases = {}
    for name, n, idx, sub in [("imp3k", 3000, 501, 0.03), ("imp10k", 10000, 502, 0.03),
                              ("imp2k_dense", 2000, 504, 0.05)]:
        cases[name] = synth.generate_contig(n, idx, sub).decode()
    for seed in (1, 2, 3):
        cases[f"craft{seed}"] = _crafted_short(seed).decode()
    with open(os.path.join(HERE, "inputs", "test2.fa")) as f:
        cur = None
        for line in f:
            line = line.strip()
            if line.startswith(">"):
                cur = "test2_" + line[1:].split()[0]
                cases[cur] = ""
            elif cur:
                cases[cur] += line.upper()
    out = {}
    for name, seq in cases.items():
        t0 = time.time()
        core = ref.BWTCore(seq + "$", 32)
        f = ref.Tier2LCPFinder(core)
        with contextlib.redirect_stdout(io.StringIO()):
            short = f.find_short_imperfect_repeats(name, set())
            lcp = f._compute_lcp_array()
            plate = f._detect_lcp_plateaus(lcp, name)
            t1 = ref.Tier1STRFinder(core.text_arr, 9, False).find_strs(name)
        out[name] = dict(seq=seq, short_imperfect=[_rec_json(r) for r in short],
                         lcp_plateaus=[_rec_json(r) for r in plate], tier1=[_rec_json(r) for r in t1],
                         seconds=round(time.time() - t0, 1))
        print(name, len(seq), len(short), len(plate), len(t1), out[name]["seconds"], flush=True)
    with open(os.path.join(HERE, "library.json"), "w") as f:
        json.dump(out, f, indent=0)


def _tier3_inputs():
    """Seeded contigs with long-period arrays (10-160 bp units, some with 2 %
    substitutions, one 3 bp array, one array at a contig's end) and long reads
    sampled over them (1 % noise on some), plus random, short and lower-case
    reads.  Returns ({name: seq}, [reads as str])."""
    r = np.random.default_rng(7)
    B = "ACGT"

    def rnd(n):
        return "".join(B[i] for i in r.integers(0, 4, n))

    def array(unit, copies, sub):
        s = list(unit * copies)
        for q in range(len(s)):
            if r.random() < sub:
                s[q] = B[(B.index(s[q]) + int(r.integers(1, 4))) % 4]
        return "".join(s)

    plan = {"chrT1": [(12, 70, 0.0), (40, 25, 0.02), (77, 12, 0.0), (3, 300, 0.0), (160, 6, 0.0)],
            "chrT2": [(25, 40, 0.0), (120, 8, 0.02), (33, 30, 0.0)],
            "chrT10": [(50, 20, 0.0), (18, 50, 0.0)]}
    contigs, spans = {}, []
    for name, arrs in plan.items():
        seq = rnd(400)
        for (u, c, sub) in arrs:
            a0 = len(seq)
            seq += array(rnd(u), c, sub)
            spans.append((name, a0, len(seq)))
            seq += rnd(int(r.integers(300, 900)))
        if name == "chrT10":          # an array running to the contig's end
            a0 = len(seq)
            seq += array(rnd(45), 14, 0.0)
            spans.append((name, a0, len(seq)))
        contigs[name] = seq
    reads = []
    for (name, a0, a1) in spans:
        seq = contigs[name]
        for _ in range(2):
            s0 = max(0, a0 - int(r.integers(60, 420)))
            ln = int(r.integers(1000, 2600))
            rd = list(seq[s0:s0 + ln])
            if r.random() < 0.3:
                for q in range(len(rd)):
                    if r.random() < 0.01:
                        rd[q] = B[(B.index(rd[q]) + 1) % 4]
            reads.append("".join(rd))
    reads.append(rnd(1500))                                 # no repeat
    reads.append(contigs["chrT1"][350:1200])                # < 1000: skipped
    reads.append(contigs["chrT2"][300:1900].lower())        # lower case (the CLI upper-cases)
    reads.append(contigs["chrT1"][:1400] + contigs["chrT2"][400:1500])   # chimeric
    return contigs, reads


def cmd_tier3(a):
    """Tier 3 long-read anchoring: the library call on each
    contig (trimmed as the CLI does, + '$') and CLI runs -> tier3.json, inputs
    tier3.fa / tier3_reads.fa / tier3_reads.fq."""
    ref = ref_module()
    contigs, reads = _tier3_inputs()
    inp = os.path.join(HERE, "inputs")
    with open(os.path.join(inp, "tier3.fa"), "w") as f:
        for name, seq in contigs.items():
            f.write(f">{name}\n")
            for i in range(0, len(seq), 60):
                f.write(seq[i:i + 60] + "\n")
    with open(os.path.join(inp, "tier3_reads.fa"), "w") as f:
        for i, rd in enumerate(reads):
            f.write(f">read{i}\n")
            for q in range(0, len(rd), 70):
                f.write(rd[q:q + 70] + "\n")
    with open(os.path.join(inp, "tier3_reads.fq"), "w") as f:
        for i, rd in enumerate(reads[:8]):
            f.write(f"@read{i}\n{rd}\n+\n{'I' * len(rd)}\n")
    out = {"library": {}, "cli": {}}
    for name, seq in contigs.items():
        trimmed = seq[30:-30]
        core = ref.BWTCore(trimmed + "$", 32)
        t0 = time.time()
        recs = ref.Tier3LongReadFinder(core).find_very_long_repeats(reads, name)
        out["library"][name] = dict(records=[_rec_json(x) for x in recs], seconds=round(time.time() - t0, 1))
        print(name, len(seq), len(recs), out["library"][name]["seconds"], flush=True)
    work = tempfile.mkdtemp()
    for fn in ("tier3.fa", "tier3_reads.fa", "tier3_reads.fq"):
        shutil.copy(os.path.join(inp, fn), os.path.join(work, fn))
    cases = [("fa.strfinder", ["--long-reads", "tier3_reads.fa", "--jobs", "2"]),
             ("fa.bed", ["--long-reads", "tier3_reads.fa", "--jobs", "2", "--format", "bed"]),
             ("fa.vcf", ["--long-reads", "tier3_reads.fa", "--jobs", "2", "--format", "vcf"]),
             ("fa.trf_dat", ["--long-reads", "tier3_reads.fa", "--jobs", "2", "--format", "trf_dat"]),
             ("fq.strfinder", ["--long-reads", "tier3_reads.fq", "--jobs", "2"]),
             ("fa.sequential", ["--long-reads", "tier3_reads.fa", "--jobs", "-1"])]
    for tag, extra in cases:
        t0 = time.time()
        run_ref_cli(ref, ["tier3.fa", "--tier3", "-o", "out.tab"] + extra, work)
        with open(os.path.join(work, "out.tab"), "rb") as f:
            data = f.read()
        out["cli"][tag] = dict(args=["--tier3"] + extra, sha256=hashlib.sha256(data).hexdigest(),
                               text=data.decode(), seconds=round(time.time() - t0, 1))
        print(tag, out["cli"][tag]["sha256"][:16], data.count(b"\n"), out["cli"][tag]["seconds"], flush=True)
    with open(os.path.join(HERE, "tier3.json"), "w") as f:
        json.dump(out, f, indent=0)


def cmd_simple(a):
    """Tier2LCPFinder.find_long_repeats -> _find_repeats_simple (SURVEY.md §8(f)
    #4) -> simple.json.  The reference stops after 30 s of wall time
    (bwt.py:2238-2257); every case here finishes well inside it (the time is
    recorded), so the stop never fired and the output is deterministic."""
    ref = ref_module()
    from bwtmi import synth
    contigs, _ = _tier3_inputs()
    cases = {
        "imp1500": (synth.generate_contig(1500, 601, 0.03).decode(), {}),
        "imp1200_nomm": (synth.generate_contig(1200, 604, 0.03).decode(), dict(allow_mismatches=False)),
        "imp900": (synth.generate_contig(900, 602, 0.02).decode(), {}),
        "long_t2_p20": (contigs["chrT2"][:1100], dict(min_period=20, max_period=60)),
        "long_t1_p10": (contigs["chrT1"][:1200], dict(min_period=10, max_period=45)),
        "imp11k_p40": (synth.generate_contig(11000, 603, 0.02).decode(), dict(min_period=40)),
    }
    with open(os.path.join(HERE, "inputs", "edge_mixed.fa")) as f:
        cur = None
        for line in f:
            line = line.strip()
            if line.startswith(">"):
                cur = "edge_" + line[1:].split()[0]
                cases[cur] = ("", {})
            elif cur:
                cases[cur] = (cases[cur][0] + line, {})
    out = {}
    for name, (seq, kw) in cases.items():
        core = ref.BWTCore(seq + "$", 32)
        f = ref.Tier2LCPFinder(core, **kw)
        seen = set()
        if name == "imp1500":   # with a Tier 1 mask, as the library's callers pass it
            with contextlib.redirect_stdout(io.StringIO()):
                seen = {(r.start, r.end) for r in ref.Tier1STRFinder(core.text_arr, 9, False).find_strs(name)}
        t0 = time.time()
        with contextlib.redirect_stdout(io.StringIO()):
            recs = f.find_long_repeats(name, seen)
        dt = time.time() - t0
        assert dt < 29.5, f"{name}: {dt:.1f} s -- the reference's 30 s stop may have fired"
        out[name] = dict(seq=seq, params=kw, tier1_seen=sorted(seen), records=[_rec_json(r) for r in recs],
                         seconds=round(dt, 1))
        print(name, len(seq), len(recs), round(dt, 1), flush=True)
    with open(os.path.join(HERE, "simple.json"), "w") as f:
        json.dump(out, f, indent=0)


# ------------------------------------------------- library finders: edge inputs
SIMPLE_EDGE_PERIODS = (63, 64, 65, 100, 127, 128, 129, 191, 192, 193, 200)
# text seeds other than 1000 + p: with those flanks the walk of a short period stops advancing on a
# small array (it resumes at an array end that is not past its position) and uses up the reference's
# 100,000 iterations before the long periods are walked with default parameters
SIMPLE_EDGE_SEEDS = {191: 3191, 200: 3200}
MANY_SYMBOLS = "ACGTRYKMSW"
PLATEAU_KEYS = ("start", "end", "motif", "copies", "length", "tier", "confidence")


def _period_text(p: int, sub: bool, copies: int, flank: int, seed: int) -> str:
    """rnd(flank) + unit * copies + unit[:p // 2] + rnd(flank) over ACGT.  With
    sub, every copy after the third and the half copy carry one substitution
    (A<->C, G<->T), each in a column of its own: extension with mismatches
    (period <= 64) takes those copies, exact extension (period >= 65) stops
    after three, and the partial copy ends at the substitution either way.
    With three copies the substitution sits at 85 % of the third: exact
    extension keeps two copies and the array passes only as two copies plus a
    partial one of >= 0.75."""
    r = np.random.default_rng(seed)
    B = "ACGT"

    def rnd(k):
        return "".join(B[i] for i in r.integers(0, 4, k))

    left, unit, right = rnd(flank), rnd(p), rnd(flank)
    arr = list(unit * copies + unit[:p // 2])
    if sub:
        swap = {"A": "C", "C": "A", "G": "T", "T": "G"}
        for c in range(3, copies):
            q = c * p + (7 + 13 * c) % p
            arr[q] = swap[arr[q]]
        if copies == 3:
            q = 2 * p + (85 * p) // 100
            arr[q] = swap[arr[q]]
        q = copies * p + p // 4
        arr[q] = swap[arr[q]]
    return left + "".join(arr) + right


def _flank(r, k: int, unit: str = "", nxt: str = "") -> str:
    """k random ACGT bases that do not continue a neighbouring array: the last
    is a transversion of the last base of `unit` (the array that follows) and
    the first one of the first base of `nxt` (the array before).  A frame
    shifted into the flank then cannot extend, and _is_maximal_fm -- which
    drops an array whose neighbour base continues its consensus -- keeps it."""
    B, tv = "ACGT", {"A": "C", "C": "A", "G": "T", "T": "G"}
    s = [B[i] for i in r.integers(0, 4, k)]
    if unit and s:
        s[-1] = tv.get(unit[-1], "A")
    if nxt and s:
        s[0] = tv.get(nxt[0], "A")
    return "".join(s)


def _crafted_subs(seed: int, subs: str, n_segments: int = 16) -> str:
    """_crafted_short with every substitution drawn from `subs`, behind a head of
    hand-made arrays of 8- and 9-base units (looked up / located directly, no
    padding needed) that put those bytes where the extension decides on them:
    the byte in one copy only -- the 2nd of 6, where it ties with the base when
    it is voted on (the smaller byte is the consensus), and the 4th of 7, where
    it is outvoted; a unit that holds the byte in every copy (the byte's own
    column); that unit with a base, or another of the bytes, there in one copy
    (the byte keeps the majority: whether the odd copy stays is decided by
    count_transversions_array's classes)."""
    r = np.random.default_rng(seed)
    out = ""
    for j, x in enumerate(subs):
        y = subs[(j + 1) % len(subs)]
        for u, cps, odd, z in (("CAGTCCTA", 6, 1, x), ("GATTCAGCA", 7, 3, x),
                               ("CT" + x + "GACTG", 6, -1, ""), ("GGC" + x + "TTACA", 6, -1, ""),
                               ("G" + x + "CTTACA", 7, 3, "ATCG"[j % 4]), ("TC" + x + "AGGTCA", 7, 2, "T"),
                               ("GT" + x + "CATCC", 7, 4, y if y != x else "C")):
            arr = [u] * cps
            if odd >= 0:
                q = 4 if x not in u else u.index(x)
                arr[odd] = u[:q] + z + u[q + 1:]
            out += _flank(r, 17 + 2 * j, u) + "".join(arr) + _flank(r, 1, "", u)
    trans = {"A": "G", "G": "A", "C": "T", "T": "C"}
    B = "ACGT"
    for _ in range(n_segments):
        k = int(r.choice([2, 3, 4, 5, 6, 7, 8, 8, 9, 9]))
        unit = "".join(B[i] for i in r.integers(0, 4, k))
        out += _flank(r, int(r.integers(10, 50)), unit)
        if r.random() < 0.6 and k < 8:
            out += "A" * (8 - k)
        arr = list(unit * int(r.integers(3, 14)))
        for q in range(len(arr)):
            v = r.random()
            if v < 0.03:
                arr[q] = subs[int(r.integers(0, len(subs)))]
            elif v < 0.05:
                arr[q] = trans[arr[q]]
        out += "".join(arr)
    return out


def _dense_unbinned(n: int = 9000, seed: int = 31) -> str:
    """'R' at every 4th base, so nearly every extension entry meets a byte
    outside A C G N T, plus three clean arrays (8- and 9-base units, and a
    3-base unit behind its A-padding), each between two 'R's."""
    r = np.random.default_rng(seed)
    B = "ACGT"
    s = ["R" if q % 4 == 3 else B[int(x)] for q, x in enumerate(r.integers(0, 4, n))]
    for pos, arr in [(1000, "CAGTTGCA" * 9), (4000, "GATCCTGAC" * 8), (7000, "AAAAA" + "CTG" * 14)]:
        s[pos:pos + len(arr)] = arr
        s[pos + len(arr)] = "R"
    return "".join(s)


def _library_edge_cases():
    """name -> dict(finder, seq, params, tier1_seen): the inputs of
    library_edges.json (the tests import this to build the same texts)."""
    r = np.random.default_rng(2024)
    B = "ACGT"

    def rnd(k):
        return "".join(B[i] for i in r.integers(0, 4, k))

    cases = {}

    def add(name, finder, seq, **params):
        cases[name] = dict(finder=finder, seq=seq, params=params, tier1_seen=[])

    # ---- short imperfect repeats
    add("si_subs_N", "short_imperfect", _crafted_subs(41, "N", 26))
    add("si_subs_NRY", "short_imperfect", _crafted_subs(42, "NRY", 14))
    add("si_subs_low_high", "short_imperfect", _crafted_subs(43, "*a", 20))   # below 'A', above 'T'
    u8, v8, u9, v9 = "ACGGTCAT", "TTCAGGCA", "GATCCTGAC", "CTTGACCAG"
    # arrays from text position 0 and up to the last base
    add("si_ends", "short_imperfect", u8 * 5 + _flank(r, 40, "T", u8) + "AAAA" + "CAGT" * 7 + _flank(r, 35, u9, "C")
        + u9 * 5)
    add("si_ends_b", "short_imperfect", v9 * 4 + _flank(r, 50, v8, v9) + v8 * 4)
    add("si_short8", "short_imperfect", "ACACACAC")
    add("si_short7", "short_imperfect", "ACGACGA")
    add("si_one", "short_imperfect", "A")
    # arrays across text positions 63/64 and 127/128: n (with the sentinel) just over 64 and 128
    add("si_n66", "short_imperfect", _flank(r, 41, u8) + u8 * 3)
    add("si_n67", "short_imperfect", _flank(r, 38, u9) + u9 * 3 + "T")
    add("si_n130", "short_imperfect", _flank(r, 50, u8) + u8 * 3 + _flank(r, 31, v8, u8) + v8 * 3)
    add("si_n131", "short_imperfect", _flank(r, 40, u9) + u9 * 3 + _flank(r, 36, v9, u9) + v9 * 3)
    add("si_dense_R", "short_imperfect", _dense_unbinned())

    # ---- simple period scan: the reference walks only the periods around the array's (it
    # needs 8 to 25 s per text for all of 1..200, too close to its 30 s stop)
    for p in SIMPLE_EDGE_PERIODS:
        for sub in (False, True):
            add(f"simple_p{p}_{'sub' if sub else 'exact'}", "simple",
                _period_text(p, sub, 4 if p <= 129 else 3, 40, SIMPLE_EDGE_SEEDS.get(p, 1000 + p)),
                min_period=p - 2, max_period=p + 2)
    for p in (65, 100):     # 1001..3000 bases: max_p = 100
        for sub in (False, True):
            add(f"simple_n1k_p{p}_{'sub' if sub else 'exact'}", "simple", _period_text(p, sub, 4, 400, 2000 + p),
                min_period=p - 2, max_period=p + 2)
    # two copies + 6/7 of one: accepted only through the partial copy (effective copies 3)
    u = rnd(70)
    add("simple_partial_p70", "simple", rnd(40) + u * 2 + u[:60] + rnd(40), min_period=66, max_period=74)
    u = rnd(60)
    for name, syms in (("simple_syms10", MANY_SYMBOLS), ("simple_syms6", MANY_SYMBOLS[:6])):
        arr = "".join(u[:5] + syms[c % len(syms)] + u[6:] for c in range(10))
        add(name, "simple", rnd(40) + arr + rnd(40), min_period=56, max_period=64)
    # arrays from position 0 and up to the last base, with partial copies cut by either end
    u, v, w = rnd(70), rnd(30), rnd(130)
    add("simple_ends", "simple", u * 3 + rnd(50) + v * 4 + v[:11], min_period=28, max_period=72)
    add("simple_ends_partial", "simple", u[-33:] + u * 3 + u[:41], min_period=66, max_period=74)
    add("simple_ends_p130", "simple", w[-50:] + w * 3 + w[:64], min_period=126, max_period=134)

    # ---- Tier 1
    unit9 = "ACGTTGCAG"
    for L in range(1, 10):
        for n in sorted({1, 2, L, 2 * L, 3 * L, 3 * L + 1}):
            add(f"t1_L{L}_n{n}", "tier1", (unit9[:L] * 4)[:n])
    add("t1_N_inside", "tier1", "ACGACGACG" + "N" + "ACGACGACGACG")
    add("t1_AN", "tier1", "GT" + "AN" * 8 + "TG")
    add("t1_A9", "tier1", "GT" + "A" * 9 + "TG")
    add("t1_A10", "tier1", "GT" + "A" * 10 + "TG")
    add("t1_AAC3", "tier1", "GT" + "AAC" * 3 + "TG")
    add("t1_AAC4", "tier1", "GT" + "AAC" * 4 + "TG")
    add("t1_at_end", "tier1", "GTCA" + "ACG" * 4)
    add("t1_iupac", "tier1", "ACRACRACRACR" + "GT" + "acgacgacgacg" + "CATCATCATCAT")

    # ---- LCP plateaus
    u20, w20 = rnd(20), rnd(20)
    add("pl_start", "lcp_plateaus", u20 * 6 + rnd(90))
    add("pl_middle", "lcp_plateaus", rnd(70) + u20 * 6 + rnd(70))
    add("pl_end", "lcp_plateaus", rnd(90) + u20 * 6)
    u5 = "CAGTT"
    add("pl_maxp5", "lcp_plateaus", rnd(50) + u5 * 12 + rnd(50), max_period=5)
    add("pl_maxp19", "lcp_plateaus", rnd(40) + rnd(19) * 6 + rnd(40) + u20 * 6, max_period=19)
    add("pl_minp21", "lcp_plateaus", rnd(40) + rnd(21) * 6 + rnd(40) + u20 * 6, min_period=21)
    add("pl_minp30", "lcp_plateaus", rnd(40) + rnd(28) * 3 + rnd(40), min_period=30)           # max LCP 56
    add("pl_minp30_no_runs", "lcp_plateaus", rnd(40) + u5 * 5 + rnd(40), min_period=30)        # max LCP < 30
    add("pl_two_arrays", "lcp_plateaus", rnd(30) + u20 * 4 + rnd(45) + w20 * 5 + rnd(30) + u20 * 4 + rnd(20))
    add("pl_all_A", "lcp_plateaus", "A" * 100)
    add("pl_n2", "lcp_plateaus", "A")
    for n in (255, 256, 257):                      # text bytes with the sentinel: the 256-thread block edge
        add(f"pl_n{n}", "lcp_plateaus", rnd(n - 1 - 80) + u20 * 4)
    return cases


def _run_library_edge(ref, name, case):
    """The reference's records of one case, or the exception's name if it raises."""
    seq, kw = case["seq"], case["params"]
    finder = case["finder"]
    core = ref.BWTCore(seq + "$", 32)
    with contextlib.redirect_stdout(io.StringIO()):
        if finder == "tier1":
            return ref.Tier1STRFinder(core.text_arr, 9, False).find_strs(name)
        f = ref.Tier2LCPFinder(core, **kw)
        seen = {tuple(x) for x in case["tier1_seen"]}
        if finder == "short_imperfect":
            return f.find_short_imperfect_repeats(name, seen)
        if finder == "lcp_plateaus":
            return f._detect_lcp_plateaus(f._compute_lcp_array(), name)
        return f.find_long_repeats(name, seen)


def cmd_library_edges(a):
    """The library finders on the input families the other goldens leave out
    (N / IUPAC / other bytes in short imperfect arrays, a side list past its
    first capacity, periods 63..200 of the simple scan, columns of up to 10
    symbols, arrays at either end of the text, tiny Tier 1 texts, plateau
    thresholds other than 20) -> library_edges.json.  Each case names the one
    finder it targets.  `seconds` is rounded up to whole seconds, so a quiet
    machine regenerates the file byte for byte; simple-scan cases must stay far
    below the reference's 30 s wall-clock stop (asserted at 10 s)."""
    import math
    ref = ref_module()
    out = {}
    for name, case in _library_edge_cases().items():
        t0 = time.time()
        try:
            recs = [_rec_json(r) for r in _run_library_edge(ref, name, case)]
            if case["finder"] == "lcp_plateaus":   # the fields a plateau record sets; the rest are defaults
                recs = [{k: d[k] for k in PLATEAU_KEYS} for d in recs]
            err = None
        except Exception as e:           # recorded: neither side is called on this input
            recs, err = [], type(e).__name__
        dt = time.time() - t0
        if case["finder"] == "simple":
            assert dt < 10.0, f"{name}: {dt:.1f} s -- too close to the reference's 30 s stop"
        out[name] = dict(case, records=recs, raises=err, seconds=int(math.ceil(dt)))
        print(name, len(case["seq"]), len(recs), err, round(dt, 1), flush=True)
    with open(os.path.join(HERE, "library_edges.json"), "w") as f:
        json.dump(out, f, indent=0)


# ------------------------------------------------------------ edge inputs
def _edge_inputs():
    """Input edge cases of SURVEY.md §7.3: natural-key
    collisions (chr1 / chr01 / CHR1, chr2 / Chr02) inside one fold unit with
    different trims, CRLF and bare-CR line ends, a '$' inside and at the end of
    a sequence, contigs of 0-62 bp around the 2 x 30 bp trim, and non-ASCII
    text (valid UTF-8 'é', and an invalid byte)."""
    r = np.random.default_rng(11)
    B = "ACGT"

    def rnd(n):
        return "".join(B[i] for i in r.integers(0, 4, n))

    def body(n, arrays):
        s = rnd(n)
        for pos, unit, cps in arrays:
            arr = unit * cps
            s = s[:pos] + arr + s[pos + len(arr):]
        return s[:n]

    def lines(seq, w=60, eol="\n"):
        return "".join(seq[i:i + w] + eol for i in range(0, len(seq), w))

    files = {}
    c1 = body(260, [(40, "CAG", 8), (100, "A", 9), (130, "GT", 7), (200, "ACGTT", 4)])
    c01 = body(50, [(5, "TG", 6), (25, "C", 7)])
    C1 = body(150, [(35, "GATA", 5), (90, "TTAGG", 4)])
    c2 = body(100, [(40, "AC", 10)])
    C02 = body(70, [(32, "G", 8)])
    files["edge_collide.fa"] = (">chr1 first copy\r\n" + lines(c1, 60, "\r\n") + ">chr01\n" + lines(c01) +
                                ">CHR1\r" + lines(C1, 70, "\r") + ">chr2\n" + lines(c2) + ">Chr02 x\n" +
                                lines(C02.lower(), 35))
    d1 = body(180, [(40, "CA", 8)])
    d1 = d1[:70] + "$$$" + d1[73:120] + "AC$AC$AC$AC$" + d1[132:]
    d2 = body(90, [(20, "T", 10)]) + "$"
    files["edge_dollar.fa"] = ">withdollar\n" + lines(d1) + ">enddollar\n" + lines(d2)
    parts = []
    for k, n in enumerate([0, 1, 6, 59, 60, 61, 62, 64]):
        seq = body(n, [(max(0, n // 2 - 6), "A", 6)] if n >= 12 else [])
        parts.append(f">short{k}  \t\n\n" + lines(seq, 25))
    files["edge_short.fa"] = "".join(parts)
    u = body(140, [(30, "CT", 9), (80, "A", 8)])
    files["edge_utf8.fa"] = ">u1\n" + u[:50] + "é" + u[50:] + "\n>u2\n" + lines(body(100, [(10, "GA", 8)]))
    return files


def cmd_edge(a):
    """Reference CLI on the edge inputs -> expected_edge.json (+ *.out)."""
    ref = ref_module()
    inp = os.path.join(HERE, "inputs")
    out_dir = os.path.join(HERE, "cli")
    work = tempfile.mkdtemp()
    man = {}
    files = _edge_inputs()
    for fn, text in files.items():
        with open(os.path.join(inp, fn), "w", newline="", encoding="utf-8") as f:
            f.write(text)
    with open(os.path.join(inp, "edge_badbyte.fa"), "wb") as f:
        f.write(b">bad\nACGTACGTACGT\xffACGTACGTACGTACGT\n")
    cases = []
    for fn in files:
        cases += [(f"{fn}.strfinder", fn, []), (f"{fn}.bed", fn, ["--format", "bed"]),
                  (f"{fn}.trim0", fn, ["--flank-trim", "0"])]
    cases.append(("edge_badbyte.fa.strfinder", "edge_badbyte.fa", []))
    for name, fn, args in cases:
        shutil.copy(os.path.join(inp, fn), os.path.join(work, fn))
        outp = os.path.join(work, "out.tab")
        if os.path.exists(outp):
            os.unlink(outp)
        err = None
        try:
            run_ref_cli(ref, [fn, "-o", "out.tab", "--jobs", "-1"] + args, work)
        except Exception as e:        # the reference's own failure is the golden
            err = f"{type(e).__name__}: {e}"
        rec = dict(input=fn, args=args)
        if err is None:
            dst = os.path.join(out_dir, name + ".out")
            shutil.copy(outp, dst)
            rec["sha256"] = sha(dst)
        else:
            rec["error"] = err
        man[name] = rec
        print(name, rec.get("sha256", rec.get("error"))[:60], flush=True)
    with open(os.path.join(HERE, "expected_edge.json"), "w") as f:
        json.dump(man, f, indent=1, sort_keys=True)


def cmd_homopolymer(a):
    """The reference's align_repeat_region on the long one-base cases, as
    fixtures (tests/golden/homopolymer_long.json: the case and the reference's
    copies / consumed length, or null), and the closed form checked on them."""
    ref = ref_module()
    orig, fast = _homopolymer_align(ref)
    t0 = time.time()
    out = []
    for c in _long_homopolymer_cases():
        seq = c["left"] + c["base"] * c["run"] + c["right"]
        r = orig(seq, c["start"], c["end"], c["base"], mismatch_fraction=c["mismatch_fraction"],
                 min_copies=c["min_copies"])
        rec = dict(c)
        rec["want"] = None if r is None else dict(copies=r.copies, consumed=r.consumed_length,
                                                   consensus=r.consensus, mismatch_rate=r.mismatch_rate,
                                                   max_errors=r.max_errors_per_copy,
                                                   ins=r.total_insertions, dels=r.total_deletions,
                                                   variations=list(r.variations))
        out.append(rec)
    _check_homopolymer_align_long(ref, orig, fast)
    with open(os.path.join(HERE, "homopolymer_long.json"), "w") as f:
        json.dump(dict(seconds=round(time.time() - t0, 1), cases=out), f, indent=0)
    print(len(out), "cases", round(time.time() - t0, 1), "s")


def cmd_hybrid(a):
    """Full-size golden via the validated hybrid oracle (--pure: the reference
    itself, nothing swapped)."""
    ref = ref_module()
    from bwtmi import synth
    cfg = synth.CONFIGS.get(a.config) if a.config else None
    lengths = cfg["lengths"] if cfg else [int(x) for x in a.lengths.split(",")]
    sub = cfg["sub_rate"] if cfg else a.sub_rate
    gaps = cfg.get("gaps") if cfg else a.gaps
    first = cfg.get("first_index", 1) if cfg else a.first_index
    if not a.pure:
        install_hybrid(ref, stub_index=True, restate_nested=True, homopolymer=bool(gaps) or a.homopolymer)
    work = a.work or tempfile.mkdtemp()
    fa = os.path.join(work, f"{a.name}.fa")
    t0 = time.time()
    fa_sha = synth.write_fasta(fa, lengths, sub, first, gaps)
    args = [os.path.basename(fa), "-o", "out.tab", "--jobs", str(a.jobs)] + a.extra.split()
    run_ref_cli(ref, args, work)
    outp = os.path.join(work, "out.tab")
    with open(outp, "rb") as f:
        data = f.read()
    rec = dict(config=a.config, lengths=lengths, sub_rate=sub, args=a.extra.split(),
               gaps=gaps, first_index=first, pure_reference=bool(a.pure),
               homopolymer_closed_form=(bool(gaps) or a.homopolymer) and not a.pure,
               fasta_sha256=fa_sha, out_sha256=hashlib.sha256(data).hexdigest(),
               out_rows=data.count(b"\n") - 1, seconds=round(time.time() - t0, 1))
    if a.keep_rows:
        lines = data.decode().splitlines()
        step = max(1, (len(lines) - 1) // a.keep_rows)
        rec["sample"] = {str(i): lines[i] for i in range(1, len(lines), step)}
    if a.save_out:
        shutil.copy(outp, os.path.join(HERE, "cli", f"{a.name}.out"))
    path = os.path.join(HERE, "expected_large.json")
    allr = json.load(open(path)) if os.path.exists(path) else {}
    allr[a.name] = rec
    with open(path, "w") as f:
        json.dump(allr, f, indent=1, sort_keys=True)
    print(json.dumps({k: v for k, v in rec.items() if k != "sample"}))


def main():
    ap = argparse.ArgumentParser()
    sp = ap.add_subparsers(dest="cmd", required=True)
    p = sp.add_parser("fixtures"); p.add_argument("--check-hybrid", action="store_true")
    sp.add_parser("rawhits")
    sp.add_parser("index")
    sp.add_parser("index_rates")
    sp.add_parser("motif")
    sp.add_parser("library")
    sp.add_parser("library_edges")
    sp.add_parser("tier3")
    sp.add_parser("simple")
    sp.add_parser("edge")
    sp.add_parser("homopolymer")
    p = sp.add_parser("hybrid")
    p.add_argument("name")
    p.add_argument("--config")
    p.add_argument("--lengths", default="100000")
    p.add_argument("--sub-rate", type=float, default=0.0)
    p.add_argument("--gaps", default=None, help="bwtmi.synth GAP_PROFILES name")
    p.add_argument("--first-index", type=int, default=1)
    p.add_argument("--homopolymer", action="store_true", help="validated one-base align closed form")
    p.add_argument("--pure", action="store_true", help="the reference itself, nothing swapped")
    p.add_argument("--extra", default="")
    p.add_argument("--jobs", type=int, default=-1)
    p.add_argument("--work")
    p.add_argument("--keep-rows", type=int, default=0)
    p.add_argument("--save-out", action="store_true")
    a = ap.parse_args()
    dict(fixtures=cmd_fixtures, rawhits=cmd_rawhits, index=cmd_index, index_rates=cmd_index_rates, motif=cmd_motif,
         hybrid=cmd_hybrid, homopolymer=cmd_homopolymer, library=cmd_library, library_edges=cmd_library_edges, tier3=cmd_tier3, simple=cmd_simple, edge=cmd_edge)[a.cmd](a)


if __name__ == "__main__":
    main()
