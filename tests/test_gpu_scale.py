"""Device tests at the benched sizes and on the multi-GPU plumbing:

* the >50 Mbp Tier-2 gate of the worker (bwt.py:3068-3072) at its boundary;
* the FM index of a C3-size (100 Mbp) contig through size-independent
  properties (bwt.py:138-333: SA, BWT, C/Occ, sampled SA, 8-mer hash) and
  backward search (bwt.py:359-389) for every canonical motif of 1..10 bp
  against k-mer counts taken straight from the text;
* the RCCL transport (csrc/comm.cpp) on one rank: typed all-reduces and the
  sharded writer going through it;
* a device fault fails the run instead of being reported per contig;
* the CLI's deferred parent indices (bwt.py:3758-3790) build on first use.
Integer work: every comparison is exact."""
import hashlib
import os

import numpy as np
import pytest

import oracle
from oracle import post

pytestmark = pytest.mark.gpu

HEADER_SHA = "02f1e37be1d898b12b48ab0c380fad02c0bd48aaebb8300fe8cd68fe35752b3b"


def _cli_sha(fa, out, args):
    from bwtmi import cli
    assert cli.main([str(fa), "-o", str(out), "--jobs", "-1"] + list(args)) == 0
    data = out.read_bytes()
    return hashlib.sha256(data).hexdigest(), data.count(b"\n") - 1


def test_tier2_gate_boundary_50mbp(gpu_ctx, tmp_path):
    """Trimmed length 50,000,000 is analysed with default parameters (the
    output equals the --progress run, which only changes stdout below the
    gate); 50,000,001 skips Tier 2: header-only, while --progress still
    analyses it."""
    from bwtmi import synth
    body = synth.generate_contig(50_000_061, 61)
    for n, gated in ((50_000_060, False), (50_000_061, True)):
        fa = tmp_path / f"b{n}.fa"
        fa.write_bytes(synth.format_fasta_record("contig1", body[:n]))
        d_sha, d_rows = _cli_sha(fa, tmp_path / "d.tab", [])
        p_sha, p_rows = _cli_sha(fa, tmp_path / "p.tab", ["--progress"])
        assert p_rows > 100_000, n
        if gated:
            assert (d_sha, d_rows) == (HEADER_SHA, 0), n
        else:
            assert (d_sha, d_rows) == (p_sha, p_rows), n
        fa.unlink()


def _rolling_counts(t2: np.ndarray, k: int, bad: np.ndarray = None) -> np.ndarray:
    """Occurrences of every k-mer (2-bit code, A<C<G<T) in an ACGT array;
    windows holding a position flagged in `bad` (a non-ACGT byte) are not
    counted."""
    m = t2.size - k + 1
    code = np.zeros(m, dtype=np.uint32)
    for j in range(k):
        code = (code << np.uint32(2)) | t2[j:j + m]
    if bad is not None:
        cb = np.concatenate(([0], np.cumsum(bad, dtype=np.int64)))
        code = code[(cb[k:] - cb[:m]) == 0]
    return np.bincount(code, minlength=4 ** k)


def _kmer_table(t: np.ndarray, k: int = 8):
    """The reference's 8-mer table (bwt.py:138-171) restated over arrays: bytes
    outside ACGTN (either case) are skipped without resetting the rolling
    window, N counts as A, the window starts at 0 (so the first k-1 valid bases
    of the text see zero-padded codes), and every valid base at i >= k appends
    position i-k+1; position 0 only when the first k bytes are all valid.
    Returns (code, position) of every entry in append order."""
    lut = np.full(256, 255, dtype=np.uint8)
    for ch, v in zip(b"ACGTNacgtn", (0, 1, 2, 3, 0, 0, 1, 2, 3, 0)):
        lut[ch] = v
    c = lut[t]
    vpos = np.flatnonzero(c != 255)
    vc = c[vpos].astype(np.uint32)
    w = np.zeros(vc.size, dtype=np.uint32)
    for j in range(k):      # w[i] = codes of valid bases i-k+1..i, zero before the first
        sh = np.zeros(vc.size, dtype=np.uint32)
        if j < vc.size:
            sh[j:] = vc[:vc.size - j]
        w |= sh << np.uint32(2 * j)
    keep = vpos >= k
    code, pos = w[keep], (vpos[keep] - (k - 1)).astype(np.int64)
    if t.size >= k and (c[:k] != 255).all():
        code = np.concatenate(([w[k - 1]], code))
        pos = np.concatenate(([0], pos))
    return code, pos


def _check_index_properties(text: bytes, rng_seed: int = 1):
    """SA a permutation with the sentinel first, sampled adjacent suffixes
    ascend (raw byte order, '$' smallest), BWT = t[SA-1], C/Occ totals, sampled
    SA = SA[::32], the 8-mer CSR equal to the reference's table (bucket sizes
    and every bucket's positions), and backward search of all 145,338
    canonical motifs of 1..10 bp giving intervals whose widths are the motifs'
    occurrence counts and whose SA rows are occurrences."""
    from bwtmi import BWTCore, MotifUtils
    n = len(text)
    core = BWTCore(text)
    sa = core.suffix_array
    assert sa.size == n and sa[0] == n - 1
    seen = np.zeros(n, dtype=bool)
    seen[sa] = True
    assert seen.all()
    del seen
    r = np.random.default_rng(rng_seed)
    for k in r.integers(1, n, 4000).tolist():
        a, b = int(sa[k - 1]), int(sa[k])
        w = 4096
        while text[a:a + w] == text[b:b + w]:
            w *= 2
        assert text[a:a + w] < text[b:b + w], k
    t = np.frombuffer(text, dtype=np.uint8)
    bwt = core.bwt_arr
    assert np.array_equal(bwt, t[(sa.astype(np.int64) - 1) % n])
    del bwt
    occ = core.occ_checkpoints
    cnt = np.bincount(t, minlength=256)
    present = np.flatnonzero(cnt).tolist()
    assert sorted(occ) == present
    for c in present:
        assert occ[c][-1] == cnt[c] and core.char_totals[chr(c)] == cnt[c]
        assert core.char_counts[chr(c)] == int(cnt[:c].sum())
    samp = core.sampled_sa
    assert len(samp) == (n + 31) // 32
    for i in r.integers(0, len(samp), 20000).tolist():
        assert samp[i * 32] == int(sa[i * 32])
    del samp
    off, pos = core.kmer_csr()
    code, kpos = _kmer_table(t)
    order = np.argsort(code.astype(np.uint16), kind="stable")
    assert np.array_equal(np.diff(off), np.bincount(code, minlength=65536)) and off[-1] == code.size
    assert np.array_equal(pos, kpos[order])
    del off, pos, code, kpos, order
    bad = ~np.isin(t[:-1], np.frombuffer(b"ACGT", dtype=np.uint8))
    t2 = np.searchsorted(np.frombuffer(b"ACGT", dtype=np.uint8), t[:-1]).astype(np.uint32) & np.uint32(3)
    anybad = bool(bad.any())
    pats = [mt for k in range(1, 11) for mt in MotifUtils.enumerate_motifs(k)]
    assert len(pats) == 145338
    got = core.backward_search_batch(pats)
    width = np.where(got[:, 0] >= 0, got[:, 1] - got[:, 0] + 1, 0)
    lut = {ord("A"): 0, ord("C"): 1, ord("G"): 2, ord("T"): 3}
    start = 0
    for k in range(1, 11):
        ck = _rolling_counts(t2, k, bad if anybad else None)
        ks = [p for p in pats[start:] if len(p) == k]
        codes = np.array([sum(lut[ord(ch)] << (2 * (k - 1 - j)) for j, ch in enumerate(p)) for p in ks],
                         dtype=np.int64)
        assert np.array_equal(width[start:start + len(ks)], ck[codes]), k
        start += len(ks)
    for i in r.integers(0, len(pats), 300).tolist():   # the interval's rows are occurrences
        sp, ep = got[i].tolist()
        if sp < 0:
            continue
        p = pats[i].encode()
        for row in range(sp, min(ep + 1, sp + 5)):
            s = int(sa[row])
            assert text[s:s + len(p)] == p, pats[i]


def test_index_100mbp_properties(gpu_ctx):
    """C3's contig (100 Mbp after the trim, ACGT: the DNA suffix sort and the
    packed-rank search) through _check_index_properties."""
    from bwtmi import synth
    seq = synth.generate_contig(100_000_000, 1)          # C3's contig1
    _check_index_properties(seq[30:len(seq) - 30] + b"$")


def test_index_100mbp_properties_with_gaps(gpu_ctx):
    """C3N's contig: C3 with assembly gaps (3.8 % N in runs of 10 bp - 958
    kbp, ~1e4 single R/Y; bwtmi.synth GAP_PROFILES "n2").  Non-ACGT text takes
    the general prefix-doubling suffix sort (ASCII order: N between G and T,
    bwt.py:212-264), the byte Occ search and the general 8-mer table (N -> A,
    R/Y skipped, bwt.py:138-171); a 958 kbp N run needs ~16 doubling rounds."""
    from bwtmi import synth
    seq = synth.generate_contig(100_000_000, 1, gaps="n2")   # C3N's contig1
    _check_index_properties(seq[30:len(seq) - 30] + b"$", rng_seed=2)


def test_cli_self_launched_ranks_match_one_process(gpu_ctx, tmp_path):
    """`bwt.py IN.fa --jobs 2` without a launcher starts two rank processes of
    the CLI (rehearsed on one GPU: BWTMI_CLI_RANKS=2, host transport, both on
    device 0) that shard the contigs and write the shared file: byte-equal to
    the one-process output in all five formats (bwt.py:3850-3912, 4141-4198)."""
    import subprocess
    import sys
    from bwtmi import cli, synth
    fa = tmp_path / "multi.fa"
    synth.write_fasta(str(fa), [300_000, 120_000, 250_000, 80_000, 200_000], 0.02, first_index=40, gaps="n1")
    script = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bwt-algorithm_amd", "bwt.py")
    for fmt in ("strfinder", "bed", "vcf", "trf_table", "trf_dat"):
        one, many = tmp_path / f"one.{fmt}", tmp_path / f"many.{fmt}"
        os.environ["BWTMI_CLI_LAUNCH"] = "0"
        try:
            assert cli.main([str(fa), "-o", str(one), "--format", fmt, "--jobs", "2"]) == 0
        finally:
            del os.environ["BWTMI_CLI_LAUNCH"]
        env = dict(os.environ, BWTMI_CLI_RANKS="2")
        r = subprocess.run([sys.executable, script, str(fa), "-o", str(many), "--format", fmt, "--jobs", "2"],
                           env=env, capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stderr[-2000:]
        assert "Completed! Found" in r.stdout
        assert many.read_bytes() == one.read_bytes(), fmt
        assert one.read_bytes().count(b"\n") > 100, fmt


def test_cli_eight_self_launched_ranks_match_c4_golden(gpu_ctx, golden_dir, tmp_path):
    """C4 (8 x 12.5 Mbp, BASELINE configs[3]) through `bwt.py C4.fa --jobs 8`
    with 8 self-launched ranks (rehearsed on one GPU: BWTMI_CLI_RANKS=8, host
    transport): each rank loads its share of the file (split loader), scans,
    post-processes and writes its rows into the shared file; the file must
    equal the C4 golden of the reference pipeline (bwt.py:3850-3912)."""
    import hashlib
    import json
    import subprocess
    import sys
    from bwtmi import synth
    with open(os.path.join(golden_dir, "expected_large.json")) as f:
        g = json.load(f)["C4"]
    fa = str(tmp_path / "C4.fa")
    assert synth.write_fasta(fa, g["lengths"], g["sub_rate"], g.get("first_index", 1), g.get("gaps")) == \
        g["fasta_sha256"]
    out = tmp_path / "C4.tab"
    script = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bwt-algorithm_amd", "bwt.py")
    env = dict(os.environ, BWTMI_CLI_RANKS="8")
    r = subprocess.run([sys.executable, script, fa, "-o", str(out), "--jobs", "8"] + list(g["args"]),
                       env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    data = out.read_bytes()
    assert data.count(b"\n") - 1 == g["out_rows"]
    assert hashlib.sha256(data).hexdigest() == g["out_sha256"]


def test_scan_and_index_lanes_switches(gpu_ctx):
    """A multi-contig job's strict scans and background index builds on 1 lane
    (BWTMI_SCAN_LANES=1, BWTMI_INDEX_LANES=1), 8, or 3 and 2: the same records."""
    from bwtmi import _lib, synth
    from bwtmi.records import Job
    seqs = [synth.generate_contig(150_000 + 40_000 * i, 70 + i, 0.02, gaps="n1" if i % 3 == 0 else None)
            for i in range(7)]

    def run():
        j = Job(min_copies=3, show_progress=True, build_index=True, threads=8)
        for i, s in enumerate(seqs):
            j.add_contig(f"chr{i + 1}", s, 30, 30)
        j.scan(gpu_ctx)
        j.postprocess()
        j.wait(gpu_ctx)
        return j.render("strfinder")
    want = run()
    assert want.count(b"\n") > 1000
    for kv in ({"SCAN_LANES": 1, "INDEX_LANES": 1}, {"SCAN_LANES": 8, "INDEX_LANES": 8},
               {"SCAN_LANES": 3, "INDEX_LANES": 2}):   # uneven lanes, another count at each site
        with _lib.knobs(**kv):
            assert run() == want, kv


def test_bind_host_moves_and_restores_affinity(gpu_ctx):
    """bwtmi_bind_host: host work onto the GPU's NUMA node (a subset of that
    node's CPUs; with BWTMI_NUMA_SMT=1 the node's allowed CPUs), and back."""
    from bwtmi import _lib
    before = os.sched_getaffinity(0)
    for smt in (0, 1):
        with _lib.knobs(NUMA_SMT=smt):
            changed = _lib.bind_host(gpu_ctx)
            now = os.sched_getaffinity(0)
            if changed:
                assert now < before, (smt, sorted(now)[:8])
            else:
                assert now == before
            _lib.bind_host(gpu_ctx, False)
            assert os.sched_getaffinity(0) == before


def test_cli_profile_json(gpu_ctx, golden_dir, tmp_path):
    """`bwt.py IN.fa --profile P.json`: wall ms, calls and bytes of every stage
    the CLI runs (load, scan, postprocess, write, index_wait) and the library's
    own split (scan, index, merge, refine..filter, render); the output file is
    the golden one."""
    import json
    from bwtmi import cli
    with open(os.path.join(golden_dir, "expected_cli.json")) as f:
        want = json.load(f)["synthetic_test.fa.strfinder"]["sha256"]
    out, prof = tmp_path / "o.tab", tmp_path / "p.json"
    fa = os.path.join(golden_dir, "inputs", "synthetic_test.fa")
    assert cli.main([fa, "-o", str(out), "--format", "strfinder", "--profile", str(prof)]) == 0
    import hashlib
    assert hashlib.sha256(out.read_bytes()).hexdigest() == want
    d = json.loads(prof.read_text())
    assert set(d["stages"]) >= {"load", "scan", "postprocess", "write", "index_wait"}
    assert d["stages"]["load"]["bytes"] == os.path.getsize(fa)
    assert d["stages"]["write"]["bytes"] == out.stat().st_size
    assert set(d["library_stage_ms"]) >= {"scan", "index", "merge", "refine..filter", "render"}
    assert d["records"] > 0 and d["bases"] > 0


def test_ktrace_records_every_launch(gpu_ctx, tmp_path):
    """BWTMI_KTRACE=path: one line per kernel launch (name, ms, idle ms) and a
    marker per resolved batch, appended to the file."""
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import numpy as np\n"
            "from bwtmi import synth\n"
            "from bwtmi.tiers import strict_scan_hits\n"
            "print(len(strict_scan_hits(np.frombuffer(synth.generate_contig(200000, 3), dtype=np.uint8), 1, 1000, 3)))\n"
            % (repo, os.path.join(repo, "bwt-algorithm_amd")))
    trace = tmp_path / "k.txt"
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, BWTMI_KTRACE=str(trace)),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = trace.read_text().splitlines()
    names = [ln.split()[0] for ln in lines if not ln.startswith("--")]
    assert "k_runs" in names and any(x.startswith("radix_hist") for x in names) and any(ln.startswith("-- resolve") for ln in lines)
    assert all(len(ln.split()) == 3 for ln in lines if not ln.startswith("--"))


def test_rccl_one_rank_collectives_and_sharded_write(gpu_ctx, golden_dir, tmp_path):
    """The RCCL transport on one rank (ncclCommInitRank with nranks = 1):
    int64 SUM / MAX with negative values and float64 MAX come back exactly,
    and the sharded writer run through it writes the single-process file in
    every format.  (One rank cannot tell a signed from an unsigned reduction;
    the types now come from rccl.h itself.)"""
    from bwtmi import _lib, comm, dist
    from bwtmi.records import Job
    c = comm.RcclComm(comm.Rendezvous(1, 0), 0)
    try:
        a = np.array([-7, 3, -(1 << 40), 0, (1 << 62)], dtype=np.int64)
        assert np.array_equal(c.allreduce(a, comm.SUM), a)
        assert np.array_equal(c.allreduce(a, comm.MAX), a)
        f = np.array([-1.5, 2.25, -1e300, 0.0], dtype=np.float64)
        assert np.array_equal(c.allreduce(f, comm.MAX), f)
        assert np.array_equal(c.allreduce(f, comm.SUM), f)
        words = comm.allgather_words(c, np.arange(-3, 9, dtype=np.int64))
        assert len(words) == 1 and words[0].tolist() == list(range(-3, 9))
        assert comm.allgather_bytes(c, b"xyz\x00\xff") == [b"xyz\x00\xff"]
        fa = os.path.join(golden_dir, "inputs", "test_all_12.fa")
        j = Job(min_copies=3)
        j.load_fasta(fa, 30)
        j.select_shard(1, 0)
        j.scan(_lib.ctx(0))
        j.postprocess()
        for fmt in ("strfinder", "bed", "vcf", "trf_table", "trf_dat"):
            out = tmp_path / f"{fmt}.out"
            dist.write_sharded(c, j, fmt, str(out))
            assert out.read_bytes() == j.render(fmt), fmt
            assert out.read_text() == post.run_file(fa, fmt), fmt
    finally:
        c.close()


def test_device_fault_fails_the_run(gpu_ctx, golden_dir, tmp_path, monkeypatch):
    """A BWTMI_E_HIP error inside a contig's scan is not the worker's per-contig
    `except Exception` (bwt.py:3137-3141): the CLI raises and writes nothing."""
    from bwtmi import _lib, cli
    fa = os.path.join(golden_dir, "inputs", "test2.fa")
    seqs, _, _ = post.load_fasta(fa, 30)
    monkeypatch.setenv("BWTMI_FAIL_CONTIG", sorted(seqs)[2])
    monkeypatch.setenv("BWTMI_FAIL_KIND", "hip")
    out = tmp_path / "out.tab"
    with pytest.raises(_lib.BwtmiError, match="injected failure"):
        cli.main([fa, "-o", str(out), "--jobs", "0"])
    assert not out.exists()


def test_cli_deferred_indices_build_on_use(gpu_ctx, golden_dir):
    """build_indices over the finder's own sequences: each contig's index is
    built on first use and equals BWTCore(seq + '$') (oracle arrays)."""
    from bwtmi import TandemRepeatFinder
    f = TandemRepeatFinder(os.path.join(golden_dir, "inputs", "test2.fa"))
    seqs = f.load_reference()
    f.build_indices(seqs)
    for name in list(seqs)[:4]:
        core = f.bwt_cores[name]
        ref = oracle.Index(seqs[name].encode() + b"$")
        assert (core.suffix_array == ref.sa).all() and (core.bwt_arr == ref.bwt).all(), name
        assert core.backward_search("AC") == ref.backward_search(b"AC")
        assert core.text == seqs[name] + "$"
    # a caller's override (and a new name) is what the deferred index is built over
    names = list(seqs)
    seqs[names[0]] = "ACGTACGTTTGACCA" * 7
    seqs["extra"] = "GATTACA" * 9
    f.build_indices(seqs)
    for name in (names[0], "extra"):
        core = f.bwt_cores[name]
        ref = oracle.Index(seqs[name].encode() + b"$")
        assert (core.suffix_array == ref.sa).all() and core.text == seqs[name] + "$", name
