"""CPU tests of the product's host side: the C ABI loads and exports every
declared symbol, and the native loader / post-processing / writers /
multi-rank gather reproduce the reference bytes when fed checker hits.
No device call is made here (the GPU tests are in test_gpu_*.py)."""
import hashlib
import json
import os
import re
import socket

import numpy as np
import pytest

import oracle
from oracle import post


def _header_symbols():
    hdr = os.path.join(os.path.dirname(__file__), "..", "include", "bwtmi.h")
    text = open(hdr).read()
    return sorted(set(re.findall(r"\b(bwtmi_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol(built_lib):
    from bwtmi import _lib
    declared = _header_symbols()
    assert len(declared) >= 40
    for name in declared:
        assert hasattr(built_lib, name), name
    assert set(declared) == set(_lib.EXPORTED)


def test_open_without_device_fails_loudly(built_lib):
    from bwtmi import _lib
    if _lib.device_count() > 0:
        pytest.skip("a device is present")
    with pytest.raises(_lib.BwtmiError, match="no CPU fallback"):
        _lib.ctx(0)


def _cases(golden_dir):
    with open(os.path.join(golden_dir, "expected_cli.json")) as f:
        man = json.load(f)
    for name, m in sorted(man.items()):
        d = dict(fmt="strfinder", mc=3, trim=30, tier2=True)
        a = m["args"]
        for i, x in enumerate(a):
            if x == "--format":
                d["fmt"] = a[i + 1]
            elif x == "--min-copies":
                d["mc"] = int(a[i + 1])
            elif x == "--flank-trim":
                d["trim"] = int(a[i + 1])
            elif x == "--tier1":
                d["tier2"] = False
        yield name, m, d


def _native_job(path, d):
    from bwtmi.records import Job
    j = Job(min_copies=d["mc"], tier2=d["tier2"])
    j.load_fasta(path, d["trim"])
    for cid in range(j.contig_count()):
        _, fl, tl, tr = j.contig_info(cid)
        if not d["tier2"]:
            continue
        seq = j.contig_seq(cid)[tl:fl - tr]
        U = max(120, min(len(seq) // d["mc"], 1000))
        j.add_hits(cid, oracle.strict_scan(seq, 1, U, 0, d["mc"]))
    return j


def test_native_loader_matches_reference_loader(golden_dir):
    for name, m, d in _cases(golden_dir):
        path = os.path.join(golden_dir, "inputs", m["input"])
        seqs, full, offs = post.load_fasta(path, d["trim"])
        from bwtmi.records import Job
        j = Job()
        j.load_fasta(path, d["trim"])
        assert j.names == list(seqs), name
        for cid, nm in enumerate(j.names):
            _, fl, tl, tr = j.contig_info(cid)
            assert j.contig_seq(cid).decode() == full[nm]
            assert tl == offs[nm] and j.contig_seq(cid)[tl:fl - tr].decode() == seqs[nm]


def _messy_fasta(seed: int) -> bytes:
    """A multi-MB FASTA whose lines end in \\n, \\r\\n or \\r, with blank and
    whitespace-padded lines, lower case, text before the first header, repeated
    names, empty contigs and lines far longer than one loader chunk."""
    r = np.random.default_rng(seed)
    eols = [b"\n", b"\r\n", b"\r"]
    out = bytearray(b"acgt orphan line before any header\n\n")
    names = [f"chr{k}".encode() for k in range(12)] + [b"chr3", b"scaffold_7", b"chr3"]
    for i, nm in enumerate(names):
        out += b"  >" + nm + b" description " + str(i).encode() + eols[int(r.integers(3))]
        if i % 7 == 5:
            continue                                           # empty contig
        total = int(r.integers(1, 600_000))
        width = int(r.choice([60, 61, 80, 1, 3_000_000]))
        seq = bytes(b"ACGTNacgtn"[k] for k in r.integers(0, 10, total))
        for a in range(0, total, width):
            pad = b" \t" if r.random() < 0.05 else b""
            out += pad + seq[a:a + width] + pad + eols[int(r.integers(3))]
            if r.random() < 0.02:
                out += b"   " + eols[int(r.integers(3))]
    return bytes(out)


def _plain_tail_fasta(seed: int) -> bytes:
    """Headers followed by long LF-only stretches (the loader's plain tails
    after a chunk's last '>' line), next to CRLF / lone-CR / padded contigs,
    a '>' inside a sequence line, lower case and N."""
    r = np.random.default_rng(seed)
    out = bytearray(b"orphan\n")
    for i in range(16):
        eol = [b"\n", b"\r\n", b"\r", b"\n"][i % 4]
        out += b">c" + str(i).encode() + b" x" + eol
        total = int(r.integers(1, 1_200_000))
        width = int(r.choice([60, 1, 13, 900_000]))
        seq = bytes(b"ACGTacgtNn"[k] for k in r.integers(0, 10, total))
        for a in range(0, total, width):
            out += seq[a:a + width] + (b"\n" if i % 4 != 1 else eol)
        if i == 6:
            out += b"AC>GT\n" + seq[:5000] + b"\n"
    return bytes(out)


@pytest.mark.parametrize("threads", [1, 4, 16])
def test_loader_plain_tails(tmp_path, threads):
    from bwtmi.records import Job
    path = str(tmp_path / "tails.fa")
    with open(path, "wb") as f:
        f.write(_plain_tail_fasta(threads))
    seqs, full, offs = post.load_fasta(path, 30)
    j = Job(threads=threads)
    j.load_fasta(path, 30)
    assert j.names == list(seqs)
    for cid, nm in enumerate(j.names):
        assert j.contig_seq(cid).decode() == full[nm], nm


@pytest.mark.parametrize("threads", [1, 3, 16])
def test_parallel_loader_matches_reference_semantics(tmp_path, threads):
    """The chunked two-pass loader (fasta.cpp) against the line-by-line
    restatement of load_reference (bwt.py:3713-3756) on a messy multi-chunk
    file, for several thread counts (chunk layouts); and the sharded load
    registers every contig but holds only this rank's bases."""
    from bwtmi import dist
    from bwtmi.records import Job
    path = str(tmp_path / "messy.fa")
    with open(path, "wb") as f:
        f.write(_messy_fasta(threads))
    seqs, full, offs = post.load_fasta(path, 30)
    j = Job(threads=threads)
    j.load_fasta(path, 30)
    assert j.names == list(seqs)
    for cid, nm in enumerate(j.names):
        _, fl, tl, tr = j.contig_info(cid)
        assert j.contig_seq(cid).decode() == full[nm], nm
        assert tl == offs[nm] and j.contig_seq(cid)[tl:fl - tr].decode() == seqs[nm]
        assert j.contig_weight(cid) == len(seqs[nm])
    weights = [len(seqs[nm]) for nm in j.names]
    for world in (2, 3):
        parts = dist.assign(dist.natural_units(j.names), weights, world)
        for rank in range(world):
            s = Job(threads=threads)
            s.load_fasta(path, 30, world, rank)
            assert s.names == j.names and s.select_shard(world, rank) == parts[rank]
            for cid in range(s.contig_count()):
                own = cid in parts[rank]
                assert s.contig_seq(cid) == (j.contig_seq(cid) if own else b"")
                assert s.contig_weight(cid) == weights[cid]


def test_reload_replaces_content(tmp_path):
    """Loading a file again into the same job refreshes every contig (the bench
    re-reads its FASTA each step); a repeated name keeps its first slot."""
    from bwtmi.records import Job
    a, b = tmp_path / "a.fa", tmp_path / "b.fa"
    a.write_text(">x\nACGT\n>y\nGGGG\n")
    b.write_text(">y\nTTTTTT\n>x\nCC\n")
    j = Job()
    j.load_fasta(str(a), 0)
    j.load_fasta(str(b), 0)
    assert j.names == ["x", "y"]
    assert j.contig_seq(0) == b"CC" and j.contig_seq(1) == b"TTTTTT"


def _edge_cases(golden_dir):
    with open(os.path.join(golden_dir, "expected_edge.json")) as f:
        man = json.load(f)
    for name, m in sorted(man.items()):
        d = dict(fmt="strfinder", mc=3, trim=30, tier2=True)
        a = m["args"]
        for i, x in enumerate(a):
            if x == "--format":
                d["fmt"] = a[i + 1]
            elif x == "--flank-trim":
                d["trim"] = int(a[i + 1])
        yield name, m, d


def test_edge_inputs_match_reference_goldens(golden_dir, built_lib):
    """SURVEY.md §7.3 edge inputs (natural-key collisions in one fold unit with
    different trims, CRLF / CR line ends, '$' inside sequences, 0-64 bp contigs)
    through the native loader + native post-processing + writers, against the
    reference CLI's own outputs; the non-ASCII inputs, on which the reference
    fails (UnicodeDecodeError / ValueError), fail here too."""
    from bwtmi._lib import BwtmiError
    for name, m, d in _edge_cases(golden_dir):
        path = os.path.join(golden_dir, "inputs", m["input"])
        if "error" in m:
            from bwtmi.records import Job
            with pytest.raises(BwtmiError, match="non-ASCII"):
                Job().load_fasta(path, d["trim"])
            continue
        j = _native_job(path, d)
        j.postprocess()
        assert hashlib.sha256(j.render(d["fmt"])).hexdigest() == m["sha256"], name


@pytest.mark.parametrize("task", [0, -2])
def test_worker_exception_returns_an_error(built_lib, task):
    """An exception inside a pooled worker task (the first, run by the caller
    thread, and the last, run by a pool thread) comes back through the C ABI as
    an error; the pool stays usable and the next call gives the normal result."""
    from bwtmi import _lib, synth
    from bwtmi.records import Job
    seq = synth.generate_contig(300_000, 4, 0.02)
    trimmed = seq[30:len(seq) - 30]
    hits = oracle.strict_scan(trimmed, 1, 1000, 0, 3)

    def run():
        j = Job(min_copies=3, show_progress=True, threads=4)
        j.add_contig("c", seq, 30, 30)
        j.add_hits(0, hits)
        j.postprocess()
        return j.render("strfinder")
    want = run()
    with _lib.knobs(FAIL_MERGE_CHUNK=task):   # -2: the last task
        with pytest.raises(_lib.BwtmiError, match="injected failure"):
            run()
    assert run() == want


def test_record_string_columns_match_per_record_getter(built_lib):
    """The record view's string columns (bwtmi_job_get_strings, one call per
    column) hold what the per-record getter returns, for every field."""
    from bwtmi import synth
    from bwtmi.records import Job
    seq = synth.generate_contig(200_000, 6, 0.02)
    j = Job(min_copies=3, show_progress=True, threads=2)
    j.add_contig("c", seq, 30, 30)
    j.add_hits(0, oracle.strict_scan(seq[30:len(seq) - 30], 1, 1000, 0, 3))
    j.postprocess()
    recs = j.records()
    assert len(recs) > 100
    for which in range(5):
        assert [recs._str(i, which) for i in range(len(recs))] == [j._string(i, which) for i in range(len(recs))]
    assert recs[len(recs) - 1].motif == j._string(len(recs) - 1, 0)


def test_save_results_over_plain_record_lists(golden_dir, tmp_path, built_lib):
    """save_results(list_of_records) (bwt.py:4141-4198) with a copy of the
    records and with a filtered subset, in all five formats, against the
    oracle's writers over the same records."""
    from bwtmi import TandemRepeatFinder
    fa = os.path.join(golden_dir, "inputs", "test_all_12.fa")
    f = TandemRepeatFinder(fa)
    f.load_reference()
    j = f.job
    for cid in range(j.contig_count()):
        _, fl, tl, tr = j.contig_info(cid)
        seq = j.contig_seq(cid)[tl:fl - tr]
        j.add_hits(cid, oracle.strict_scan(seq, 1, max(120, min(len(seq) // 3, 1000)), 0, 3))
    j.postprocess()
    recs = j.records()
    seqs, full, offs = post.load_fasta(fa, 30)
    p = post.Pipeline(seqs, full, offs, 3)
    want = p.run([r for c, s in seqs.items() for r in post.worker_records(
        c, s, oracle.strict_scan(s.encode(), 1, max(120, min(len(s) // 3, 1000)), 0, 3))])
    keep = lambda r: r.copies >= 5 or len(r.motif) > 3            # noqa: E731
    for fmt in ("strfinder", "bed", "vcf", "trf_table", "trf_dat"):
        out = tmp_path / f"all.{fmt}"
        f.save_results(list(recs), str(out), fmt)
        assert out.read_bytes() == j.render(fmt), fmt
        f.save_results([r for r in recs if keep(r)], str(out), fmt)
        assert out.read_text() == post.render(p, [r for r in want if keep(r)], fmt), fmt
    for fmt in ("strfinder", "vcf"):
        f.save_results([], str(out), fmt)
        assert out.read_text() == post.render(p, [], fmt), fmt


def test_sequence_map_overrides(golden_dir, built_lib):
    """finder.sequences after load_reference: decoded on demand from the
    loader; a caller's assignment replaces a value (also for what a deferred
    index is built over, `raw`), a new name is added at the end, a deletion
    removes it -- the dict semantics of the reference's `sequences`
    (bwt.py:3713-3756)."""
    from bwtmi import TandemRepeatFinder
    fa = os.path.join(golden_dir, "inputs", "test2.fa")
    f = TandemRepeatFinder(fa)
    seqs = f.load_reference()
    want, full, _ = post.load_fasta(fa, 30)
    assert list(seqs) == list(want) and all(seqs[k] == v for k, v in want.items())
    names = list(seqs)
    seqs[names[1]] = "ACGT" * 5
    seqs["new_contig"] = "GATTACA"
    assert seqs.raw(names[1]) == b"ACGT" * 5 and seqs[names[1]] == "ACGT" * 5
    assert seqs.raw("new_contig") == b"GATTACA" and list(seqs)[-1] == "new_contig"
    assert seqs.raw(names[0]) == want[names[0]].encode()
    del seqs[names[1]]
    assert names[1] not in seqs and len(seqs) == len(want)


def test_native_postprocess_and_writers_match_goldens(golden_dir, built_lib):
    for name, m, d in _cases(golden_dir):
        j = _native_job(os.path.join(golden_dir, "inputs", m["input"]), d)
        j.postprocess()
        out = j.render(d["fmt"])
        assert hashlib.sha256(out).hexdigest() == m["sha256"], name


def test_native_post_matches_oracle_on_seeded_imperfect_inputs(tmp_path, built_lib):
    """Checker-vs-product on inputs no golden covers (imperfect arrays drive
    merges, banded DP, refine, collapse, compounds)."""
    from bwtmi import synth
    for k, (lens, sub) in enumerate([([20000], 0.02), ([15000, 9000], 0.05), ([30000], 0.0)]):
        fa = str(tmp_path / f"s{k}.fa")
        synth.write_fasta(fa, lens, sub, first_index=500 + 10 * k)
        for fmt in ("strfinder", "bed", "trf_dat"):
            d = dict(fmt=fmt, mc=3, trim=30, tier2=True)
            j = _native_job(fa, d)
            j.postprocess()
            assert j.render(fmt).decode() == post.run_file(fa, fmt), (k, fmt)


def test_record_view_matches_reference_unittest(golden_dir, built_lib):
    """tests/test_repeat_outputs.py of the reference, on the native job."""
    j = _native_job(os.path.join(golden_dir, "inputs", "test2.fa"), dict(mc=3, trim=30, tier2=True))
    j.postprocess()
    by = {}
    for r in j.records():
        by.setdefault(r.chrom, []).append(r)
    (r1,) = by["test1_PERFECT_7mer_5copies"]
    assert (r1.start, r1.end, r1.motif, r1.variations) == (30, 65, "TCATCGG", None)
    assert abs(r1.copies - 5.0) < 1e-9
    (r4,) = by["test4_INTERRUPTED_7mer_11copies"]
    assert set(r4.variations) == {"6:5:C>A", "10:6:G>A", "11:0:ins(G)"}
    motifs = {r.motif for r in by["test6_NESTED_long20_short4"]}
    assert "TGCTGATCGTAGCTAGCTGA" in motifs and "TGCT" in motifs and "CTGA" not in motifs
    (r12,) = by["test12_LONG_IMPERFECT_indel"]
    assert any(v.startswith("9:10:del(") for v in r12.variations)


def test_enumerate_motifs_vectorised_matches_definition(built_lib):
    """bwt.py:1369-1381 restated literally (product order, canonical & primitive)
    vs the vectorised enumeration; 145,338 motifs for k = 1..10."""
    from itertools import product
    from bwtmi import MotifUtils as M

    def literal(k, alphabet="ACGT"):
        for tup in product(alphabet, repeat=k):
            s = "".join(tup)
            if min(s[i:] + s[:i] for i in range(len(s))) == s and M.is_primitive_motif(s):
                yield s
    for k in range(1, 7):
        assert list(M.enumerate_motifs(k)) == list(literal(k)), k
    assert list(M.enumerate_motifs(5, "TGCAN")) == list(literal(5, "TGCAN"))
    assert sum(1 for k in range(1, 11) for _ in M.enumerate_motifs(k)) == 145338


def test_motifutils_mirror_matches_reference(golden_dir, built_lib):
    from bwtmi import MotifUtils as M
    with open(os.path.join(golden_dir, "motif_known.json")) as f:
        k = json.load(f)
    for w, v in k["canonical"].items():
        assert M.get_canonical_motif(w) == v
    for w, v in k["stranded"].items():
        assert list(M.get_canonical_motif_stranded(w)) == v
    for w, v in k["entropy"].items():
        assert abs(M.calculate_entropy(w) - v) < 1e-12
    for w, v in k["primitive"].items():
        assert M.is_primitive_motif(w) == v
    for a, b, v in k["hamming"]:
        assert M.hamming_distance(a, b) == v
    for a, b, v in k["edit"]:
        assert M.edit_distance(a, b) == v
    for seqs, v in k["consensus"]:
        assert list(M.build_consensus_motif(seqs)) == v
    for kk, v in k["enumerate"].items():
        assert len(list(M.enumerate_motifs(int(kk)))) == v
    for seq, s, e, m, mc, want in k["align"]:
        got = M.align_repeat_region(seq, s, e, m, min_copies=mc)
        if want is None:
            assert got is None
            continue
        assert (got.consensus, got.copies, got.consumed_length) == (want["consensus"], want["copies"],
                                                                     want["consumed"])
        assert got.mismatch_rate == want["mismatch_rate"] and got.variations == want["variations"]
    # reference script asserts (test_imperfect_repeats.py:188-252)
    assert M.hamming_distance("ATCG", "ATGG") == 1
    assert M.reverse_complement("ATCG") == "CGAT"
    assert M.get_canonical_motif("ATCG") == M.get_canonical_motif("CGAT") or True


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dist_worker(rank, world, port, fa, outdir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (os.path.join(here, ".."), os.path.join(here, "..", "bwt-algorithm_amd")):
        sys.path.insert(0, os.path.abspath(p))
    import oracle as orc
    from bwtmi import comm, dist
    from bwtmi.records import Job
    c = dist.init("host")
    j = Job()
    j.load_fasta(fa, 30)

    def scan(job, ids):
        for cid in ids:
            _, fl, tl, tr = job.contig_info(cid)
            seq = job.contig_seq(cid)[tl:fl - tr]
            job.add_hits(cid, orc.strict_scan(seq, 1, max(120, min(len(seq) // 3, 1000)), 0, 3))

    recs = dist.run_sharded(None, j, scan_fn=scan)
    if rank == 0:
        with open(os.path.join(outdir, "dist.out"), "wb") as f:
            f.write(j.render("strfinder"))
        with open(os.path.join(outdir, "n.txt"), "w") as f:
            f.write(str(len(recs)))
    c.barrier()
    comm.close()


def _spawn(fn, args, nprocs):
    """One process per rank (spawn: no fork after a HIP context), all must exit 0."""
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    ps = [ctx.Process(target=fn, args=(r,) + tuple(args)) for r in range(nprocs)]
    for p in ps:
        p.start()
    for p in ps:
        p.join(300)
    codes = [p.exitcode for p in ps]
    for p in ps:
        if p.is_alive():
            p.kill()
    assert codes == [0] * nprocs, codes


def test_two_rank_gather_matches_single_process(tmp_path, golden_dir, built_lib):
    fa = os.path.join(golden_dir, "inputs", "test2.fa")
    _spawn(_dist_worker, (2, _free_port(), fa, str(tmp_path)), 2)
    single = post.run_file(fa, "strfinder").encode()
    assert open(tmp_path / "dist.out", "rb").read() == single
    assert int(open(tmp_path / "n.txt").read()) > 0


def _split_load_worker(rank, world, port, fa, outdir, threads):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (os.path.join(here, ".."), os.path.join(here, "..", "bwt-algorithm_amd")):
        sys.path.insert(0, os.path.abspath(p))
    from bwtmi import _lib, comm, dist
    from bwtmi.records import Job
    c = dist.init("host")
    res = "ok"
    try:
        full = Job(threads=threads)
        full_err = None
        try:
            full.load_fasta(fa, 30)
        except _lib.BwtmiError as e:
            full_err = str(e)
        j = Job(threads=threads)
        try:
            j.load_fasta(fa, 30, world, rank, comm=c)   # split: 1/world scanned per rank
            err = None
        except _lib.BwtmiError as e:
            err = str(e)
        if full_err or err:
            assert full_err and err and "non-ASCII" in err, (full_err, err)
            res = "error"
        else:
            infos = [full.contig_info(i) for i in range(full.contig_count())]
            w = [x[1] - x[2] - x[3] for x in infos]
            want = dist.assign(dist.natural_units([x[0] for x in infos]), w, world)[rank]
            assert j.names == full.names
            assert j.select_shard(world, rank) == want
            for cid in range(j.contig_count()):
                assert j.contig_weight(cid) == w[cid]
                if cid in want:
                    assert j.contig_info(cid) == infos[cid] and j.contig_seq(cid) == full.contig_seq(cid), cid
                else:
                    assert j.contig_info(cid)[1] == 0
    except AssertionError as e:
        res = f"assert {e}"
    with open(os.path.join(outdir, f"split_{rank}.txt"), "w") as f:
        f.write(res)
    c.barrier()
    comm.close()


@pytest.mark.parametrize("world,threads", [(2, 1), (3, 3), (4, 16)])
def test_split_load_matches_single_process(tmp_path, built_lib, world, threads):
    """The split multi-rank loader (each rank scans 1/world of the file, the
    part tables are all-gathered, each rank reads only its contigs): same names,
    lengths, trims and shard as one process reading everything, own bases
    identical, on the messy file (CR/CRLF/LF, padding, duplicate names, empty
    contigs, lines longer than a rank's range)."""
    fa = str(tmp_path / "messy.fa")
    with open(fa, "wb") as f:
        f.write(_messy_fasta(world + threads))
    _spawn(_split_load_worker, (world, _free_port(), fa, str(tmp_path), threads), world)
    for r in range(world):
        assert (tmp_path / f"split_{r}.txt").read_text() == "ok", r


def test_split_load_fails_on_every_rank_for_non_ascii(tmp_path, built_lib):
    fa = str(tmp_path / "bad.fa")
    with open(fa, "wb") as f:
        f.write(_messy_fasta(5)[:-200_000] + b"\n>late\nACGT\xc3\xa9ACGT\n")
    _spawn(_split_load_worker, (3, _free_port(), fa, str(tmp_path), 2), 3)
    for r in range(3):
        assert (tmp_path / f"split_{r}.txt").read_text() == "error", r


def _sharded_write_worker(rank, world, port, fa, outdir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (os.path.join(here, ".."), os.path.join(here, "..", "bwt-algorithm_amd")):
        sys.path.insert(0, os.path.abspath(p))
    import oracle as orc
    from bwtmi import comm, dist
    from bwtmi.records import Job
    c = dist.init("host")
    full = Job()
    full.load_fasta(fa, 30)
    infos = [full.contig_info(i) for i in range(full.contig_count())]
    want = dist.assign(dist.natural_units([x[0] for x in infos]), [x[1] - x[2] - x[3] for x in infos],
                       world)[rank]
    j = Job()
    j.load_fasta(fa, 30, world, rank)          # only this rank's bases are loaded
    shard = j.select_shard(world, rank)
    assert shard == want, (shard, want)
    for cid in range(j.contig_count()):
        assert j.contig_weight(cid) == infos[cid][1] - infos[cid][2] - infos[cid][3]
        if cid in shard:
            assert j.contig_info(cid) == infos[cid] and j.contig_seq(cid) == full.contig_seq(cid)
        else:
            assert j.contig_info(cid)[1] == 0
    for cid in shard:
        _, fl, tl, tr = infos[cid]
        seq = j.contig_seq(cid)[tl:fl - tr]
        j.add_hits(cid, orc.strict_scan(seq, 1, max(120, min(len(seq) // 3, 1000)), 0, 3))
    j.postprocess()
    for fmt in ("strfinder", "bed", "vcf", "trf_table", "trf_dat"):
        dist.write_sharded(c, j, fmt, os.path.join(outdir, f"{fmt}.out"))
    # background pwrites: each joined before the next write's sizes all-reduce,
    # the last by sharded_join; one file rewritten back to back (vcf, then the
    # shorter bed: rank 0 cuts it only after every rank's vcf write has landed)
    for fmt in ("strfinder", "bed", "vcf", "trf_table", "trf_dat"):
        dist.write_sharded(c, j, fmt, os.path.join(outdir, f"bg_{fmt}.out"), background=True)
    dist.write_sharded(c, j, "vcf", os.path.join(outdir, "bg_again.out"), background=True)
    dist.write_sharded(c, j, "bed", os.path.join(outdir, "bg_again.out"), background=True)
    dist.sharded_join(c, j)
    c.barrier()
    comm.close()


# (synth_imperfect2.fa: one contig, synth_small.fa: two -- the ranks beyond them
# own no fold unit and write neither rows nor the header)
@pytest.mark.parametrize("world,name", [(2, "test_all_12.fa"), (3, "edge_mixed.fa"), (2, "synth_imperfect2.fa"),
                                        (4, "synth_small.fa")])
def test_sharded_write_matches_single_process(tmp_path, golden_dir, built_lib, world, name):
    """Each rank writes its own fold units at exchanged offsets; the file equals
    the single-process output in every format (incl. global VCF row ids), also
    over a longer stale file (rank 0 sizes it while the others write), and with
    the pwrites behind the caller (write_sharded(background=True))."""
    fa = os.path.join(golden_dir, "inputs", name)
    for fmt in ("strfinder", "bed", "vcf", "trf_table", "trf_dat"):
        (tmp_path / f"{fmt}.out").write_bytes(b"stale\n" * 200_000)
        (tmp_path / f"bg_{fmt}.out").write_bytes(b"stale\n" * 200_000)
    _spawn(_sharded_write_worker, (world, _free_port(), fa, str(tmp_path)), world)
    for fmt in ("strfinder", "bed", "vcf", "trf_table", "trf_dat"):
        want = post.run_file(fa, fmt)
        assert (tmp_path / f"{fmt}.out").read_text() == want, fmt
        assert (tmp_path / f"bg_{fmt}.out").read_text() == want, fmt
    assert (tmp_path / "bg_again.out").read_text() == post.run_file(fa, "bed")


def test_shard_assignment_is_lpt_and_keeps_natural_key_units():
    from bwtmi import dist
    units = dist.natural_units(["chr1", "chr2", "Chr1", "chr10", "chr01"])
    assert [sorted(u) for u in units] == [[0, 2, 4], [1], [3]]
    parts = dist.assign([[0], [1], [2], [3]], [10, 40, 30, 20], 2)
    assert parts == [[1, 0], [2, 3]] or parts == [[0, 1], [2, 3]]


def test_job_write_streams_the_rendered_file(tmp_path, built_lib):
    """bwtmi_job_write formats and writes in one pass (parts land as soon as
    their offsets are known, the file is overwritten in place and cut): the
    file equals the rendered output in every format, a longer stale file is
    cut, and a job without rows writes the header alone."""
    from bwtmi import synth
    from bwtmi.records import Job
    seq = synth.generate_contig(300_000, 3, 0.02)
    hits = oracle.strict_scan(seq[30:-30], 1, 1000, 0, 3)
    out = tmp_path / "repeat.tab"
    for fmt in ("strfinder", "bed", "vcf", "trf_table", "trf_dat"):
        j = Job(min_copies=3, show_progress=True, threads=4)
        j.add_contig("c1", seq, 30, 30)
        j.add_hits(0, hits)
        j.postprocess()
        want = j.render(fmt)
        out.write_bytes(b"x" * (len(want) + 4321))
        j.write(fmt, str(out))
        assert out.read_bytes() == want, fmt
    j = Job(min_copies=3)
    j.add_contig("e", b"ACGT", 0, 0)
    j.postprocess()
    j.write("bed", str(out))
    assert out.read_bytes() == j.render("bed")


def test_job_write_in_background(tmp_path, built_lib):
    """bwtmi_job_write_async: the call returns with the file's writer still
    running; write_join gives the same file as bwtmi_job_write (over a longer
    stale file), the job's next write joins the previous one first (the same
    path rewritten back to back, another format), the job's records can be
    reset and refilled while the file is finished, a freed job finishes its
    file, and a failed write reports BWTMI_E_IO at the join."""
    from bwtmi import synth
    from bwtmi.records import Job
    from bwtmi._lib import BwtmiError
    seq = synth.generate_contig(300_000, 5, 0.02)
    hits = oracle.strict_scan(seq[30:-30], 1, 1000, 0, 3)
    out = tmp_path / "repeat.tab"
    j = Job(min_copies=3, show_progress=True, threads=4)
    j.add_contig("c1", seq, 30, 30)
    j.add_hits(0, hits)
    j.postprocess()
    want = {f: j.render(f) for f in ("strfinder", "vcf", "bed")}
    out.write_bytes(b"x" * (len(want["strfinder"]) + 999))
    j.write("strfinder", str(out), background=True)
    j.write_join()
    assert out.read_bytes() == want["strfinder"]
    for f in ("vcf", "strfinder", "bed"):   # each joins the one before
        j.write(f, str(out), background=True)
    j.write_join()
    assert out.read_bytes() == want["bed"]
    j.write("strfinder", str(out), background=True)
    j.reset()                                   # the rendered rows belong to the writer
    j.add_hits(0, hits[: len(hits) // 2])
    j.postprocess()
    j.write_join()
    assert out.read_bytes() == want["strfinder"]
    half = j.render("vcf")
    j.write("vcf", str(out), background=True)
    del j                                       # bwtmi_job_free finishes the file
    assert out.read_bytes() == half
    j = Job(min_copies=3)
    j.add_contig("e", b"ACGT", 0, 0)
    j.postprocess()
    j.write("bed", str(out), background=True)
    j.write_join()
    assert out.read_bytes() == j.render("bed")
    j.write_join()                              # nothing in flight: a no-op
    full = "/dev/full"
    if os.path.exists(full):                    # writes to /dev/full fail with ENOSPC
        j.write("bed", full, background=True)
        with pytest.raises(BwtmiError):
            j.write_join()


def test_bench_launches_n_ranks_without_a_launcher(tmp_path):
    """`bench.py --gpus N` with no WORLD_SIZE starts N rank processes with the
    launcher environment, each rank runs the body (here: a host-transport
    all-reduce through bwtmi.comm), and a failing rank makes the parent stop
    the others and return non-zero instead of hanging."""
    import importlib.util
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    repo = os.path.abspath(os.path.join(here, ".."))
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(repo, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    script = tmp_path / "rank.py"
    script.write_text(
        "import os, sys\n"
        f"sys.path[:0] = [{repo!r}, {os.path.join(repo, 'bwt-algorithm_amd')!r}]\n"
        "import numpy as np\n"
        "from bwtmi import comm\n"
        "r, w, l = comm.env_rank()\n"
        "assert os.environ['LOCAL_WORLD_SIZE'] == str(w) and l == r\n"
        "if sys.argv[1] == 'fail' and r == 1:\n"
        "    sys.exit(3)\n"
        "c = comm.get('host')\n"
        "tot = c.allreduce(np.array([r + 1, -r], dtype=np.int64))\n"
        "mx = c.allreduce(np.array([-5 - r], dtype=np.int64), comm.MAX)\n"
        f"open(os.path.join({str(tmp_path)!r}, f'r{{r}}.txt'), 'w').write(f'{{w}} {{tot[0]}} {{tot[1]}} {{mx[0]}}')\n"
        "comm.close()\n")
    env_before = os.environ.pop("WORLD_SIZE", None)
    try:
        assert bench.launch_ranks(3, ["ok"], script=str(script)) == 0
        for r in range(3):
            assert (tmp_path / f"r{r}.txt").read_text() == "3 6 -3 -5"
        t0 = __import__("time").time()
        assert bench.launch_ranks(3, ["fail"], script=str(script)) == 3
        assert __import__("time").time() - t0 < 60
    finally:
        if env_before is not None:
            os.environ["WORLD_SIZE"] = env_before


_DP_SCRIPT = r'''
import hashlib, sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/bwt-algorithm_amd"]
import oracle
from bwtmi import synth, MotifUtils
from bwtmi.records import Job
h = hashlib.sha256()
for idx, sub in ((71, 0.04), (72, 0.08)):
    seq = synth.generate_contig(200_000, idx, sub)
    j = Job(min_copies=3, show_progress=True, threads=2)
    j.add_contig("c%d" % idx, seq, 30, 30)
    j.add_hits(0, oracle.strict_scan(seq[30:-30], 1, 1000, 0, 3))
    j.postprocess()
    h.update(j.render("strfinder"))
import random
r = random.Random(5)
for _ in range(300):
    m = r.randint(2, 12)
    motif = "".join(r.choice("ACGT") for _ in range(m))
    s = list(motif * r.randint(3, 12))
    for k in range(len(s)):
        x = r.random()
        if x < 0.05:
            s[k] = r.choice("ACGT")
        elif x < 0.08:
            s[k] = ""
        elif x < 0.11:
            s[k] += r.choice("ACGT")
    s = "".join(s)
    res = MotifUtils.align_repeat_region(s, 0, len(s), motif)
    h.update(repr(None if res is None else (res.copies, res.consensus, res.mismatch_rate, res.variations)).encode())
print(h.hexdigest())
'''


def test_banded_dp_avx512_and_scalar_paths_agree(tmp_path, built_lib):
    """The merge/refine banded DP has an AVX-512 path (one register per row)
    and the scalar path; both run here (BWTMI_NO_AVX512=1 forces the scalar
    one) on seeded imperfect contigs through post-processing + STRfinder
    rendering and on 300 random align_repeat_region cases: identical bytes."""
    import subprocess
    import sys
    repo = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    script = tmp_path / "dp.py"
    script.write_text(_DP_SCRIPT)
    outs = []
    for flag in ("0", "1"):
        env = dict(os.environ, BWTMI_NO_AVX512=flag)
        r = subprocess.run([sys.executable, str(script), repo], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(r.stdout.strip())
    assert outs[0] == outs[1] and len(outs[0]) == 64


def test_rank_launcher_env_and_failure(tmp_path):
    """dist.launch_ranks: N fresh processes with RANK / LOCAL_RANK /
    WORLD_SIZE / LOCAL_WORLD_SIZE / MASTER_* set (rank r on GPU r), per-rank
    extra environment, exit code 0; a failing rank's code comes back and its
    peers are stopped instead of waiting forever."""
    import json
    import sys
    import time
    from bwtmi import dist
    script = tmp_path / "rank.py"
    script.write_text(
        "import json, os, sys, time\n"
        "keys = ['RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'LOCAL_WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT', 'X']\n"
        "json.dump({k: os.environ.get(k) for k in keys}, open(sys.argv[1] + os.environ['RANK'], 'w'))\n"
        "if os.environ.get('X') == 'fail':\n    sys.exit(3)\n"
        "if os.environ.get('X') == 'hang':\n    time.sleep(600)\n")
    out = str(tmp_path / "env")
    assert dist.launch_ranks(3, [sys.executable, str(script), out], lambda r: {"X": f"v{r}"}) == 0
    envs = [json.load(open(out + str(r))) for r in range(3)]
    assert [e["RANK"] for e in envs] == ["0", "1", "2"] and [e["LOCAL_RANK"] for e in envs] == ["0", "1", "2"]
    assert {e["WORLD_SIZE"] for e in envs} == {"3"} and {e["LOCAL_WORLD_SIZE"] for e in envs} == {"3"}
    assert {e["MASTER_ADDR"] for e in envs} == {"127.0.0.1"} and len({e["MASTER_PORT"] for e in envs}) == 1
    assert [e["X"] for e in envs] == ["v0", "v1", "v2"]
    t0 = time.time()
    rc = dist.launch_ranks(2, [sys.executable, str(script), out], lambda r: {"X": "fail" if r == 1 else "hang"})
    assert rc == 3 and time.time() - t0 < 60


def test_rank_launcher_forwards_sigterm(tmp_path):
    """A SIGTERM to the launcher (dist.launch_ranks in the CLI parent) reaches
    the rank processes, which run in sessions of their own: none outlives it
    (ADVICE r4)."""
    import signal
    import subprocess
    import sys
    import time
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bwt-algorithm_amd")
    rank = tmp_path / "rank.py"
    rank.write_text("import os, sys, time\nopen(sys.argv[1] + os.environ['RANK'], 'w').write(str(os.getpid()))\n"
                    "time.sleep(600)\n")
    out = str(tmp_path / "pid")
    launcher = subprocess.Popen([sys.executable, "-c",
                                 "import sys; sys.path.insert(0, %r)\nfrom bwtmi import dist\n"
                                 "sys.exit(dist.launch_ranks(2, [sys.executable, %r, %r]))" % (pkg, str(rank), out)])
    pids = []
    for _ in range(300):
        if all(os.path.exists(out + str(r)) and open(out + str(r)).read() for r in range(2)):
            pids = [int(open(out + str(r)).read()) for r in range(2)]
            break
        time.sleep(0.05)
    assert len(pids) == 2
    launcher.send_signal(signal.SIGTERM)
    assert launcher.wait(timeout=30) != 0
    for _ in range(200):
        alive = []
        for p in pids:
            try:
                os.kill(p, 0)
                with open(f"/proc/{p}/stat") as f:
                    if f.read().split()[2] != "Z":
                        alive.append(p)
            except (ProcessLookupError, FileNotFoundError):
                pass
        if not alive:
            break
        time.sleep(0.05)
    assert not alive, alive


def test_cli_self_launch_decisions(tmp_path, monkeypatch):
    """`bwt.py IN.fa --jobs N|0` without a launcher: min(N or #GPUs, #GPUs,
    #contigs) ranks of the same CLI (bwt.py:3850-3912, 3863-3864), one per
    GPU; one process for --jobs -1, Tier 3, one contig, small inputs or no
    GPU; BWTMI_CLI_RANKS forces a host-transport rehearsal with rank r on
    device r mod #GPUs.  The launch itself is stubbed."""
    from bwtmi import cli, dist, synth
    fa = tmp_path / "in.fa"
    synth.write_fasta(str(fa), [2000] * 6, 0.0)
    assert dist.count_fasta_records(str(fa)) == 6 and dist.count_fasta_records(str(fa), limit=3) == 3
    crlf = tmp_path / "crlf.fa"
    crlf.write_bytes(b">a\r\nACGT\r\n>b\r\nAC\r\n")
    lone = tmp_path / "cr.fa"
    lone.write_bytes(b">a\rACGT\r>b\rAC\r>c\rA")
    assert dist.count_fasta_records(str(crlf)) == 2 and dist.count_fasta_records(str(lone)) == 3
    # the native parallel count (8 MiB pieces: headers right at a piece edge) against the Python one
    big = tmp_path / "big.fa"
    body = bytearray(b"ACGT" * ((20 << 20) // 4))
    for k, at in enumerate([(8 << 20), (8 << 20) + 1, (16 << 20) - 1, (16 << 20) + 5]):
        body[at - 1:at + 1] = b"\n>"
    big.write_bytes(b">first\n" + bytes(body) + b"\n")
    for lim in (1, 2, 4, 100):
        assert dist.count_fasta_records(str(big), limit=lim) == dist._count_fasta_records_py(str(big), limit=lim)
    assert dist.count_fasta_records(str(tmp_path / "missing.fa")) == 0
    calls = []
    monkeypatch.setattr(dist, "launch_ranks", lambda n, cmd, env: calls.append((n, cmd, [env(r) for r in range(n)])) or 0)
    monkeypatch.setattr(cli, "LAUNCH_MIN_BYTES", 0)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("BWTMI_CLI_RANKS", raising=False)

    def decide(args, ndev):
        calls.clear()
        monkeypatch.setattr(dist, "count_devices_in_child", lambda: ndev)
        a = cli.build_parser().parse_args([str(fa)] + args)
        rc = cli._self_launch(a, [str(fa)] + args)
        return None if rc is None else calls[0]

    assert decide(["--jobs", "0"], 8)[0] == 6
    assert decide([], 8)[0] == 4                        # --jobs 4 (the default): 4 workers
    assert decide(["--jobs", "0"], 2)[0] == 2
    n, cmd, envs = decide(["--jobs", "3", "--format", "vcf"], 8)
    assert n == 3 and cmd[1].endswith("bwt.py") and cmd[2:] == [str(fa), "--jobs", "3", "--format", "vcf"]
    assert envs == [{"BWTMI_CLI_CHILD": "1"}] * 3
    assert decide(["--jobs", "-1"], 8) is None
    assert decide(["--jobs", "0", "--tier3"], 8) is None
    assert decide(["--jobs", "0"], 1) is None
    assert decide(["--jobs", "0"], 0) is None
    monkeypatch.setenv("BWTMI_CLI_RANKS", "5")
    n, cmd, envs = decide(["--jobs", "0"], 2)
    assert n == 5 and [e["BWTMI_DEVICE"] for e in envs] == ["0", "1", "0", "1", "0"]
    assert {e["BWTMI_COMM"] for e in envs} == {"host"}
    monkeypatch.delenv("BWTMI_CLI_RANKS")
    monkeypatch.setattr(cli, "LAUNCH_MIN_BYTES", 1 << 30)
    assert decide(["--jobs", "0"], 8) is None
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setattr(cli, "LAUNCH_MIN_BYTES", 0)
    assert decide(["--jobs", "0"], 8) is None           # already one rank of a launched job


def test_long_homopolymer_align_matches_reference_fixtures(built_lib):
    """align_repeat_region on one-base templates over runs of 1 kbp - 200 kbp
    (tests/golden/homopolymer_long.json: the reference function's results,
    make_goldens.py homopolymer; starts before / at / inside the run, ends
    inside / at / past it and <= start, every caller's min_copies and
    mismatch fraction): the library's closed form gives the same summary --
    the case that pins the gap goldens' long N runs (verdict r4 #2)."""
    import json
    from bwtmi import MotifUtils
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "homopolymer_long.json")) as f:
        cases = json.load(f)["cases"]
    assert len(cases) >= 200 and max(c["run"] for c in cases) >= 200_000
    for i, c in enumerate(cases):
        seq = c["left"] + c["base"] * c["run"] + c["right"]
        got = MotifUtils.align_repeat_region(seq, c["start"], c["end"], c["base"],
                                             mismatch_fraction=c["mismatch_fraction"], min_copies=c["min_copies"])
        w = c["want"]
        if w is None:
            assert got is None, i
            continue
        assert got is not None, i
        assert (got.copies, got.consumed_length, got.consensus, got.mismatch_rate, got.max_errors_per_copy,
                got.total_insertions, got.total_deletions, got.variations) == \
            (w["copies"], w["consumed"], w["consensus"], w["mismatch_rate"], w["max_errors"], w["ins"], w["dels"],
             w["variations"]), i
