"""The FM index at sample rates other than 32 / 128 and on alphabets past 16
symbols, against the CPU oracle (pinned to the reference on the same kind of
grid by tests/test_oracle.py::test_index_rates_match_reference).  Integer
work: every comparison is exact.

The rates select the code that runs (index.hip, sa_dna.hip; d_rank's consumers
in search.hip):

  occ_sample 16 .. 1024, a power of two, <= 16 symbols   k_occ_groups<1 .. 64>
  any other rate or more than 16 symbols                k_occ_blocks, with
      16-aligned blocks and <= 16 symbols               SWAR compares alone
      blocks that are no multiple of 16                 the byte loop alone
      16-aligned blocks and > 16 symbols                16 SWAR rows + byte loop
  occ_sample as d_rank's block (k_bsearch, k_loc_seed)  pos / k, a tail of < k bytes
  sa_sample in the string sorts' last pass              k_dna_final
  sa_sample after the general doubling                  k_sample
  16 .. 94 symbols in the doubling's first key          b = 5, 6, 7 bits a symbol
"""
import ctypes as C
import hashlib
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

PRINTABLE = bytes(c for c in range(0x21, 0x7F) if c != ord("$"))     # 93 symbols, '$' left out
WIDE20 = b'!"#%+09:AMZ_agtz{|}~'       # 20 symbols: three below '$', lower case, the top of ASCII
assert len(set(WIDE20)) == 20 and set(WIDE20) <= set(PRINTABLE)


def _runs(rng, t, lo, symbols):
    """Plant homopolymer runs into t[lo:]: three of 40-70 symbols when there is
    room (the BWT then has long equal stretches), else one over half of it."""
    L = len(t) - lo
    if L >= 200:
        for _ in range(3):
            k = int(rng.integers(40, 71))
            p = lo + int(rng.integers(0, L - k))
            t[p:p + k] = int(symbols[int(rng.integers(0, len(symbols)))])
    elif L >= 8:
        t[lo + L // 4:lo + L // 4 + L // 2] = int(symbols[int(rng.integers(0, len(symbols)))])


def _text(kind: str, n: int, seed: int, alphabet: bytes = WIDE20) -> bytes:
    """A text of n bytes, the final '$' included.
    acgt  random ACGT with planted runs (the 2-bit string sort, packed rank)
    gaps  the same with an N run and single R / Y (the 3-bit string sort)
    wide  random symbols of `alphabet`, every one present once n allows it
          (the general doubling; more than 16 symbols: k_occ_blocks)"""
    rng = np.random.default_rng(seed * 1_000_003 + n)
    L = n - 1
    if kind == "wide":
        a = np.frombuffer(alphabet, dtype=np.uint8)
        t = a[rng.integers(0, len(a), L)].copy()
        lo = 0
        if L >= len(a):
            t[:len(a)] = rng.permutation(a)
            lo = len(a)
        _runs(rng, t, lo, a)
    else:
        a = np.frombuffer(b"ACGT", dtype=np.uint8)
        t = a[rng.integers(0, 4, L)].copy()
        _runs(rng, t, 0, a)
        if kind == "gaps" and L >= 1:
            k = max(1, min(45, L // 3))
            p = int(rng.integers(0, L - k + 1))
            t[p:p + k] = ord("N")
            if L >= 6:
                t[int(rng.integers(0, L))] = ord("R")
                t[int(rng.integers(0, L))] = ord("Y")
    return t.tobytes() + b"$"


def _check_index(text: bytes, sa: int = 32, occ: int = 128):
    """Every array of BWTCore(text, sa, occ) equals oracle.Index(text, sa, occ)'s
    (test_gpu.py's _check_index, with the rates, the Occ row length and the
    alphabet's keys checked as well); returns (core, oracle index)."""
    from bwtmi import BWTCore
    from bwtmi._lib import lib
    core = BWTCore(text.decode("ascii"), sa, occ)
    ref = oracle.Index(text, sa, occ)
    n = len(text)
    tag = (n, sa, occ)
    assert (core.suffix_array == ref.sa).all(), tag
    assert (core.bwt_arr == ref.bwt).all(), tag
    occ_len = 1 + n // occ + (n % occ != 0)
    assert lib().bwtmi_index_occ_len(core._h) == occ_len == ref.occ.shape[1], tag
    cp = core.occ_checkpoints
    assert sorted(cp) == ref.alphabet(), tag
    for c in ref.alphabet():
        assert cp[c].shape == (occ_len,) and (cp[c] == ref.occ[c]).all(), tag + (c,)
        assert core.char_counts[chr(c)] == ref.C[c] and core.char_totals[chr(c)] == ref.totals[c], tag + (c,)
    assert lib().bwtmi_index_sampled_len(core._h) == len(ref.sampled_sa) == -(-n // sa), tag
    assert core.sampled_sa == ref.sampled_sa, tag
    off, pos = core.kmer_csr()
    assert (off == ref.kmer_offsets).all() and (pos == ref.kmer_pos).all(), tag
    assert (core.lcp_array() == ref.lcp()).all(), tag
    return core, ref


class _Launches:
    """with _Launches(ctx) as k: ...; k.count(name) = launches of that kernel
    inside the block (the library's kernel statistics, every kernel timed)."""

    def __init__(self, ctx):
        self.ctx, self.stats = ctx, {}

    def __enter__(self):
        from bwtmi import _lib
        _lib.kernel_stats_filter(self.ctx, "")
        _lib.kernel_stats(self.ctx, enable=True, reset=True)
        return self

    def __exit__(self, *exc):
        from bwtmi import _lib
        self.stats = _lib.kernel_stats(self.ctx, enable=False, reset=True)
        return False

    def count(self, name):
        return self.stats.get(name, (0.0, 0, 0.0))[1]


def _three_searches(gpu_ctx, core, pats, fm_bytes):
    """backward_search_batch, locate_batch (k = 1) and smem_batch of pats under
    BWTMI_FM_BYTES=fm_bytes: the kernel launches, and every array returned."""
    from bwtmi import _lib
    with _lib.knobs(FM_BYTES=fm_bytes), _Launches(gpu_ctx) as k:
        iv = core.backward_search_batch(pats)
        loc = core.locate_batch(pats, max_mismatches=1, both_strands=True)
        sm = core.smem_batch(pats, min_len=8, both_strands=True)
    arrays = [iv, loc.offsets, loc.positions, loc.mismatches, loc.strand, sm.offsets, sm.qstart, sm.qend, sm.strand,
              sm.count, sm.pos_offsets, sm.positions]
    return k, [np.asarray(a).tolist() for a in arrays] + [int(loc.candidates), int(sm.positions_total), int(sm.work)]


@pytest.mark.parametrize("case", ["packed", "bytes-by-knob", "bytes-by-text"])
def test_rank_path_dispatch_of_the_three_searches(gpu_ctx, case):
    """The choice of rank path (search.hip, with_rank) as each of the three
    searches makes it: one launch of the chosen path's seed kernel under its
    statistics name and none of its twin -- the packed rank on an ACGT text,
    the byte rank on the same text under BWTMI_FM_BYTES=1 and on a gap text,
    which has no packed rank -- and the two paths return the same on the ACGT
    text."""
    from bwtmi import BWTCore
    text = _text("gaps" if case == "bytes-by-text" else "acgt", 2001, 4242)
    rng = np.random.default_rng(99)
    pats = []
    for _ in range(20):
        m = int(rng.integers(12, 41))
        a = int(rng.integers(0, len(text) - 1 - m))
        pats.append(text[a:a + m].decode())
    core = BWTCore(text, 32, 128)
    fm_bytes = int(case == "bytes-by-knob")
    k, got = _three_searches(gpu_ctx, core, pats, fm_bytes)
    for name in ("k_bsearch", "k_loc_seed", "k_smem_ms"):
        mine, twin = (name + "2", name) if case == "packed" else (name, name + "2")
        assert k.count(mine) == 1 and k.count(twin) == 0, (case, name, k.stats.keys())
    assert all(sp >= 0 for sp, _ in got[0])           # every pattern was cut from the text
    if case != "bytes-by-text":
        _, other = _three_searches(gpu_ctx, core, pats, 1 - fm_bytes)
        assert got == other


# ------------------------------------------------------------------ Occ checkpoints
OCC_RATES = [1, 7, 16, 32, 48, 64, 100, 128, 129, 256, 512, 1024, 2048]


def _occ_sizes(occ):
    """Text lengths of the Occ sweep: a last 16-byte piece of 1, 7, 8, 9 and 15
    bytes, n % occ of 0, 1 and occ - 1, n < occ, n < 16, and the end of a
    256-lane workgroup of k_occ_groups (4096 = 256 x 16)."""
    ns = {1, 2, 9, 15, 16, 17, 24, 25, occ - 1, occ, occ + 1, 2 * occ, 2 * occ + 8, 4095, 4096, 4097, 4105, 5000}
    return sorted(n for n in ns if n >= 1)


def _occ_arm(occ, sigma):
    """The kernel and path index_build_device takes for this rate and alphabet."""
    if 16 <= occ <= 1024 and occ & (occ - 1) == 0 and sigma <= 16:
        return f"groups<{occ // 16}>"
    return "blocks:bytes" if occ % 16 else "blocks:swar" if sigma <= 16 else "blocks:swar+bytes"


@pytest.mark.parametrize("kind", ["acgt", "gaps", "wide"])
@pytest.mark.parametrize("occ", OCC_RATES)
def test_occ_rates_vs_oracle(gpu_ctx, occ, kind):
    """Every arm of the occ_sample switch and the three paths of k_occ_blocks,
    fed by each of the three suffix sorts.  One "occ_blocks" launch per build:
    no build was skipped."""
    sizes = _occ_sizes(occ)
    arms = set()
    with _Launches(gpu_ctx) as k:
        for n in sizes:
            _, ref = _check_index(_text(kind, n, occ), 32, occ)
            sigma = len(ref.alphabet())
            if kind == "wide" and n >= 24:
                assert sigma == 21        # past kMaxSig = 16
            if kind != "wide":
                assert sigma <= 8
            arms.add(_occ_arm(occ, sigma))
    assert k.count("occ_blocks") == len(sizes)
    # the wide texts stand on both sides of kMaxSig: the short ones hold <= 16 symbols
    assert arms == {_occ_arm(occ, 5)} | ({_occ_arm(occ, 21)} if kind == "wide" else set())


# ------------------------------------------------------------------ sampled SA
@pytest.mark.parametrize("kind", ["acgt", "gaps", "wide", "gaps-general"])
def test_sa_sample_rates_vs_oracle(gpu_ctx, kind):
    """sampled_len = ceil(n / sa_sample) of 1, n and values not derived from 32:
    written by the string sorts' last pass (dna_final: ACGT and the small
    alphabet) and by k_sample after the general doubling (a 21-symbol text,
    and a gap text with BWTMI_SA_SMALL=0).  "$" alone goes to the doubling, and so
    may a text of under 9 bytes whose first keys tie with the zero-padded end
    ("N$": sa_sort gives up at h >= 2 n); from 33 bytes on the path is fixed."""
    from bwtmi import _lib
    total = 0
    with _lib.knobs(SA_SMALL=0 if kind == "gaps-general" else 1):
        for n in (1, 2, 33, 1000, 5000):
            text = _text(kind.split("-")[0], n, 77)
            builds = 0
            with _Launches(gpu_ctx) as k:
                for sa in sorted({1, 2, 7, 31, 32, 33, 1000, n - 1, n, n + 1}):
                    if sa <= 0:
                        continue
                    core, _ = _check_index(text, sa, 128)
                    assert list(core.sampled_sa) == list(range(0, n, sa))
                    builds += 1
            print(kind, n, "builds", builds, "dna_final", k.count("dna_final"), "k_sample", k.count("k_sample"))
            assert k.count("dna_final") + k.count("k_sample") == builds, n
            if n == 1 or kind in ("wide", "gaps-general"):
                assert k.count("k_sample") == builds, n
            elif n >= 33:
                assert k.count("dna_final") == builds, n
            total += builds
    assert total >= 40


# ------------------------------------------------------------------ wide alphabets
@pytest.mark.parametrize("sigma", [15, 16, 17, 18, 33, 41, 64, 65, 66, 94])
def test_wide_alphabets_vs_oracle(gpu_ctx, sigma):
    """sigma symbols, '$' included: sa_doubling packs 64 / b symbols of b bits
    (b = bits for sigma + 1 codes: 4, 5, 6 and 7 here) into its first key, and
    the Occ build leaves k_occ_groups for k_occ_blocks past 16 symbols.  A
    random 3000-byte text with every symbol present, and alphabet * 40 (long
    ties in the doubling); bytes below '$' and, at 94, lower case.  Past 64
    symbols the Occ rows outgrow one launch of the row scan (64 rows): 94
    symbols were refused as a bad argument until the scan took them in pieces,
    and 64 / 65 / 66 stand on both sides of that split."""
    alpha = PRINTABLE[:sigma - 1]
    b = {15: 4, 16: 5, 17: 5, 18: 5, 33: 6, 41: 6, 64: 7, 65: 7, 66: 7, 94: 7}[sigma]
    assert (1 << (b - 1)) < sigma + 1 <= (1 << b)
    with _Launches(gpu_ctx) as k:
        for occ in (128, 100):
            for text in (_text("wide", 3000, sigma, alpha), alpha * 40 + b"$"):
                _, ref = _check_index(text, 32, occ)
                assert len(ref.alphabet()) == sigma
    assert k.count("sa_init_keys") == 4 and k.count("k_sample") == 4 and k.count("occ_blocks") == 4


# ------------------------------------------------------------------ consumers of the byte rank
def _search_patterns(text: bytes):
    s = text.decode()
    pats = ["".join(m) for k in range(1, 5) for m in itertools.product("ACGT", repeat=k)]
    return pats + ["ACGTACGTAC", "N", "", "TTTTTTTTTT", "GATTACA", "$", "A$", "$A", "C$", s[-9:], s[:12], s[100:164],
                   "ACGN"]


@pytest.mark.parametrize("kind", ["acgt", "gaps"])
@pytest.mark.parametrize("occ", [1, 16, 100, 2048])
def test_backward_search_byte_rank_at_other_rates(gpu_ctx, occ, kind):
    """d_rank (k_bsearch) with a block of 1, 16, 100 and 2048 bytes -- pos / k,
    a tail of up to k - 1 bytes, checkpoint n / k at pos == n -- on an ACGT text
    under BWTMI_FM_BYTES=1 and on a gap text, which has no packed rank."""
    from bwtmi import BWTCore, _lib
    text = _text(kind, 5001, 300 + occ)
    pats = _search_patterns(text)
    core = BWTCore(text, 32, occ)
    ref = oracle.Index(text, 32, occ)
    with _lib.knobs(FM_BYTES=int(kind == "acgt")), _Launches(gpu_ctx) as k:
        got = core.backward_search_batch(pats)
    assert k.count("k_bsearch") == 1 and k.count("k_bsearch2") == 0
    found = 0
    for p, (sp, ep) in zip(pats, got.tolist()):
        assert (sp, ep) == ref.backward_search(p.encode()), (occ, p)
        found += sp >= 0
    assert found > 300


@pytest.mark.parametrize("occ", [1, 16, 100, 2048])
def test_rank_every_position(gpu_ctx, occ):
    """BWTCore.rank(c, pos) over the device's checkpoints and BWT for every
    present symbol and every pos in -1 .. n + 1, against prefix counts."""
    from bwtmi import BWTCore
    text = _text("gaps", 300, occ)
    n = len(text)
    core = BWTCore(text, 32, occ)
    bwt = oracle.Index(text, 32, occ).bwt
    for c in sorted(set(text)):
        prefix = np.concatenate([[0], np.cumsum(bwt == c)])
        for pos in range(-1, n + 2):
            want = int(prefix[min(max(pos, 0), n)])
            assert core.rank(c, pos) == want and core.rank(chr(c), pos) == want, (occ, c, pos)
    assert core.rank(ord("X"), 17) == 0


# ------------------------------------------------------------------ arguments
def test_sample_rates_below_one_are_argument_errors(gpu_ctx, built_lib):
    from bwtmi import BWTCore
    from bwtmi._lib import BwtmiError
    text = np.frombuffer(b"ACGTACGT$", dtype=np.uint8)
    for sa, occ in ((0, 128), (-1, 128), (32, 0), (32, -1)):
        out = C.c_void_p(0x5A5A)
        rc = built_lib.bwtmi_index_build(gpu_ctx, text.ctypes.data_as(C.c_void_p), text.size, sa, occ, 0, C.byref(out))
        assert rc == -1                                   # BWTMI_E_ARG
        assert built_lib.bwtmi_last_error()
        assert out.value == 0x5A5A                        # *out untouched
        with pytest.raises(BwtmiError):
            BWTCore(text.tobytes(), sa, occ)
    ok = C.c_void_p()
    assert built_lib.bwtmi_index_build(gpu_ctx, text.ctypes.data_as(C.c_void_p), text.size, 1, 1, 0, C.byref(ok)) == 0
    assert ok.value and built_lib.bwtmi_index_sampled_len(ok) == 9 and built_lib.bwtmi_index_occ_len(ok) == 10
    assert built_lib.bwtmi_index_free(ok) == 0


# ------------------------------------------------------------------ the worker path's --sa-sample
def _golden_sha(golden_dir, name):
    with open(os.path.join(golden_dir, "expected_cli.json")) as f:
        return json.load(f)[name]["sha256"]


def test_job_index_sample_rate_leaves_output_unchanged(gpu_ctx, built_lib, golden_dir):
    """The job's background index builds (one per contig, behind the scan) at
    sa_sample 1, 7 and 1000: they finish without error and the rendered
    records are the sa_sample = 32 run's, the reference golden's."""
    from bwtmi.records import Job
    fa = os.path.join(golden_dir, "inputs", "test2.fa")
    out = {}
    for s in (32, 1, 7, 1000):
        job = Job(min_copies=3, show_progress=True, build_index=True, sa_sample=s)
        job.load_fasta(fa, 30, dev_ctx=gpu_ctx)
        job.upload(gpu_ctx)
        job.scan(gpu_ctx)
        assert built_lib.bwtmi_job_wait(gpu_ctx, job.h) == 0, built_lib.bwtmi_last_error()
        assert not job.contig_errors()
        job.postprocess()
        out[s] = job.render("strfinder")
    assert hashlib.sha256(out[32]).hexdigest() == _golden_sha(golden_dir, "test2.fa.strfinder")
    for s in (1, 7, 1000):
        assert out[s] == out[32], s


def test_cli_sa_sample(gpu_ctx, golden_dir, tmp_path):
    here = os.path.dirname(os.path.abspath(__file__))
    bwt = os.path.join(here, "..", "bwt-algorithm_amd", "bwt.py")
    out = tmp_path / "repeat.tab"
    subprocess.run([sys.executable, bwt, os.path.join(golden_dir, "inputs", "test.fa"), "-o", str(out),
                    "--jobs", "0", "--sa-sample", "7"], check=True, capture_output=True)
    assert hashlib.sha256(out.read_bytes()).hexdigest() == _golden_sha(golden_dir, "test.fa.strfinder")
