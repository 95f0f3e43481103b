"""The library finders' kernels (library.hip: k_extend_cols, k_seed_flags,
k_simple_extend, k_t1_flags, k_plateau_*) on the inputs the other suites leave
out: N / IUPAC / other bytes in short imperfect arrays, a side list past its
first capacity, periods 63..200 of the simple scan, columns of more symbols
than a lane keeps, arrays at either end of the text, tiny Tier 1 texts and
plateau thresholds other than 20.

tests/golden/library_edges.json holds the reference's own records
(make_goldens.py library_edges; each case names the finder it targets).  CPU
tests pin the oracle restatement (oracle/library.py) to them on every field;
GPU tests check the device path against both, and read the counters that the
finders print under BWTMI_STATS=1 to show that the path a case is about was
taken.

The simple-scan fixtures walk only the periods around the planted one (the
reference needs 8 to 25 s for all of 1..200 on these texts, too close to its
30 s wall-clock stop); the full walk with default parameters is checked
against the oracle alone.  Oracle time of the slowest case of each family,
measured on the CPU: short imperfect 1.5 s (the 9 kbp dense-'R' text; the
motif enumeration alone is 0.9 s, and 3 s where a text shorter than 8 bases
leaves no k-mer table), simple scan with default parameters 3.5 s (period
200), Tier 1 and plateaus below 0.01 s, the 70,000-base homopolymer 1.1 s.
"""
import json
import os
import re
import sys

import numpy as np
import pytest

import oracle
from oracle import library as olib

from test_library import DEV_FIELDS, FIELDS, _as_dicts, _cmp, _finder
from test_simple import _device as _simple_device
from test_simple import _oracle as _simple_oracle

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
from make_goldens import MANY_SYMBOLS, SIMPLE_EDGE_PERIODS, _flank, _library_edge_cases  # noqa: E402

CASES = _library_edge_cases()
PLATEAU_FIELDS = ("start", "end", "motif", "copies", "length", "tier", "confidence")


def _names(finder):
    return [k for k, c in CASES.items() if c["finder"] == finder]


@pytest.fixture(scope="module")
def edges(golden_dir):
    with open(os.path.join(golden_dir, "library_edges.json")) as f:
        return json.load(f)


def _text(case) -> bytes:
    return case["seq"].encode() + b"$"


_ORACLE = {}


def _oracle_records(name, case):
    """The oracle's records of a fixture case, computed once per session."""
    if name not in _ORACLE:
        t, kw, finder = _text(case), case["params"], case["finder"]
        if finder == "short_imperfect":
            got = olib.short_imperfect(name, t, oracle.Index(t))
        elif finder == "tier1":
            got = olib.tier1_find_strs(name, t)
        elif finder == "lcp_plateaus":
            idx = oracle.Index(t)
            got = olib.lcp_plateaus(name, t, idx.sa, idx.lcp(), **kw)
        else:
            got = _simple_oracle(name, case["seq"].encode(), kw, [])
        _ORACLE[name] = got
    return _ORACLE[name]


# --------------------------------------------------------------- oracle vs reference
def test_fixture_holds_the_generators_cases(edges):
    """The texts the GPU tests build are the ones the reference ran on, and it
    raised on none of them (a case it raises on would be recorded and neither
    side called)."""
    assert list(edges) == list(CASES)
    for name, case in CASES.items():
        for k in ("finder", "seq", "params", "tier1_seen"):
            assert edges[name][k] == case[k], (name, k)
        assert edges[name]["raises"] is None, name
        assert len(case["seq"]) <= 3000 or name == "si_dense_R"
        if case["finder"] == "simple":
            assert edges[name]["seconds"] <= 5, name     # far below the reference's 30 s stop


@pytest.mark.parametrize("finder", ["short_imperfect", "simple", "tier1", "lcp_plateaus"])
def test_oracle_matches_reference_on_edges(edges, finder):
    fields = PLATEAU_FIELDS if finder == "lcp_plateaus" else FIELDS
    some = 0
    for name in _names(finder):
        want = edges[name]["records"]
        _cmp(_oracle_records(name, edges[name]), want, fields)
        some += len(want)
    assert some


def test_oracle_extension_votes_on_N():
    """Known answers of _extend_tandem_fm's vote: N ties with a base at two
    copies -- the smaller byte is the consensus and the other one a
    transversion of it either way, so the copy is refused; a column of N in
    every copy costs nothing; a byte outside 65..84 is of N's class, so it
    mismatches N without being a transversion."""
    assert olib.extend(b"CAGTCCTACAGTNCTA$", 0, 8) == (0, 8, 1)      # C < N: consensus C, N refused
    assert olib.extend(b"CAGTTCTACAGTNCTA$", 0, 8) == (0, 8, 1)      # N < T: consensus N, T refused
    assert olib.extend(b"CANTCCTACANTCCTACANTCCTA$", 0, 8) == (0, 24, 3)
    assert olib.extend(b"CANTCCTACAYTCCTACANTCCTA$", 0, 8) == (0, 24, 3)
    assert olib.extend(b"CANTCCTACARTCCTACANTCCTA$", 0, 8) == (0, 8, 1)      # R is a class of its own


# --------------------------------------------------------------------- device
_EXT = re.compile(r"extension kernel [\d.]+ ms \((\d+) side entries, (\d+) relaunches")
_SI = re.compile(r"short_imperfect: .*; (\d+) side entries, (\d+) unbinned\)")
_SIMPLE = re.compile(r"simple scan: \d+ walks, \d+ rounds, (\d+) requests, (\d+) host redos")


def _short_stats(capfd, f, name, seen=frozenset()):
    """records and (side entries, unbinned side entries, relaunches) of one call."""
    from bwtmi import _lib
    capfd.readouterr()
    with _lib.knobs(STATS=1):
        got = _as_dicts(f.find_short_imperfect_repeats(name, set(seen)))
    err = capfd.readouterr().err
    ext, si = _EXT.findall(err), _SI.findall(err)
    assert len(ext) == 1 and len(si) == 1, err
    side, unbinned = (int(x) for x in si[0])
    assert int(ext[0][0]) == side
    return got, side, unbinned, int(ext[0][1])


def _dollar_entries(t: bytes) -> int:
    """Extension entries (start cs, unit L <= 9) of a text whose only byte outside
    A C G N T is the final '$' that read it: the unit itself ends on it (cs + L
    == n), or the right extension -- which tries the copies at cs + L, cs + 2L,
    ... for as long as the one before was taken -- comes to the copy that ends
    at n.  That needs (n - cs) % L == 0 and every copy before it taken, which
    is what the oracle's extension of the text without its '$' reports as an
    end of n - L.  (The left extension runs away from the '$'.)"""
    n, body, cnt = len(t), t[:-1], 0
    for L in range(1, 10):
        for cs in range(0, n - L + 1):
            if cs + L == n:
                cnt += 1
            elif (n - cs) % L == 0 and olib.extend(body, cs, L)[1] == n - L:
                cnt += 1
    return cnt


SI_EMPTY = {"si_short8", "si_short7", "si_one"}        # too short for three copies of a >= 2-base unit


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names("short_imperfect"))
def test_device_short_imperfect_edges(gpu_ctx, edges, capfd, name):
    case = edges[name]
    t, seq = _text(case), case["seq"]
    want = _oracle_records(name, case)
    assert bool(want) == (name not in SI_EMPTY)
    got, side, unbinned, relaunches = _short_stats(capfd, _finder(seq), name)
    _cmp(got, want, DEV_FIELDS)
    _cmp(got, case["records"], DEV_FIELDS)
    spans = [(w["start"], w["end"]) for w in want]
    if set(seq) <= set("ACGTN"):
        # only the '$' is unbinned: the host's scalar extension ran for exactly the entries that read it
        assert unbinned == _dollar_entries(t)
        assert side == unbinned                          # no count near 0xffff either
    if name == "si_subs_N":
        assert any("N" in w["motif"] for w in want)      # a column the N bin wins
        # the arrays with N in one copy only are cut there, and a cut array is not maximal: no record
        assert not any(w["motif"] in ("CAGTCCTA", "GATTCAGCA") for w in want)
    if name in ("si_subs_NRY", "si_subs_low_high"):
        others = set(seq) - set("ACGTN")
        assert any(others & set(w["motif"]) for w in want)
        # at least the entries whose own unit holds such a byte went to extend_host; the records
        # come from both that and the kernel's binned path
        own = sum(1 for L in range(1, 10) for cs in range(len(t) - L + 1) if set(t[cs:cs + L]) - set(b"ACGNT"))
        assert own > 1000 and own <= unbinned < 65536
    if name == "si_dense_R":
        assert side > 65536 and unbinned > 65536 and relaunches >= 1
    else:
        assert relaunches == 0
    if name in ("si_ends", "si_ends_b"):
        assert any(s == 0 for s, e in spans) and any(e == len(seq) for s, e in spans)
    if name in ("si_n66", "si_n67", "si_n130", "si_n131"):
        assert any(s <= 63 and e > 64 for s, e in spans)           # across the first ballot word's edge
        assert (len(t) + 63) // 64 * 64 > len(t)                   # the last word is partial
    if name in ("si_n130", "si_n131"):
        assert any(s <= 127 and e > 128 for s, e in spans)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["first_base", "last_base", "just_before", "just_after"])
def test_device_short_imperfect_seen_on_array_boundaries(gpu_ctx, edges, which):
    """tier1_seen intervals that start or end exactly on an array's first or
    last base (the interval is half-open: `start <= p < end`)."""
    name = "si_ends"
    t = _text(edges[name])
    idx = oracle.Index(t)
    base = _oracle_records(name, edges[name])
    assert len(base) == 3
    seen = {"first_base": {(w["start"], w["start"] + 1) for w in base},
            "last_base": {(w["end"] - 1, w["end"]) for w in base},
            "just_before": {(max(0, w["start"] - 4), w["start"]) for w in base},
            "just_after": {(w["end"], w["end"] + 4) for w in base}}[which]
    want = olib.short_imperfect(name, t, idx, tier1_seen=seen)
    assert want
    got = _as_dicts(_finder(edges[name]["seq"]).find_short_imperfect_repeats(name, seen))
    _cmp(got, want, DEV_FIELDS)


@pytest.mark.gpu
def test_device_short_imperfect_long_homopolymer(gpu_ctx, capfd):
    """70,000 'A's: the unit-1 entries inside the run count 65,535 copies or more
    on one side and go to the side list as binned entries.  No record the
    oracle can produce in test time depends on the counts they carry (a
    one-base motif never passes the entropy filter), so this shows only that
    the path runs and disturbs nothing else."""
    r = np.random.default_rng(5)
    u = "ACGGTCAT"
    seq = _flank(r, 200, "C") + "A" * 70000 + _flank(r, 200, u, "A") + u * 6 + _flank(r, 100, "", u)
    t = seq.encode() + b"$"
    want = olib.short_imperfect("c", t, oracle.Index(t))
    assert any(w["motif"] == u for w in want)
    got, side, unbinned, relaunches = _short_stats(capfd, _finder(seq), "c")
    _cmp(got, want, DEV_FIELDS)
    assert side - unbinned > 0
    # the last 300 bases are the array and a random flank: no extension from before them reaches the '$'
    assert unbinned == _dollar_entries(t[-300:])


# ------------------------------------------------------------------ simple scan
def _simple_stats(capfd, name, seq, params):
    from bwtmi import _lib
    capfd.readouterr()
    with _lib.knobs(STATS=1):
        got = _simple_device(name, seq, params, [])
    found = _SIMPLE.findall(capfd.readouterr().err)
    assert len(found) == 1, found
    return got, int(found[0][0]), int(found[0][1])


def _planted_period(name):
    m = re.search(r"_p(\d+)", name)
    return int(m.group(1)) if m else None


def _check_period_records(name, want):
    """The planted array's record: all of its copies (four; three for periods
    from 191, so that the text stays short), or only those before the first
    substituted copy when the period is past the mismatch-tolerant range --
    three of four, and two of three, where the array passes for its partial
    third copy of 0.85 alone."""
    p = _planted_period(name)
    if p is None:
        return
    hit = [w for w in want if len(w["motif"]) == p]
    assert hit, (name, [(w["start"], w["end"], len(w["motif"])) for w in want])
    planted = 4.0 if p <= 129 else 3.0
    if name.endswith("_sub") and p >= 65:
        assert all(w["copies"] == planted - 1 for w in hit)
    elif name.endswith(("_sub", "_exact")):
        assert all(w["copies"] >= planted for w in hit)


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names("simple"))
def test_device_simple_scan_edges(gpu_ctx, edges, capfd, name):
    case = edges[name]
    seq = case["seq"]
    want = _oracle_records(name, case)
    assert want
    _check_period_records(name, want)
    got, nreq, redos = _simple_stats(capfd, name, seq, case["params"])
    _cmp(got, want)
    _cmp(got, case["records"])
    assert nreq > 0
    if name == "simple_syms10":
        assert redos >= 1            # a column of 10 symbols: the lane keeps 6, the host redoes the request
    else:
        assert redos == 0            # simple_syms6 included: exactly 6 symbols stay on the device
    if name.startswith("simple_n1k"):
        assert 1000 < len(seq) <= 3000
    elif _planted_period(name):
        assert len(seq) <= 1000
    spans = [(w["start"], w["end"]) for w in want]
    if name.startswith("simple_ends"):
        assert any(s == 0 for s, e in spans) and any(e == len(seq) for s, e in spans)
    if name == "simple_partial_p70":
        assert [w["copies"] for w in want] == [2.0]      # taken for its partial third copy alone


@pytest.mark.gpu
@pytest.mark.parametrize("sub", [False, True], ids=["exact", "sub"])
@pytest.mark.parametrize("p", SIMPLE_EDGE_PERIODS + (1065, 1100))
def test_device_simple_scan_periods_full_walk(gpu_ctx, capfd, p, sub):
    """The same texts with default parameters: every period from 1 is walked, so
    the planted array meets the walks of its divisors and neighbours first
    (1065 and 1100: periods 65 and 100 in a text of 1001..3000 bases)."""
    name = f"simple_n1k_p{p - 1000}" if p > 1000 else f"simple_p{p}"
    name += "_sub" if sub else "_exact"
    seq = CASES[name]["seq"]
    want = _simple_oracle(name, seq.encode(), {}, [])
    _check_period_records(name, want)
    got, nreq, redos = _simple_stats(capfd, name, seq, {})
    _cmp(got, want)
    assert redos == 0


def test_many_symbol_columns_are_what_they_claim(edges):
    """Column 5 of the 60-base unit holds 10 (6) distinct bytes over the 10
    copies, every other column one: more than (exactly) what a lane keeps."""
    assert len(set(MANY_SYMBOLS)) == 10
    for name, k in (("simple_syms10", 10), ("simple_syms6", 6)):
        seq = edges[name]["seq"]
        cols = [{seq[40 + 60 * c + q] for c in range(10)} for q in range(60)]
        assert len(cols[5]) == k and all(len(x) == 1 for q, x in enumerate(cols) if q != 5)


# ----------------------------------------------------------------------- Tier 1
def _t1_expect_records(name):
    """Whether Tier 1 has a record: three copies fit when the text holds 3L bases
    (the walk runs while i < n - L with the '$' counted in n); a one-base
    motif has entropy 0 and these runs are shorter than 10."""
    m = re.match(r"t1_L(\d)_n(\d+)", name)
    if m:
        L, n = int(m.group(1)), int(m.group(2))
        return L >= 2 and n >= 3 * L
    return name not in ("t1_AN", "t1_A9", "t1_AAC3")


@pytest.mark.gpu
def test_device_tier1_edges(gpu_ctx, edges):
    from bwtmi.tiers import Tier1STRFinder
    for name in _names("tier1"):
        case = edges[name]
        want = _oracle_records(name, case)
        assert bool(want) == _t1_expect_records(name), name
        t = np.frombuffer(_text(case), dtype=np.uint8)
        got = _as_dicts(Tier1STRFinder(t, 9).find_strs(name))
        _cmp(got, want, DEV_FIELDS)
        _cmp(got, case["records"], DEV_FIELDS)
    rec = {n: [(w["start"], w["end"], w["motif"]) for w in _ORACLE[n]] for n in _names("tier1")}
    assert rec["t1_N_inside"] == [(0, 9, "ACG"), (10, 22, "ACG")]
    assert rec["t1_A10"] == [(2, 12, "AA")] and rec["t1_AAC4"] == [(2, 14, "AAC")]
    assert rec["t1_at_end"] == [(4, 16, "ACG")]              # up to the last base before '$'
    assert rec["t1_iupac"] == [(26, 38, "CAT")]              # neither the 'R' nor the lower-case array


# ----------------------------------------------------------------- LCP plateaus
PL_EMPTY = {"pl_minp30", "pl_minp30_no_runs", "pl_all_A", "pl_n2"}


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names("lcp_plateaus"))
def test_device_lcp_plateaus_edges(gpu_ctx, edges, name):
    case = edges[name]
    t, kw = _text(case), case["params"]
    idx = oracle.Index(t)
    lcp = idx.lcp()
    want = _oracle_records(name, case)
    assert bool(want) == (name not in PL_EMPTY)
    f = _finder(case["seq"])
    for k, v in kw.items():
        setattr(f, k, v)
    dev_lcp = f._compute_lcp_array()
    assert np.array_equal(np.asarray(dev_lcp, dtype=np.int64), np.asarray(lcp, dtype=np.int64))
    got = _as_dicts(f._detect_lcp_plateaus(dev_lcp, name))
    _cmp(got, want, PLATEAU_FIELDS)
    _cmp(got, case["records"], PLATEAU_FIELDS)
    # the threshold the case is about
    lmax = int(lcp.max())
    thr = max(kw.get("min_period", 1), min(kw.get("max_period", 1000), lmax, 20))
    expect = {"pl_maxp5": 5, "pl_maxp19": 19, "pl_minp21": 21, "pl_minp30": 30}.get(name, 20)
    if name == "pl_minp30":
        assert lmax == 56
    if name == "pl_minp30_no_runs":
        assert lmax < 30                                      # no position reaches the threshold
    elif name == "pl_n2":
        assert lmax == 0
    else:
        assert thr == expect
        assert all(w["length"] == w["copies"] * thr for w in want)
    # An array at the text's start or end: every member of a progression has an LCP >= thr, so
    # thr bytes follow it and no record runs past the text (k_plateau_eval's `sp + thr <= n` and
    # `min(c * thr, n - sp)` never decide); the run's first suffix is not among sa[i:j], so the
    # reference's records start one unit inside the array.  What is checked is the agreement.
    if name in ("pl_start", "pl_end"):
        a0 = 0 if name == "pl_start" else len(case["seq"]) - 120
        assert all(a0 <= w["start"] and w["end"] <= a0 + 120 for w in want)
    if name == "pl_two_arrays":
        assert len({w["motif"] for w in want}) > 20           # rotations of both units: several runs
