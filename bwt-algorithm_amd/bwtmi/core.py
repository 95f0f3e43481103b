"""BWTCore -- the reference's FM-index class (bwt.py:98-427) over the device
index built by libbwtmi (suffix array, BWT, C, Occ checkpoints, sampled SA
and 8-mer hash all constructed by HIP kernels on gfx950).  Host copies of
the arrays are fetched lazily, on first attribute access.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib
from ._lib import check, lib


class _LazyText:
    """`BWTCore.text` for an index built from bytes: the str is decoded on
    first use only (nothing on the CLI path reads it)."""

    def __init__(self, raw: bytes):
        self._raw, self._s = raw, None

    def _str(self) -> str:
        if self._s is None:
            self._s = self._raw.decode("latin-1")
        return self._s

    def __len__(self):
        return len(self._raw)

    def __str__(self):
        return self._str()

    def __eq__(self, other):
        return self._str() == (str(other) if isinstance(other, _LazyText) else other)

    def __hash__(self):
        return hash(self._str())

    def __getitem__(self, k):
        return self._str()[k]

    def __iter__(self):
        return iter(self._str())

    def __contains__(self, x):
        return x in self._str()

    def __getattr__(self, name):
        return getattr(self._str(), name)


class LocateResult:
    """Hits of BWTCore.locate_batch: `offsets` (int64[npat + 1]) into `positions`
    (int64), `mismatches` (uint8) and `strand` (uint8, 0 = '+', 1 = '-');
    result[i] = the three slices of pattern i, sorted by (position, strand).
    `candidates` is the call's candidate count (what max_candidates caps)."""

    __slots__ = ("offsets", "positions", "mismatches", "strand", "candidates")

    def __init__(self, offsets, positions, mismatches, strand, candidates=0):
        self.offsets, self.positions, self.mismatches, self.strand = offsets, positions, mismatches, strand
        self.candidates = candidates

    def __len__(self):
        return self.offsets.size - 1

    def __getitem__(self, i: int):
        if not -len(self) <= i < len(self):
            raise IndexError(i)
        i %= len(self)
        a, b = int(self.offsets[i]), int(self.offsets[i + 1])
        return self.positions[a:b], self.mismatches[a:b], self.strand[a:b]


class SmemResult:
    """SMEMs of BWTCore.smem_batch: `offsets` (int64[nq + 1]) into `qstart`,
    `qend` (int32), `strand` (uint8, 0 = '+', 1 = '-') and `count` (int64);
    `pos_offsets` (int64[nsmem + 1]) into `positions` (int64, ascending per
    SMEM, empty where count > max_occ).  result[i] = (qstart, qend, strand,
    count, positions per SMEM) of query i, its SMEMs by (strand, qstart).
    `positions_total` is the call's position count (what max_positions caps),
    `work` the sum of the matching statistics (smem_batch's rank steps),
    `steps` the rank steps smem_long_batch really took (0 from smem_batch)."""

    __slots__ = ("offsets", "qstart", "qend", "strand", "count", "pos_offsets", "positions", "positions_total",
                 "work", "steps")

    def __init__(self, offsets, qstart, qend, strand, count, pos_offsets, positions, positions_total=0, work=0,
                 steps=0):
        self.offsets, self.qstart, self.qend, self.strand, self.count = offsets, qstart, qend, strand, count
        self.pos_offsets, self.positions = pos_offsets, positions
        self.positions_total, self.work, self.steps = positions_total, work, steps

    def __len__(self):
        return self.offsets.size - 1

    def __getitem__(self, i: int):
        if not -len(self) <= i < len(self):
            raise IndexError(i)
        i %= len(self)
        a, b = int(self.offsets[i]), int(self.offsets[i + 1])
        po = self.pos_offsets
        return (self.qstart[a:b], self.qend[a:b], self.strand[a:b], self.count[a:b],
                [self.positions[int(po[j]):int(po[j + 1])] for j in range(a, b)])


class MapResult:
    """Chains of BWTCore.map_batch: `offsets` (int64[nq + 1]) into `strand`
    (uint8, 0 = '+', 1 = '-'), `score`, `n_anchors`, `qstart`, `qend` (int32),
    `rstart`, `rend` (int64); `member_offsets` (int64[nchain + 1]) into the
    chains' anchors `member_q`, `member_len` (int32) and `member_r` (int64).
    Query coordinates are the original query's on both strands.  result[i] =
    (strand, score, n_anchors, qstart, qend, rstart, rend, anchors per chain as
    int64[k, 3] rows (q, r, len)) of query i, its chains by strand, then in the
    chainer's order.  `positions_total` is the SMEM step's position count (what
    max_positions caps), `anchors` the anchors chained, `skipped_smems` the SMEMs
    above max_occ (no anchors), `evals` the predecessors the DP evaluated."""

    __slots__ = ("offsets", "strand", "score", "n_anchors", "qstart", "qend", "rstart", "rend", "member_offsets",
                 "member_q", "member_r", "member_len", "positions_total", "skipped_smems", "anchors", "evals")

    def __init__(self, offsets, strand, score, n_anchors, qstart, qend, rstart, rend, member_offsets, member_q,
                 member_r, member_len, positions_total=0, skipped_smems=0, anchors=0, evals=0):
        self.offsets, self.strand, self.score, self.n_anchors = offsets, strand, score, n_anchors
        self.qstart, self.qend, self.rstart, self.rend = qstart, qend, rstart, rend
        self.member_offsets, self.member_q, self.member_r, self.member_len = member_offsets, member_q, member_r, member_len
        self.positions_total, self.skipped_smems, self.anchors, self.evals = positions_total, skipped_smems, anchors, evals

    def __len__(self):
        return self.offsets.size - 1

    def members(self, k: int) -> np.ndarray:
        """The anchors of chain k: int64[n, 3] rows (q, r, len), in chain order."""
        a, b = int(self.member_offsets[k]), int(self.member_offsets[k + 1])
        return np.stack([self.member_q[a:b].astype(np.int64), self.member_r[a:b],
                         self.member_len[a:b].astype(np.int64)], axis=1)

    def take(self, keep) -> "MapResult":
        """The chains with keep != 0 (one flag per chain), in their order, as a
        MapResult of the same queries: exactly the arrays map_batch returns, so
        align_chains and map_rows take it unchanged.  Offsets and members are
        rebuilt; the four counters are carried over."""
        keep = np.asarray(keep).astype(bool).reshape(-1)
        if keep.size != self.strand.size:
            raise ValueError(f"keep has {keep.size} flags for {self.strand.size} chains")
        offsets = np.asarray(self.offsets, dtype=np.int64)
        moff = np.asarray(self.member_offsets, dtype=np.int64)
        before = np.concatenate([[0], np.cumsum(keep, dtype=np.int64)])      # kept chains ahead of chain k
        sizes = (moff[1:] - moff[:-1])[keep]
        new_moff = np.concatenate([[0], np.cumsum(sizes, dtype=np.int64)])
        # member t of the result is member moff[k] + (t - new_moff[k']) of its chain k (k' its new index)
        owner = np.repeat(np.arange(sizes.size, dtype=np.int64), sizes)
        src = moff[:-1][keep][owner] + (np.arange(owner.size, dtype=np.int64) - new_moff[:-1][owner])
        cols = [np.asarray(getattr(self, k))[keep] for k in ("strand", "score", "n_anchors", "qstart", "qend", "rstart",
                                                             "rend")]
        mem = [np.asarray(getattr(self, k))[src] for k in ("member_q", "member_r", "member_len")]
        return MapResult(before[offsets], *cols, new_moff, *mem, self.positions_total, self.skipped_smems, self.anchors,
                         self.evals)

    def __getitem__(self, i: int):
        if not -len(self) <= i < len(self):
            raise IndexError(i)
        i %= len(self)
        a, b = int(self.offsets[i]), int(self.offsets[i + 1])
        return (self.strand[a:b], self.score[a:b], self.n_anchors[a:b], self.qstart[a:b], self.qend[a:b],
                self.rstart[a:b], self.rend[a:b], [self.members(k) for k in range(a, b)])


class AlignResult:
    """Base-level alignments of BWTCore.align_chains, one per chain of the
    MapResult it was given: `cigar_offsets` (int64[nchain + 1]) into `cigar`
    (uint32, len << 4 | op with BAM's codes I = 1, D = 2, '=' = 7, X = 8; on
    strand '-' in the reverse complement's order, PAF's convention); `nm` (the
    bases in X, I and D), `n_eq` (the bases in '='), `cols` (all columns),
    `qstart`, `qend` (int32, the original query's coordinates on both strands)
    and `rstart`, `rend` (int64): the aligned span, from the chain's first
    anchor to its last.  `cells_total` is the DP cells of the call (what
    max_cells caps), `gaps` the gaps by class: (no DP, one lane, one wave).
    With extend=True the CIGAR, the counts and the span include the extensions
    past the outer anchors, `head_score` and `tail_score` (int32 per chain) are
    their best scores and `ext_rows` the DP rows they took; all three are None
    without extension."""

    __slots__ = ("cigar_offsets", "cigar", "nm", "n_eq", "cols", "qstart", "qend", "rstart", "rend", "cells_total",
                 "gaps", "head_score", "tail_score", "ext_rows")
    OPS = {1: "I", 2: "D", 7: "=", 8: "X"}

    def __init__(self, cigar_offsets, cigar, nm, n_eq, cols, qstart, qend, rstart, rend, cells_total=0, gaps=(0, 0, 0),
                 head_score=None, tail_score=None, ext_rows=None):
        self.cigar_offsets, self.cigar, self.nm, self.n_eq, self.cols = cigar_offsets, cigar, nm, n_eq, cols
        self.qstart, self.qend, self.rstart, self.rend = qstart, qend, rstart, rend
        self.cells_total, self.gaps = cells_total, gaps
        self.head_score, self.tail_score, self.ext_rows = head_score, tail_score, ext_rows

    def __len__(self):
        return self.cigar_offsets.size - 1

    def cigar_string(self, k: int) -> str:
        """Chain k's CIGAR as text, e.g. 40=1X145=24D74=."""
        a, b = int(self.cigar_offsets[k]), int(self.cigar_offsets[k + 1])
        return "".join(f"{int(v) >> 4}{self.OPS[int(v) & 15]}" for v in self.cigar[a:b])


class BWTCore:
    BASE_TO_BITS = {"A": 0, "C": 1, "G": 2, "T": 3, "N": 0}
    BITS_TO_BASE = {0: "A", 1: "C", 2: "G", 3: "T"}

    def __init__(self, text: Union[str, bytes], sa_sample_rate: int = 32, occ_sample_rate: int = 128,
                 device: Optional[int] = None, build_kmer: bool = True, reverse_index: bool = False):
        # reverse_index: also build the index of the reversed text that
        # smem_long_batch steps through (BWTMI_INDEX_REVERSE: the text's last
        # character must occur once, as the '$' of seq + '$' does; ValueError
        # otherwise); the build then takes about twice as long
        # bytes are taken as the encoded text itself (no str is built: the CLI
        # hands over the loader's native contig bytes)
        raw = bytes(text) if isinstance(text, (bytes, bytearray, memoryview)) else None
        self.text = text if raw is None else _LazyText(raw)
        self.n = len(text)
        self.sa_sample_rate = sa_sample_rate
        self.occ_sample_rate = occ_sample_rate
        self.text_arr = np.frombuffer(raw if raw is not None else text.encode("utf-8"), dtype=np.uint8)
        self._ctx = _lib.ctx(device)
        self._h = C.c_void_p()
        buf = self.text_arr if self.text_arr.size else np.zeros(1, dtype=np.uint8)
        rc = lib().bwtmi_index_build(self._ctx, buf.ctypes.data_as(C.c_void_p), self.text_arr.size,
                                     sa_sample_rate, occ_sample_rate,
                                     (0 if build_kmer else 1) | (2 if reverse_index else 0), C.byref(self._h))
        if rc == -1 and reverse_index:   # BWTMI_E_ARG: the last byte is not unique
            msg = lib().bwtmi_last_error()
            raise ValueError(msg.decode(errors="replace") if msg else "bad argument")
        check(rc)
        self.has_reverse_index = bool(lib().bwtmi_index_has_reverse(self._h))
        totals = np.zeros(256, dtype=np.int64)
        cum = np.zeros(256, dtype=np.int64)
        check(lib().bwtmi_index_get_counts(self._h, totals.ctypes.data_as(C.c_void_p),
                                           cum.ctypes.data_as(C.c_void_p)))
        self._totals, self._C = totals, cum
        if raw is not None or text.isascii():
            # ASCII text (O(1) test on a CPython str): the characters are the
            # byte values the device histogram found (bwt.py:129)
            self.alphabet = [chr(c) for c in np.nonzero(totals)[0].tolist()]
        else:
            self.alphabet = sorted(set(text))
        self.char_to_code = {c: ord(c) for c in self.alphabet}
        self.code_to_char = {ord(c): c for c in self.alphabet}
        self.char_counts = {c: int(cum[ord(c)]) for c in self.alphabet if ord(c) < 256}
        self.char_totals = {c: int(totals[ord(c)]) for c in self.alphabet if ord(c) < 256}
        self.char_counts_code = {ord(k): v for k, v in self.char_counts.items()}
        self.char_totals_code = {ord(k): v for k, v in self.char_totals.items()}
        self._sa = self._bwt = self._occ = self._sampled = self._kmer = None

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib._lib is not None:
            _lib._lib.bwtmi_index_free(h)
            self._h = None

    # ---------------------------------------------------------------- arrays
    @property
    def suffix_array(self) -> np.ndarray:
        if self._sa is None:
            a = np.zeros(max(self.text_arr.size, 1), dtype=np.int32)
            check(lib().bwtmi_index_get_sa(self._h, a.ctypes.data_as(C.c_void_p)))
            self._sa = a[:self.text_arr.size]
        return self._sa

    @property
    def bwt_arr(self) -> np.ndarray:
        if self._bwt is None:
            a = np.zeros(max(self.text_arr.size, 1), dtype=np.uint8)
            check(lib().bwtmi_index_get_bwt(self._h, a.ctypes.data_as(C.c_void_p)))
            self._bwt = a[:self.text_arr.size]
        return self._bwt

    @property
    def occ_checkpoints(self) -> Dict[int, np.ndarray]:
        if self._occ is None:
            L = lib().bwtmi_index_occ_len(self._h)
            occ = {}
            if self.text_arr.size:
                for code in np.nonzero(self._totals)[0].tolist():
                    a = np.zeros(L, dtype=np.int32)
                    check(lib().bwtmi_index_get_occ(self._h, code, a.ctypes.data_as(C.c_void_p)))
                    occ[int(code)] = a
                for ch in self.alphabet:       # bwt.py:319-325
                    if ord(ch) not in occ:
                        occ[ord(ch)] = np.zeros(L, dtype=np.int32)
            self._occ = occ
        return self._occ

    @property
    def sampled_sa(self) -> Dict[int, int]:
        if self._sampled is None:
            m = lib().bwtmi_index_sampled_len(self._h)
            a = np.zeros(max(m, 1), dtype=np.int32)
            if m:
                check(lib().bwtmi_index_get_sampled(self._h, a.ctypes.data_as(C.c_void_p)))
            self._sampled = {i * self.sa_sample_rate: int(a[i]) for i in range(m)}
        return self._sampled

    def kmer_csr(self) -> Tuple[np.ndarray, np.ndarray]:
        m = lib().bwtmi_index_kmer_count(self._h)
        off = np.zeros(65537, dtype=np.int64)
        pos = np.zeros(max(m, 1), dtype=np.int32)
        check(lib().bwtmi_index_get_kmer(self._h, off.ctypes.data_as(C.c_void_p),
                                         pos.ctypes.data_as(C.c_void_p)))
        return off, pos[:m]

    @property
    def kmer_hash(self) -> Dict[int, List[int]]:
        if self._kmer is None:
            off, pos = self.kmer_csr()
            nz = np.nonzero(np.diff(off))[0]
            self._kmer = {int(c): pos[off[c]:off[c + 1]].tolist() for c in nz.tolist()}
        return self._kmer

    def get_kmer_positions(self, kmer: str) -> List[int]:
        """bwt.py:173-193 (including its direct lookup of k < 8 codes)."""
        if len(kmer) > 8 or not self.kmer_hash:
            return self.locate_positions(kmer)
        w = 0
        for b in kmer.upper():
            if b not in self.BASE_TO_BITS:
                return []
            w = (w << 2) | self.BASE_TO_BITS[b]
        return list(self.kmer_hash.get(w, []))

    def clear(self):
        self.text = ""
        self.text_arr = np.array([], dtype=np.uint8)
        self._sa = np.array([], dtype=np.int32)
        self._bwt = np.array([], dtype=np.uint8)
        self._sampled, self._occ = {}, {}
        self.char_counts, self.char_totals, self.alphabet = {}, {}, []
        self.char_to_code, self.code_to_char = {}, {}
        self.char_counts_code, self.char_totals_code = {}, {}
        if self._h and _lib._lib is not None:
            _lib._lib.bwtmi_index_free(self._h)
            self._h = None

    # ---------------------------------------------------------------- queries
    def rank(self, char: Union[str, int], pos: int) -> int:
        if pos <= 0:
            return 0
        pos = min(pos, self.n)
        code = ord(char) if isinstance(char, str) else int(char)
        cp = self.occ_checkpoints.get(code)
        if cp is None:
            return 0
        k = self.occ_sample_rate
        ci = pos // k
        base = int(cp[ci])
        if pos > ci * k:
            base += int(np.count_nonzero(self.bwt_arr[ci * k:pos] == code))
        return base

    @staticmethod
    def pack_patterns(patterns: Sequence[str]) -> Tuple[np.ndarray, np.ndarray]:
        """(concatenated bytes, offsets[n + 1]) for backward_search_packed."""
        enc = [p.encode("utf-8") for p in patterns]
        off = np.zeros(len(enc) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(e) for e in enc]) if enc else 0
        blob = np.frombuffer(b"".join(enc) or b"\0", dtype=np.uint8)
        return blob, off

    def backward_search_packed(self, blob: np.ndarray, off: np.ndarray) -> np.ndarray:
        npat = off.size - 1
        out = np.zeros((max(npat, 1), 2), dtype=np.int64)
        check(lib().bwtmi_backward_search_batch(self._ctx, self._h, blob.ctypes.data_as(C.c_void_p),
                                                off.ctypes.data_as(C.c_void_p), npat,
                                                out.ctypes.data_as(C.c_void_p)))
        return out[:npat]

    def backward_search_batch(self, patterns: Sequence[str]) -> np.ndarray:
        """Device batch of BWTCore.backward_search: int64[len(patterns), 2]."""
        return self.backward_search_packed(*self.pack_patterns(patterns))

    def backward_search(self, pattern: str) -> Tuple[int, int]:
        if not pattern:
            return (0, self.n - 1)
        if any(ch not in self.char_counts for ch in pattern):   # non-byte / absent symbols
            return (-1, -1)
        sp, ep = self.backward_search_batch([pattern])[0].tolist()
        return (int(sp), int(ep))

    def count_occurrences(self, pattern: str) -> int:
        sp, ep = self.backward_search(pattern)
        return 0 if sp == -1 else ep - sp + 1

    def locate_positions(self, pattern: str) -> List[int]:
        sp, ep = self.backward_search(pattern)
        if sp == -1:
            return []
        return sorted(self.suffix_array[sp:ep + 1].tolist())

    def locate_batch(self, patterns: Sequence[Union[str, bytes]], max_mismatches: int = 0,
                     both_strands: bool = False, max_candidates: Optional[int] = None) -> "LocateResult":
        """Every occurrence of every pattern with at most `max_mismatches`
        (0..3) substitutions, on the text's strand or on both, located on the
        device (include/bwtmi.h, bwtmi_index_locate_batch, states the contract).
        ValueError for an empty pattern, one shorter than max_mismatches + 1
        or longer than 1024 bytes, or max_mismatches outside 0..3; BwtmiError
        with the candidate count when it exceeds max_candidates (default 2^27)."""
        if max_candidates is not None and int(max_candidates) <= 0:
            raise ValueError("max_candidates must be positive")
        # encoded as pack_patterns does (bytes are taken as they are)
        enc = [p.encode("utf-8") if isinstance(p, str) else bytes(p) for p in patterns]
        off = np.zeros(len(enc) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(e) for e in enc]) if enc else 0
        blob = np.frombuffer(b"".join(enc) or b"\0", dtype=np.uint8)
        npat = off.size - 1
        hoff, pos, mm, strand = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        nh, cand = C.c_int64(0), C.c_int64(0)
        rc = lib().bwtmi_index_locate_batch(self._ctx, self._h, blob.ctypes.data_as(C.c_void_p),
                                            off.ctypes.data_as(C.c_void_p), npat, int(max_mismatches),
                                            1 if both_strands else 0,
                                            0 if max_candidates is None else int(max_candidates),
                                            C.byref(hoff), C.byref(pos), C.byref(mm), C.byref(strand),
                                            C.byref(nh), C.byref(cand))
        if rc == -1:   # BWTMI_E_ARG
            msg = lib().bwtmi_last_error()
            raise ValueError(msg.decode(errors="replace") if msg else "bad argument")
        check(rc)
        try:
            n = nh.value

            def take(p, dtype, count):
                if not count:
                    return np.zeros(0, dtype=dtype)
                return np.ctypeslib.as_array(C.cast(p, C.POINTER(np.ctypeslib.as_ctypes_type(dtype))),
                                             shape=(count,)).copy()
            return LocateResult(take(hoff, np.int64, npat + 1), take(pos, np.int64, n), take(mm, np.uint8, n),
                                take(strand, np.uint8, n), cand.value)
        finally:
            for p in (hoff, pos, mm, strand):
                lib().bwtmi_free(p)

    def smem_batch(self, queries: Sequence[Union[str, bytes]], min_len: int = 1, both_strands: bool = False,
                   max_occ: Optional[int] = None, max_positions: Optional[int] = None) -> "SmemResult":
        """The super-maximal exact matches (>= `min_len` bytes) of every query
        against the index text, on the text's strand or on both, with their
        occurrences when there are at most `max_occ` (default 1024), found on
        the device (include/bwtmi.h, bwtmi_index_smem_batch, states the
        contract).  ValueError for an empty query, one longer than 1024 bytes
        or min_len < 1; BwtmiError with the position count when it exceeds
        max_positions (default 2^27)."""
        return self._smem(False, queries, min_len, both_strands, max_occ, max_positions)

    def smem_long_batch(self, queries: Sequence[Union[str, bytes]], min_len: int = 1, both_strands: bool = False,
                        max_occ: Optional[int] = None, max_positions: Optional[int] = None) -> "SmemResult":
        """smem_batch for long reads: the same contract and, for queries that
        both accept, the same result, for queries of up to 1,048,576 bytes
        (include/bwtmi.h, bwtmi_index_smem_long_batch).  The index must have
        been built with reverse_index=True (BwtmiError otherwise).  The
        result's `steps` is the rank steps taken: linear in the read length
        when the read matches in a few long stretches, quadratic again when
        its SMEMs overlap almost completely (a repeat tract longer than the
        text's)."""
        return self._smem(True, queries, min_len, both_strands, max_occ, max_positions)

    def _smem(self, long_entry, queries, min_len, both_strands, max_occ, max_positions) -> "SmemResult":
        for name, v in (("max_occ", max_occ), ("max_positions", max_positions)):
            if v is not None and int(v) <= 0:
                raise ValueError(f"{name} must be positive")
        enc = [q.encode("utf-8") if isinstance(q, str) else bytes(q) for q in queries]
        off = np.zeros(len(enc) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(e) for e in enc]) if enc else 0
        blob = np.frombuffer(b"".join(enc) or b"\0", dtype=np.uint8)
        nq = off.size - 1
        ptrs = [C.c_void_p() for _ in range(7)]
        ns, npos, total, work, steps = (C.c_int64(0) for _ in range(5))
        entry = lib().bwtmi_index_smem_long_batch if long_entry else lib().bwtmi_index_smem_batch
        rc = entry(self._ctx, self._h, blob.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p), nq,
                   int(min_len), 1 if both_strands else 0, 0 if max_occ is None else int(max_occ),
                   0 if max_positions is None else int(max_positions), *[C.byref(p) for p in ptrs], C.byref(ns),
                   C.byref(npos), C.byref(total), C.byref(work), *([C.byref(steps)] if long_entry else []))
        if rc == -1:   # BWTMI_E_ARG
            msg = lib().bwtmi_last_error()
            raise ValueError(msg.decode(errors="replace") if msg else "bad argument")
        check(rc)
        try:
            def take(p, dtype, count):
                if not count:
                    return np.zeros(0, dtype=dtype)
                return np.ctypeslib.as_array(C.cast(p, C.POINTER(np.ctypeslib.as_ctypes_type(dtype))),
                                             shape=(count,)).copy()
            n = ns.value
            return SmemResult(take(ptrs[0], np.int64, nq + 1), take(ptrs[1], np.int32, n), take(ptrs[2], np.int32, n),
                              take(ptrs[3], np.uint8, n), take(ptrs[4], np.int64, n), take(ptrs[5], np.int64, n + 1),
                              take(ptrs[6], np.int64, npos.value), total.value, work.value, steps.value)
        finally:
            for p in ptrs:
                lib().bwtmi_free(p)

    def chain_anchors(self, group_off, q, r, length, **chain_params) -> dict:
        """The device chainer on a caller's anchors (include/bwtmi.h,
        bwtmi_chain_anchors, states the contract): see bwtmi._lib.chain_anchors."""
        return _lib.chain_anchors(self._ctx, group_off, q, r, length, **chain_params)

    def map_batch(self, queries: Sequence[Union[str, bytes]], min_len: int = 19, both_strands: bool = False,
                  long: bool = False, max_occ: Optional[int] = None, max_positions: Optional[int] = None,
                  **chain_params) -> "MapResult":
        """Where every query lies in the index text: its SMEMs (smem_batch, or
        smem_long_batch with long=True, which needs reverse_index=True) turned
        into anchors and chained on the device (include/bwtmi.h,
        bwtmi_index_map_batch, states the contract).  chain_params: max_gap,
        bandwidth, max_pred, min_score, min_anchors (absent: the defaults 5000,
        500, 1024, 40, 1).  ValueError as smem_batch raises it, and for
        max_pred > 4096 or bandwidth > max_gap; BwtmiError with the position
        count when it exceeds max_positions, and for long=True without a
        reverse index."""
        for name, v in (("max_occ", max_occ), ("max_positions", max_positions)):
            if v is not None and int(v) <= 0:
                raise ValueError(f"{name} must be positive")
        cp = _lib.chain_params(**chain_params)
        enc = [q.encode("utf-8") if isinstance(q, str) else bytes(q) for q in queries]
        off = np.zeros(len(enc) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(e) for e in enc]) if enc else 0
        blob = np.frombuffer(b"".join(enc) or b"\0", dtype=np.uint8)
        nq = off.size - 1
        ptrs = [C.c_void_p() for _ in range(12)]
        nc, nm, total, skipped, anchors, evals = (C.c_int64(0) for _ in range(6))
        rc = lib().bwtmi_index_map_batch(self._ctx, self._h, blob.ctypes.data_as(C.c_void_p),
                                         off.ctypes.data_as(C.c_void_p), nq, int(min_len),
                                         (1 if both_strands else 0) | (4 if long else 0),
                                         0 if max_occ is None else int(max_occ),
                                         0 if max_positions is None else int(max_positions), C.byref(cp),
                                         *[C.byref(p) for p in ptrs], C.byref(nc), C.byref(nm), C.byref(total),
                                         C.byref(skipped), C.byref(anchors), C.byref(evals))
        if rc == -1:   # BWTMI_E_ARG
            msg = lib().bwtmi_last_error()
            raise ValueError(msg.decode(errors="replace") if msg else "bad argument")
        check(rc)
        try:
            n, m = nc.value, nm.value
            kinds = (np.int64, np.uint8, np.int32, np.int32, np.int32, np.int32, np.int64, np.int64, np.int64, np.int32,
                     np.int64, np.int32)
            counts = (nq + 1, n, n, n, n, n, n, n, n + 1, m, m, m)
            return MapResult(*[_lib.take(p, t, k) for p, t, k in zip(ptrs, kinds, counts)], total.value, skipped.value,
                             anchors.value, evals.value)
        finally:
            for p in ptrs:
                lib().bwtmi_free(p)

    def align_chains(self, queries: Sequence[Union[str, bytes]], map_result, band: Optional[int] = None,
                     max_cells: Optional[int] = None, extend: bool = False, ext_band: Optional[int] = None,
                     match: Optional[int] = None, mismatch: Optional[int] = None, gap: Optional[int] = None,
                     xdrop: Optional[int] = None) -> "AlignResult":
        """Every chain of `map_result` (a MapResult of map_batch on the same
        `queries`, or any object with its arrays: hand-made chains) aligned
        base by base on the device: a banded edit-distance DP with traceback
        per gap between anchors, one CIGAR per chain (include/bwtmi.h,
        bwtmi_index_align_chains, states the contract).  band: the DP's W
        (default 32, 0 is legal, at most 1024); max_cells: the cap on the
        call's DP cells (default 2^30).  ValueError for chains the contract
        refuses and for a band outside 0..1024; BwtmiError, with the count in
        its `cells_total`, when the cells exceed max_cells.
        extend=True (bwtmi_index_align_extend): every chain is also extended
        past its outer anchors towards the read's ends, a scored banded DP
        with X-drop; ext_band its band (default 32, at most 1024), match,
        mismatch, gap its scores (defaults 1, 3, 3; at most 64), xdrop its X
        (default 30).  The result then carries head_score, tail_score and
        ext_rows."""
        if band is not None and int(band) < 0:
            raise ValueError("band must not be negative")
        ext = dict(ext_band=ext_band, match=match, mismatch=mismatch, gap=gap, xdrop=xdrop)
        for k, v in ext.items():
            if v is not None and not extend:
                raise ValueError(f"{k} needs extend=True")
            if v is not None and int(v) < 0:
                raise ValueError(f"{k} must not be negative")
        if max_cells is not None and int(max_cells) <= 0:
            raise ValueError("max_cells must be positive")
        enc = [q.encode("utf-8") if isinstance(q, str) else bytes(q) for q in queries]
        off = np.zeros(len(enc) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(e) for e in enc]) if enc else 0
        blob = np.frombuffer(b"".join(enc) or b"\0", dtype=np.uint8)
        nq = off.size - 1
        r = map_result
        arrs = [np.ascontiguousarray(a, dtype=t) for a, t in (
            (r.offsets, np.int64), (r.strand, np.uint8), (r.member_offsets, np.int64), (r.member_q, np.int32),
            (r.member_r, np.int64), (r.member_len, np.int32))]
        coff, strand, moff, mq, mr, ml = arrs
        if coff.size != nq + 1 or moff.size != strand.size + 1 or not mq.size == mr.size == ml.size:
            raise ValueError("the chains' arrays do not fit the queries or each other")
        ap = _lib.ExtendParams() if extend else _lib.AlignParams()
        ap.band = -1 if band is None else int(band)
        ap.max_cells = 0 if max_cells is None else int(max_cells)
        for k, v in ext.items():
            if extend:
                setattr(ap, k, -1 if v is None else int(v))
        ptrs = [C.c_void_p() for _ in range(11 if extend else 9)]
        nc, cells, rows = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        gaps = (C.c_int64 * 3)()
        ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None      # noqa: E731
        entry = lib().bwtmi_index_align_extend if extend else lib().bwtmi_index_align_chains
        rc = entry(self._ctx, self._h, blob.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p), nq,
                   coff.ctypes.data_as(C.c_void_p), ptr(strand), moff.ctypes.data_as(C.c_void_p), ptr(mq), ptr(mr),
                   ptr(ml), strand.size, mq.size, C.byref(ap), *[C.byref(p) for p in ptrs], C.byref(nc),
                   C.byref(cells), gaps, *([C.byref(rows)] if extend else []))
        if rc == -1:   # BWTMI_E_ARG
            msg = lib().bwtmi_last_error()
            raise ValueError(msg.decode(errors="replace") if msg else "bad argument")
        try:
            check(rc)
        except _lib.BwtmiError as e:
            e.cells_total = cells.value   # the count a tripped cap reports (0 for any other failure)
            raise
        try:
            n = strand.size
            kinds = (np.int64, np.uint32, np.int32, np.int32, np.int32, np.int32, np.int32, np.int64, np.int64)
            counts = (n + 1, nc.value, n, n, n, n, n, n, n)
            res = AlignResult(*[_lib.take(p, t, k) for p, t, k in zip(ptrs, kinds, counts)], cells.value,
                              tuple(int(v) for v in gaps))
            if extend:
                res.head_score, res.tail_score = (_lib.take(p, np.int32, n) for p in ptrs[9:])
                res.ext_rows = rows.value
            return res
        finally:
            for p in ptrs:
                lib().bwtmi_free(p)

    def _get_suffix_position(self, sa_index: int) -> int:
        return int(self.suffix_array[sa_index])

    def lcp_array(self) -> np.ndarray:
        """Kasai LCP over the index text (bwt.py:56-95) computed on the device."""
        out = np.zeros(max(self.text_arr.size, 1), dtype=np.int32)
        if self.text_arr.size:
            check(lib().bwtmi_index_lcp(self._ctx, self._h, out.ctypes.data_as(C.c_void_p)))
        return out[:self.text_arr.size]
