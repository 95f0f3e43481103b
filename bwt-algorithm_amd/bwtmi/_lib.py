"""ctypes binding of libbwtmi.so (C ABI in include/bwtmi.h).

The shared library is built in-tree (``make -C bwt-algorithm_amd``) and loaded
from the package's parent directory.  There is deliberately no fallback: if
the library or a gfx950 device is missing, the calls below raise.
"""
from __future__ import annotations

import atexit
import ctypes as C
import os
import threading
from typing import Dict, Optional

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("BWTMI_LIB", os.path.join(_PKG_ROOT, "libbwtmi.so"))

FMT = {"strfinder": 0, "bed": 1, "vcf": 2, "trf_table": 3, "trf_dat": 4}


class BwtmiError(RuntimeError):
    pass


class Hit(C.Structure):
    _fields_ = [("start", C.c_int64), ("end", C.c_int64), ("unit_len", C.c_int32),
                ("prim_len", C.c_int32), ("copies", C.c_int64)]


class Params(C.Structure):
    _fields_ = [("min_copies", C.c_int32), ("max_unit_len", C.c_int32),
                ("show_progress", C.c_int32), ("tier2", C.c_int32), ("threads", C.c_int32),
                ("build_index", C.c_int32), ("sa_sample", C.c_int32), ("reserved", C.c_int32)]


class ChainParams(C.Structure):
    _fields_ = [("max_gap", C.c_int32), ("bandwidth", C.c_int32), ("max_pred", C.c_int32),
                ("min_score", C.c_int32), ("min_anchors", C.c_int32), ("reserved", C.c_int32 * 3)]


class AlignParams(C.Structure):
    _fields_ = [("band", C.c_int32), ("reserved", C.c_int32 * 3), ("max_cells", C.c_int64)]


class ExtendParams(C.Structure):
    _fields_ = [("band", C.c_int32), ("ext_band", C.c_int32), ("match", C.c_int32), ("mismatch", C.c_int32),
                ("gap", C.c_int32), ("xdrop", C.c_int32), ("reserved", C.c_int32 * 2), ("max_cells", C.c_int64)]


class SelectParams(C.Structure):
    _fields_ = [("mask", C.c_int32), ("pri_ratio", C.c_int32), ("best_n", C.c_int32), ("full", C.c_int32),
                ("reserved", C.c_int32 * 4)]


class LibParams(C.Structure):
    _fields_ = [("min_period", C.c_int32), ("max_period", C.c_int32), ("max_short_motif", C.c_int32),
                ("min_copies", C.c_int32), ("min_array_length", C.c_int32), ("allow_mismatches", C.c_int32),
                ("min_entropy", C.c_double)]


_lib = None
_lock = threading.RLock()    # ctx() -> lib() re-enters

# name -> (restype, argtypes)
_P = C.c_void_p
_SIGS = {
    "bwtmi_last_error": (C.c_char_p, []),
    "bwtmi_version": (C.c_char_p, []),
    "bwtmi_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "bwtmi_open": (C.c_int, [C.c_int, C.POINTER(_P)]),
    "bwtmi_close": (C.c_int, [_P]),
    "bwtmi_free": (None, [_P]),
    "bwtmi_last_timing": (C.c_int, [_P, C.POINTER(C.c_double)]),
    "bwtmi_kernel_stats": (C.c_int, [_P, C.c_int, C.c_int, C.c_char_p, C.c_int64]),
    "bwtmi_kernel_stats_filter": (C.c_int, [_P, C.c_char_p]),
    "bwtmi_strict_scan": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                    C.POINTER(C.POINTER(Hit)), C.POINTER(C.c_int64)]),
    "bwtmi_screen_hits": (C.c_int, [_P, _P, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int64,
                                    C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
    "bwtmi_radix_sort": (C.c_int, [_P, C.c_int32, _P, _P, C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    "bwtmi_exclusive_scan": (C.c_int, [_P, C.c_int32, _P, _P, C.c_int64, C.c_int32, C.c_int64, C.c_int32,
                                       C.c_int32, C.c_int64]),
    "bwtmi_index_build": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, C.c_uint32, C.POINTER(_P)]),
    "bwtmi_index_free": (C.c_int, [_P]),
    "bwtmi_index_has_reverse": (C.c_int, [_P]),
    "bwtmi_index_size": (C.c_int64, [_P]),
    "bwtmi_index_get_sa": (C.c_int, [_P, _P]),
    "bwtmi_index_get_bwt": (C.c_int, [_P, _P]),
    "bwtmi_index_get_counts": (C.c_int, [_P, _P, _P]),
    "bwtmi_index_occ_len": (C.c_int64, [_P]),
    "bwtmi_index_get_occ": (C.c_int, [_P, C.c_uint8, _P]),
    "bwtmi_index_sampled_len": (C.c_int64, [_P]),
    "bwtmi_index_get_sampled": (C.c_int, [_P, _P]),
    "bwtmi_index_kmer_count": (C.c_int64, [_P]),
    "bwtmi_index_get_kmer": (C.c_int, [_P, _P, _P]),
    "bwtmi_index_lcp": (C.c_int, [_P, _P, _P]),
    "bwtmi_backward_search_batch": (C.c_int, [_P, _P, _P, _P, C.c_int64, _P]),
    "bwtmi_index_locate_batch": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int32, C.c_uint32, C.c_int64,
                                           C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                           C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "bwtmi_index_smem_batch": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int32, C.c_uint32, C.c_int64, C.c_int64] +
                               [C.POINTER(C.c_void_p)] * 7 + [C.POINTER(C.c_int64)] * 4),
    "bwtmi_index_smem_long_batch": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int32, C.c_uint32, C.c_int64, C.c_int64] +
                                    [C.POINTER(C.c_void_p)] * 7 + [C.POINTER(C.c_int64)] * 5),
    "bwtmi_chain_anchors": (C.c_int, [_P, _P, C.c_int64, _P, _P, _P, C.POINTER(ChainParams)] +
                            [C.POINTER(C.c_void_p)] * 9 + [C.POINTER(C.c_int64)] * 3),
    "bwtmi_index_map_batch": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int32, C.c_uint32, C.c_int64, C.c_int64,
                                        C.POINTER(ChainParams)] + [C.POINTER(C.c_void_p)] * 12 +
                              [C.POINTER(C.c_int64)] * 6),
    "bwtmi_select_chains": (C.c_int, [_P, _P, C.c_int64, _P, _P, _P, C.POINTER(SelectParams)] +
                            [C.POINTER(C.c_void_p)] * 4 + [C.POINTER(C.c_int64)] * 2),
    "bwtmi_index_align_chains": (C.c_int, [_P, _P, _P, _P, C.c_int64, _P, _P, _P, _P, _P, _P, C.c_int64, C.c_int64,
                                           C.POINTER(AlignParams)] + [C.POINTER(C.c_void_p)] * 9 +
                                 [C.POINTER(C.c_int64)] * 2 + [_P]),
    "bwtmi_index_align_extend": (C.c_int, [_P, _P, _P, _P, C.c_int64, _P, _P, _P, _P, _P, _P, C.c_int64, C.c_int64,
                                           C.POINTER(ExtendParams)] + [C.POINTER(C.c_void_p)] * 11 +
                                 [C.POINTER(C.c_int64)] * 2 + [_P, C.POINTER(C.c_int64)]),
    "bwtmi_index_lcp_plateaus": (C.c_int, [_P, _P, C.POINTER(LibParams), C.POINTER(C.c_void_p),
                                           C.POINTER(C.c_int64)]),
    "bwtmi_index_short_imperfect": (C.c_int, [_P, _P, C.POINTER(LibParams), _P, C.c_int64, _P, C.c_int32]),
    "bwtmi_job_tier1": (C.c_int, [_P, _P, C.c_int32, C.c_int32]),
    "bwtmi_index_long_repeats": (C.c_int, [_P, _P, C.POINTER(LibParams), _P, C.c_int64, _P, C.c_int32]),
    "bwtmi_index_tier3": (C.c_int, [_P, _P, _P, _P, C.c_int64, _P, C.c_int32, C.c_int32]),
    "bwtmi_job_create": (C.c_int, [C.POINTER(Params), C.POINTER(_P)]),
    "bwtmi_job_free": (C.c_int, [_P]),
    "bwtmi_job_add_contig": (C.c_int, [_P, C.c_char_p, _P, C.c_int64, C.c_int64, C.c_int64,
                                       C.POINTER(C.c_int32)]),
    "bwtmi_job_scan": (C.c_int, [_P, _P]),
    "bwtmi_job_wait": (C.c_int, [_P, _P]),
    "bwtmi_job_upload": (C.c_int, [_P, _P]),
    "bwtmi_job_reset": (C.c_int, [_P]),
    "bwtmi_job_set_params": (C.c_int, [_P, C.POINTER(Params)]),
    "bwtmi_job_select": (C.c_int, [_P, _P, C.c_int32]),
    "bwtmi_job_add_hits": (C.c_int, [_P, C.c_int32, _P, C.c_int64]),
    "bwtmi_job_raw_count": (C.c_int64, [_P]),
    "bwtmi_job_postprocess": (C.c_int, [_P]),
    "bwtmi_job_count": (C.c_int64, [_P]),
    "bwtmi_job_render": (C.c_int, [_P, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
    "bwtmi_job_write": (C.c_int, [_P, C.c_int, C.c_char_p]),
    "bwtmi_job_write_async": (C.c_int, [_P, C.c_int, C.c_char_p]),
    "bwtmi_job_write_join": (C.c_int, [_P]),
    "bwtmi_job_unit_count": (C.c_int32, [_P]),
    "bwtmi_job_unit_rows": (C.c_int, [_P, _P]),
    "bwtmi_job_render_units": (C.c_int, [_P, C.c_int, _P, _P]),
    "bwtmi_job_write_units": (C.c_int, [_P, C.c_char_p, _P, C.c_int]),
    "bwtmi_job_write_units_async": (C.c_int, [_P, C.c_char_p, _P, C.c_int]),
    "bwtmi_job_get_records": (C.c_int, [_P, _P, _P]),
    "bwtmi_job_get_string": (C.c_int64, [_P, C.c_int64, C.c_int, _P, C.c_int64]),
    "bwtmi_job_get_strings": (C.c_int64, [_P, C.c_int, _P, C.c_int64, _P]),
    "bwtmi_fasta_count_records": (C.c_int64, [C.c_char_p, C.c_int64]),
    "bwtmi_job_export": (C.c_int, [_P, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
    "bwtmi_job_import": (C.c_int, [_P, _P, C.c_int64]),
    "bwtmi_job_stage_ms": (C.c_int, [_P, C.POINTER(C.c_double)]),
    "bwtmi_align_region": (C.c_int, [C.c_char_p, C.c_int64, C.c_int64, C.c_int64, C.c_char_p, C.c_int64,
                                     C.c_double, C.c_int64, C.c_int64, _P, C.POINTER(C.c_double), _P,
                                     C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "bwtmi_job_load_fasta": (C.c_int, [_P, C.c_char_p, C.c_int32]),
    "bwtmi_job_load_fasta_dev": (C.c_int, [_P, _P, C.c_char_p, C.c_int32]),
    "bwtmi_job_device_text": (C.c_int, [_P, _P, C.c_int32, C.c_void_p]),
    "bwtmi_job_contig_count": (C.c_int32, [_P]),
    "bwtmi_job_contig_info": (C.c_int64, [_P, C.c_int32, C.c_char_p, C.c_int64, C.POINTER(C.c_int64),
                                          C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "bwtmi_job_contig_seq": (C.c_int, [_P, C.c_int32, _P]),
    "bwtmi_job_load_fasta_shard": (C.c_int, [_P, C.c_char_p, C.c_int32, C.c_int32, C.c_int32]),
    "bwtmi_job_fasta_scan_part": (C.c_int, [_P, C.c_char_p, C.c_int32, C.c_int32, C.POINTER(C.c_void_p),
                                            C.POINTER(C.c_int64)]),
    "bwtmi_job_fasta_scan_part_dev": (C.c_int, [_P, _P, C.c_char_p, C.c_int32, C.c_int32, C.POINTER(C.c_void_p),
                                                C.POINTER(C.c_int64)]),
    "bwtmi_job_load_fasta_parts": (C.c_int, [_P, C.c_char_p, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int64]),
    "bwtmi_job_load_fasta_parts_dev": (C.c_int, [_P, _P, C.c_char_p, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int64]),
    "bwtmi_job_contig_weight": (C.c_int64, [_P, C.c_int32]),
    "bwtmi_job_select_shard": (C.c_int, [_P, C.c_int32, C.c_int32, _P, _P]),
    "bwtmi_host_info": (C.c_int, [C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "bwtmi_comm_unique_id": (C.c_int, [_P]),
    "bwtmi_comm_init": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _P, C.POINTER(_P)]),
    "bwtmi_comm_allreduce": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32]),
    "bwtmi_comm_free": (C.c_int, [_P]),
    "bwtmi_device_sync": (C.c_int, [C.c_int32]),
    "bwtmi_job_set_records": (C.c_int, [_P, _P, C.c_int64]),
    "bwtmi_wire_record_size": (C.c_int, []),
    "bwtmi_job_contig_error": (C.c_int64, [_P, C.c_int32, C.c_char_p, C.c_int64]),
    "bwtmi_source_hash": (C.c_char_p, []),
    "bwtmi_trace_push": (C.c_int, [C.c_char_p]),
    "bwtmi_trace_pop": (C.c_int, []),
    "bwtmi_knob_set": (C.c_int, [C.c_char_p, C.c_int64]),
    "bwtmi_knob_get": (C.c_int, [C.c_char_p, C.POINTER(C.c_int64)]),
    "bwtmi_knob_default": (C.c_int, [C.c_char_p, C.POINTER(C.c_int64)]),
    "bwtmi_knob_names": (C.c_char_p, []),
    "bwtmi_bind_host": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int)]),
    "bwtmi_host_binding_plan": (C.c_int, [C.c_char_p, C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_char_p,
                                          C.c_char_p, C.c_int64, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
}
EXPORTED = tuple(_SIGS)


def lib():
    """Load libbwtmi.so (raises BwtmiError if it was not built)."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise BwtmiError(f"{LIB_PATH} not found: build it with `make -C {_PKG_ROOT}` "
                                 "(there is no CPU fallback)")
            L = C.CDLL(LIB_PATH)
            for name, (res, args) in _SIGS.items():
                fn = getattr(L, name)
                fn.restype = res
                fn.argtypes = args
            _lib = L
    return _lib


def check(rc: int) -> None:
    if rc != 0:
        msg = lib().bwtmi_last_error()
        raise BwtmiError(f"libbwtmi error {rc}: {msg.decode(errors='replace') if msg else ''}")


_ctxs: Dict[int, C.c_void_p] = {}


def device_count() -> int:
    n = C.c_int(0)
    check(lib().bwtmi_device_count(C.byref(n)))
    return n.value


def ctx(device: Optional[int] = None) -> C.c_void_p:
    """Per-process device context (opened once per device, closed at exit)."""
    if device is None:
        device = int(os.environ.get("BWTMI_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    with _lock:
        h = _ctxs.get(device)
        if h is None:
            h = C.c_void_p()
            check(lib().bwtmi_open(device, C.byref(h)))
            _ctxs[device] = h
    return h


@atexit.register
def _close_all():
    if _lib is None:
        return
    for h in list(_ctxs.values()):
        _lib.bwtmi_close(h)
    _ctxs.clear()


def source_hash() -> str:
    """sha256 of csrc/* and include/bwtmi.h embedded when libbwtmi.so was built."""
    return lib().bwtmi_source_hash().decode()


def tree_source_hash() -> str:
    """The same hash computed from the sources in this tree (Makefile SRC_HASH):
    the files in byte order of their paths, concatenated."""
    import glob
    import hashlib
    csrc = os.path.join(_PKG_ROOT, "csrc")
    files = sorted(glob.glob(os.path.join(csrc, "*.cpp")) + glob.glob(os.path.join(csrc, "*.h")) +
                   glob.glob(os.path.join(csrc, "*.hip")))
    files.append(os.path.join(os.path.dirname(_PKG_ROOT), "include", "bwtmi.h"))
    h = hashlib.sha256()
    for f in files:
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()


def check_build() -> str:
    """Fails loudly when the loaded library was built from other sources than
    this tree's (a stale or foreign libbwtmi.so); returns the hash."""
    got, want = source_hash(), tree_source_hash()
    if got != want:
        raise BwtmiError(f"{LIB_PATH} was built from sources {got[:16]}..., this tree holds {want[:16]}...: "
                         f"rebuild with `make -C {_PKG_ROOT}`")
    return got


def knob(name: str, value: Optional[int] = None) -> int:
    """Read (and with value, set) a run-time switch BWTMI_<name>;
    returns the value before the call."""
    v = C.c_int64()
    check(lib().bwtmi_knob_get(name.encode(), C.byref(v)))
    if value is not None:
        check(lib().bwtmi_knob_set(name.encode(), int(value)))
    return v.value


def knob_names() -> list:
    return lib().bwtmi_knob_names().decode().split(",")


class knobs:
    """with knobs(RUNS_DENSE=1, ...): set switches for the block, restore after."""

    def __init__(self, **kv):
        self.kv = kv
        self.old = {}

    def __enter__(self):
        for k, v in self.kv.items():
            self.old[k] = knob(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.old.items():
            knob(k, v)
        return False


def bind_host(h, on: bool = True) -> bool:
    """Move this process's host work onto the CPUs of its GPU's NUMA node (the
    CLI, bench and rank launcher ask for it; the library never does on its own);
    on=False restores the affinity the binding replaced.  True when it changed."""
    b = C.c_int(0)
    check(lib().bwtmi_bind_host(h, int(on), C.byref(b)))
    return bool(b.value)


def binding_plan(sysroot: str, local_rank: int, rank_pci, threads: int, allowed: str, smt: bool = False):
    """(cpulist or '', node, local ranks on that node) the binding would choose,
    from a sysfs tree under sysroot; no affinity change."""
    out = C.create_string_buffer(8192)
    node, peers = C.c_int(-1), C.c_int(0)
    check(lib().bwtmi_host_binding_plan(sysroot.encode(), local_rank, ",".join(rank_pci).encode(), threads, int(smt),
                                        allowed.encode(), out, len(out), C.byref(node), C.byref(peers)))
    return out.value.decode(), node.value, peers.value


def kernel_stats(h, enable: bool = True, reset: bool = True) -> dict:
    """{kernel: (total_ms, launches, algorithmic_bytes)} from HIP events on the ctx stream."""
    buf = C.create_string_buffer(1 << 16)
    check(lib().bwtmi_kernel_stats(h, int(enable), int(reset), buf, len(buf)))
    out = {}
    for line in buf.value.decode().splitlines():
        name, ms, n, b = line.split()
        out[name] = (float(ms), int(n), float(b))
    return out


def kernel_stats_filter(h, name: str = "") -> None:
    """Time only the launches named `name` ("" = every launch)."""
    check(lib().bwtmi_kernel_stats_filter(h, name.encode() if name else None))


def screen_hits(h, hits, text_len: int, min_copies: int = 3, drop: bool = False, maxlen: int = -1):
    """The device screen (bwtmi_screen_hits) on hits = int64[k,5] rows (start, end,
    unit_len, prim_len, copies): int64[j,4] rows (start, len, prim, cut) of the
    survivors in screen order."""
    import numpy as np
    hits = np.asarray(hits, dtype=np.int64).reshape(-1, 5)
    arr = np.zeros(max(len(hits), 1), dtype=[("start", "<i8"), ("end", "<i8"), ("unit_len", "<i4"),
                                             ("prim_len", "<i4"), ("copies", "<i8")])
    assert arr.dtype.itemsize == C.sizeof(Hit)
    for k, name in enumerate(arr.dtype.names):
        arr[name][:len(hits)] = hits[:, k]
    out, n = C.c_void_p(), C.c_int64(0)
    check(lib().bwtmi_screen_hits(h, arr.ctypes.data_as(C.c_void_p), len(hits), int(text_len), int(min_copies),
                                  int(bool(drop)), int(maxlen), C.byref(out), C.byref(n)))
    try:
        rows = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_int64)), shape=(max(n.value, 1) * 4,))
        return rows[:n.value * 4].reshape(-1, 4).copy()
    finally:
        lib().bwtmi_free(out)


CHAIN_PARAMS = ("max_gap", "bandwidth", "max_pred", "min_score", "min_anchors")


def chain_params(**kv) -> ChainParams:
    """bwtmi_chain_params from keyword arguments (absent or None: the default)."""
    bad = set(kv) - set(CHAIN_PARAMS) - {"reserved"}
    if bad:
        raise TypeError(f"unknown chain parameter(s): {', '.join(sorted(bad))}")
    p = ChainParams()
    for k in CHAIN_PARAMS:
        if kv.get(k) is not None:
            if int(kv[k]) <= 0:
                raise ValueError(f"{k} must be positive")
            setattr(p, k, int(kv[k]))
    for i, v in enumerate(kv.get("reserved") or ()):
        p.reserved[i] = int(v)
    return p


def take(p, dtype, count: int):
    """A copy of `count` elements of `dtype` at the library's malloc'd block p."""
    import numpy as np
    if not count:
        return np.zeros(0, dtype=dtype)
    return np.ctypeslib.as_array(C.cast(p, C.POINTER(np.ctypeslib.as_ctypes_type(dtype))), shape=(count,)).copy()


def chain_anchors(h, group_off, q, r, length, **params) -> dict:
    """The device chainer (bwtmi_chain_anchors) on anchors (q, r, length) in
    groups group_off[ng + 1]: a dict of chain_off, score, n_anchors, qstart, qend,
    rstart, rend, member_off, member (input indices) and evals.  ValueError on
    BWTMI_E_ARG."""
    import numpy as np
    go = np.ascontiguousarray(group_off, dtype=np.int64)
    aq, ar, al = (np.ascontiguousarray(a, dtype=t) for a, t in ((q, np.int32), (r, np.int64), (length, np.int32)))
    if go.ndim != 1 or go.size < 1 or not aq.size == ar.size == al.size:
        raise ValueError("group_off needs ng + 1 entries, q / r / length equal sizes")
    cp = chain_params(**params)
    ptrs = [C.c_void_p() for _ in range(9)]
    nc, nm, ev = C.c_int64(-1), C.c_int64(-1), C.c_int64(0)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
    rc = lib().bwtmi_chain_anchors(h, go.ctypes.data_as(C.c_void_p), go.size - 1, ptr(aq), ptr(ar), ptr(al), C.byref(cp),
                                   *[C.byref(p) for p in ptrs], C.byref(nc), C.byref(nm), C.byref(ev))
    if rc == -1:   # BWTMI_E_ARG: nothing was written
        untouched = all(p.value is None for p in ptrs) and nc.value == -1 and nm.value == -1
        msg = lib().bwtmi_last_error()
        raise ValueError((msg.decode(errors="replace") if msg else "bad argument") +
                         ("" if untouched else " [outputs were written]"))
    check(rc)
    try:
        n, ng = nc.value, go.size - 1
        names = ("chain_off", "score", "n_anchors", "qstart", "qend", "rstart", "rend", "member_off", "member")
        kinds = (np.int64, np.int32, np.int32, np.int32, np.int32, np.int64, np.int64, np.int64, np.int64)
        counts = (ng + 1, n, n, n, n, n, n, n + 1, nm.value)
        out = {k: take(p, t, c) for k, p, t, c in zip(names, ptrs, kinds, counts)}
        out["evals"] = ev.value
        return out
    finally:
        for p in ptrs:
            lib().bwtmi_free(p)


SELECT_PARAMS = ("mask", "pri_ratio", "best_n", "full")


def select_chains(h, chain_off, score, qstart, qend, mask=None, pri_ratio=None, best_n=None, full=None,
                  reserved=None) -> dict:
    """The device selection (bwtmi_select_chains) on chain rows (score, qstart,
    qend) in groups chain_off[ng + 1], one group per read: a dict of parent
    (int32, relative to the group's first chain), sub (int32), mapq, keep
    (uint8), n_primary and n_kept.  A parameter left None takes the library's
    default.  ValueError on BWTMI_E_ARG."""
    import numpy as np
    co = np.ascontiguousarray(chain_off, dtype=np.int64)
    sc, qs, qe = (np.ascontiguousarray(a, dtype=np.int32) for a in (score, qstart, qend))
    if co.ndim != 1 or co.size < 1 or not sc.size == qs.size == qe.size:
        raise ValueError("chain_off needs ng + 1 entries, score / qstart / qend equal sizes")
    if co[-1] != sc.size:
        raise ValueError(f"chain_off ends at {int(co[-1])}, the chain arrays hold {sc.size}")
    sp = SelectParams()
    for k, v in zip(SELECT_PARAMS, (mask, pri_ratio, best_n, full)):
        if v is not None and int(v) < 0:
            raise ValueError(f"{k} must not be negative")
        setattr(sp, k, -1 if v is None else int(v))
    for i, v in enumerate(reserved or ()):
        sp.reserved[i] = int(v)
    ptrs = [C.c_void_p() for _ in range(4)]
    npri, nkept = C.c_int64(0), C.c_int64(0)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None      # noqa: E731
    rc = lib().bwtmi_select_chains(h, co.ctypes.data_as(C.c_void_p), co.size - 1, ptr(sc), ptr(qs), ptr(qe), C.byref(sp),
                                   *[C.byref(p) for p in ptrs], C.byref(npri), C.byref(nkept))
    if rc == -1:   # BWTMI_E_ARG: every output pointer is NULL, every count 0
        clean = all(p.value is None for p in ptrs) and npri.value == 0 and nkept.value == 0
        msg = lib().bwtmi_last_error()
        raise ValueError((msg.decode(errors="replace") if msg else "bad argument") +
                         ("" if clean else " [outputs were written]"))
    check(rc)
    try:
        n = sc.size
        out = {k: take(p, t, n) for k, p, t in zip(("parent", "sub", "mapq", "keep"), ptrs,
                                                   (np.int32, np.int32, np.uint8, np.uint8))}
        out["n_primary"], out["n_kept"] = npri.value, nkept.value
        return out
    finally:
        for p in ptrs:
            lib().bwtmi_free(p)


# bwtmi_radix_sort kinds: name -> (code, key dtype, value dtype or None)
SORT_KINDS = {"k64v64": (0, "<u8", "<u8"), "k64v32": (1, "<u8", "<u4"), "k64": (2, "<u8", None),
              "k32v32": (3, "<u4", "<u4"), "k16v32": (4, "<u2", "<u4"), "pass_k32": (5, "<u4", "<u4")}
SCAN_KINDS = {"u32": (0, "<u4"), "i64": (1, "<i8")}


def radix_sort(h, kind: str, keys, vals, bit0: int, bit1: int, skew: int = 0):
    """The device radix sort (bwtmi_radix_sort) of `kind` (SORT_KINDS) on copies of
    keys / vals by the key bits [bit0, bit1): (sorted keys, their values or None).
    pass_k32: one pass by the digit at bit0."""
    import numpy as np
    code, kt, vt = SORT_KINDS[kind]
    k = np.array(keys, dtype=kt).reshape(-1)
    v = np.array(vals, dtype=vt).reshape(-1) if vt else None
    assert v is None or v.size == k.size
    check(lib().bwtmi_radix_sort(h, code, k.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p) if vt else None,
                                 k.size, int(bit0), int(bit1), int(skew)))
    return k, v


def exclusive_scan(h, kind: str, a, n: Optional[int] = None, rows: int = 1, stride: int = 0, skew: int = 0,
                   in_place: bool = False, epoch: int = 0, out=None):
    """The device exclusive scan (bwtmi_exclusive_scan) of `kind` (SCAN_KINDS) over
    `rows` rows of n elements of a, `stride` apart (one row: all of a).  Returns
    the output array; out of place it starts as a copy of `out` (zeros if None)."""
    import numpy as np
    code, dt = SCAN_KINDS[kind]
    a = np.ascontiguousarray(a, dtype=dt).reshape(-1)
    n = a.size if n is None else int(n)
    assert a.size == (rows - 1) * stride + n
    o = np.zeros_like(a) if out is None else np.array(out, dtype=dt).reshape(-1)
    assert o.size == a.size
    check(lib().bwtmi_exclusive_scan(h, code, a.ctypes.data_as(C.c_void_p), o.ctypes.data_as(C.c_void_p), n, int(rows),
                                     int(stride), int(skew), int(bool(in_place)), int(epoch)))
    return o


def host_info() -> dict:
    """CPUs visible to this process, ranks on the node, post-processing threads per rank."""
    v, lw, t = C.c_int32(), C.c_int32(), C.c_int32()
    check(lib().bwtmi_host_info(C.byref(v), C.byref(lw), C.byref(t)))
    return {"cpus_visible": v.value, "local_world": lw.value, "threads_per_rank": t.value}


def last_timing(h) -> tuple:
    out = (C.c_double * 3)()
    check(lib().bwtmi_last_timing(h, out))
    return tuple(out)
