"""Selection of a read's chains over every contig: which chain is the read's
placement (primary), which are echoes of it (secondary), the primary's mapping
quality and which secondaries are worth keeping (include/bwtmi.h,
bwtmi_select_chains, states the contract).

`map.py` builds one index per contig, so a read's chains arrive as one
MapResult per contig.  The decision must see all of them at once: a read's copy
on contig B earns no confident MAPQ when contig A holds a better one.
merge_groups lays the contigs' chains of every read back to back (numpy only),
the device decides, and select_chains cuts the answer back into one Selection
per MapResult.
"""
from __future__ import annotations

from typing import List, Sequence

import numpy as np


class Selection:
    """The selection's answer for the chains of one MapResult, aligned to them:
    `primary` (bool), `mapq` (uint8; 0 for a secondary), `sub` (int32: the score
    of a primary's best secondary, else 0), `keep` (bool), and the parent's
    origin `parent_result` (int32: the index of its MapResult in the list the
    selection ran on) and `parent_chain` (int64: its chain index there); a
    primary is its own parent.  `n_primary` and `n_kept` are the counts of the
    whole call, over every MapResult of the list."""

    __slots__ = ("primary", "mapq", "sub", "keep", "parent_result", "parent_chain", "n_primary", "n_kept")

    def __init__(self, primary, mapq, sub, keep, parent_result, parent_chain, n_primary=0, n_kept=0):
        self.primary, self.mapq, self.sub, self.keep = primary, mapq, sub, keep
        self.parent_result, self.parent_chain = parent_result, parent_chain
        self.n_primary, self.n_kept = n_primary, n_kept

    def __len__(self):
        return self.keep.size

    def take(self, keep) -> "Selection":
        """The rows with keep != 0, in their order: the Selection of
        MapResult.take(keep)'s chains.  parent_chain still names the chain in
        the MapResult the selection ran on."""
        keep = np.asarray(keep).astype(bool).reshape(-1)
        if keep.size != self.keep.size:
            raise ValueError(f"keep has {keep.size} flags for {self.keep.size} chains")
        return Selection(self.primary[keep], self.mapq[keep], self.sub[keep], self.keep[keep], self.parent_result[keep],
                         self.parent_chain[keep], self.n_primary, self.n_kept)


def merge_groups(results: Sequence) -> dict:
    """The chains of `results` (MapResults over the same nq queries, one per
    contig) as one group per query: chain_off (int64[nq + 1]), score, qstart,
    qend (int32) and origin (int64[n, 2] rows (result index, chain index)).
    Query q's group is its chains of results[0] in that result's order, then
    those of results[1], and so on.  ValueError when the results differ in nq."""
    results = list(results)
    if not results:
        raise ValueError("merge_groups needs at least one result")
    offs = [np.asarray(r.offsets, dtype=np.int64) for r in results]
    nq = offs[0].size - 1
    for i, o in enumerate(offs):
        if o.size - 1 != nq:
            raise ValueError(f"result {i} holds {o.size - 1} queries, result 0 holds {nq}")
    counts = np.stack([o[1:] - o[:-1] for o in offs], axis=1)               # [nq, nres]
    chain_off = np.concatenate([[0], np.cumsum(counts.sum(axis=1), dtype=np.int64)])
    # where the chains of (query q, result i) start in the merged order: query-major, then result
    flat = counts.reshape(-1)
    start = (np.cumsum(flat, dtype=np.int64) - flat).reshape(counts.shape)
    n = int(chain_off[-1])
    score, qstart, qend = (np.zeros(n, dtype=np.int32) for _ in range(3))
    origin = np.zeros((n, 2), dtype=np.int64)
    for i, (r, o) in enumerate(zip(results, offs)):
        c = counts[:, i]
        own = np.repeat(np.arange(nq, dtype=np.int64), c)                    # the query of each chain of result i
        k = np.arange(own.size, dtype=np.int64)
        at = start[own, i] + (k - o[:-1][own]) if own.size else k
        score[at], qstart[at], qend[at] = np.asarray(r.score), np.asarray(r.qstart), np.asarray(r.qend)
        origin[at, 0], origin[at, 1] = i, k
    return {"chain_off": chain_off, "score": score, "qstart": qstart, "qend": qend, "origin": origin}


def select_chains(results, ctx=None, **params) -> List[Selection]:
    """One Selection per MapResult of `results` (a list over the same queries,
    one per contig; a single MapResult may be passed bare), from one device
    call over all of them.  params: mask, pri_ratio, best_n, full (absent or
    None: the library's defaults 50, 80, 5, 100).  ctx: the device context
    (default: the process's).  ValueError as bwtmi._lib.select_chains raises it."""
    from . import _lib
    if hasattr(results, "offsets"):
        results = [results]
    results = list(results)
    m = merge_groups(results)
    got = _lib.select_chains(_lib.ctx() if ctx is None else ctx, m["chain_off"], m["score"], m["qstart"], m["qend"],
                             **params)
    n = m["score"].size
    group = np.repeat(np.arange(m["chain_off"].size - 1, dtype=np.int64), np.diff(m["chain_off"]))
    par = m["chain_off"][:-1][group] + got["parent"] if n else np.zeros(0, dtype=np.int64)   # the parent's merged index
    primary = par == np.arange(n, dtype=np.int64)
    out = []
    for i in range(len(results)):
        rows = np.flatnonzero(m["origin"][:, 0] == i)      # ascending: the result's chains in their order
        p = par[rows]
        out.append(Selection(primary[rows], got["mapq"][rows], got["sub"][rows], got["keep"][rows].astype(bool),
                             m["origin"][p, 0].astype(np.int32), m["origin"][p, 1].astype(np.int64),
                             got["n_primary"], got["n_kept"]))
    return out
