"""The host side of the chain selection, without the library: MapResult.take
against a per-chain loop, merge_groups' group order and origins, and map_rows
with a Selection (column 12 and the tp:A: tag)."""
from types import SimpleNamespace

import numpy as np
import pytest

_COLS = ("strand", "score", "n_anchors", "qstart", "qend", "rstart", "rend")
_MEM = ("member_q", "member_r", "member_len")


def _result(per_query):
    """A MapResult of per_query = [[(strand, score, qstart, qend, rstart, rend, [(q, r, len), ...]), ...], ...]."""
    from bwtmi.core import MapResult
    chains = [c for q in per_query for c in q]
    off = np.concatenate([[0], np.cumsum([len(q) for q in per_query])]).astype(np.int64)
    moff = np.concatenate([[0], np.cumsum([len(c[6]) for c in chains])]).astype(np.int64)
    mem = [m for c in chains for m in c[6]]
    col = lambda k, t: np.array([c[k] for c in chains], dtype=t)      # noqa: E731
    mcol = lambda k, t: np.array([m[k] for m in mem], dtype=t)        # noqa: E731
    return MapResult(off, col(0, np.uint8), col(1, np.int32), np.array([len(c[6]) for c in chains], np.int32),
                     col(2, np.int32), col(3, np.int32), col(4, np.int64), col(5, np.int64), moff, mcol(0, np.int32),
                     mcol(1, np.int64), mcol(2, np.int32), positions_total=11, skipped_smems=2, anchors=9, evals=33)


def _hand_made():
    # query 0: a '+' chain of two anchors, a '-' chain of three (its member_q descend); query 1: one chain;
    # query 2: none; query 3: two chains
    return _result([
        [(0, 88, 5, 100, 1000, 1089, [(5, 1000, 45), (56, 1045, 44)]),
         (1, 70, 10, 95, 200, 285, [(70, 200, 25), (40, 230, 25), (10, 260, 25)])],
        [(0, 40, 0, 40, 7, 47, [(0, 7, 40)])],
        [],
        [(0, 30, 0, 30, 400, 430, [(0, 400, 30)]), (1, 25, 2, 27, 900, 925, [(12, 900, 15), (2, 915, 10)])]])


def _take_by_loop(res, keep):
    """What take must give, chain by chain."""
    off, moff = [0], [0]
    cols, mem = {k: [] for k in _COLS}, {k: [] for k in _MEM}
    for q in range(len(res)):
        for k in range(int(res.offsets[q]), int(res.offsets[q + 1])):
            if not keep[k]:
                continue
            for name in _COLS:
                cols[name].append(getattr(res, name)[k])
            for name in _MEM:
                mem[name] += getattr(res, name)[int(res.member_offsets[k]):int(res.member_offsets[k + 1])].tolist()
            moff.append(len(mem["member_q"]))
        off.append(len(cols["score"]))
    return off, moff, cols, mem


def _same_arrays(a, b):
    for name in ("offsets", "member_offsets") + _COLS + _MEM:
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == y.dtype and x.tolist() == y.tolist(), name


@pytest.mark.parametrize("keep", [[0, 0, 0, 0, 0], [1, 1, 1, 1, 1], [1, 1, 0, 1, 1], [0, 1, 1, 0, 1], [1, 0, 0, 0, 0],
                                  [0, 0, 0, 0, 2]])
def test_take_against_a_per_chain_loop(keep):
    res = _hand_made()
    got = res.take(np.array(keep, dtype=np.uint8))
    off, moff, cols, mem = _take_by_loop(res, keep)
    assert got.offsets.tolist() == off and got.member_offsets.tolist() == moff
    assert got.offsets.dtype == got.member_offsets.dtype == np.int64
    for name in _COLS + _MEM:
        want = {**cols, **mem}[name]
        assert getattr(got, name).tolist() == want and getattr(got, name).dtype == getattr(res, name).dtype, name
    assert (got.positions_total, got.skipped_smems, got.anchors, got.evals) == (11, 2, 9, 33)
    assert len(got) == len(res) == 4


def test_take_edges():
    res = _hand_made()
    _same_arrays(res.take(np.ones(5, bool)), res)                  # all true: the input's arrays
    none = res.take(np.zeros(5, bool))
    assert none.offsets.tolist() == [0] * 5 and none.member_offsets.tolist() == [0] and none.score.size == 0
    mid = res.take([1, 1, 0, 1, 1])                                # query 1 loses its only chain
    assert mid.offsets.tolist() == [0, 2, 2, 2, 4] and mid.member_offsets.tolist() == [0, 2, 5, 6, 8]
    minus = res.take([0, 1, 0, 0, 1])                              # the strand-1 chains keep their member order
    assert minus.strand.tolist() == [1, 1] and minus.member_q.tolist() == [70, 40, 10, 12, 2]
    assert minus.members(0).tolist() == res.members(1).tolist() and minus.members(1).tolist() == res.members(4).tolist()
    _same_arrays(mid.take([1, 0, 1, 0]), res.take([1, 0, 0, 1, 0]))  # take composes
    with pytest.raises(ValueError, match="keep"):
        res.take([1, 0])
    empty = _result([[], []])
    assert empty.take([]).offsets.tolist() == [0, 0, 0]


def test_merge_groups_order_and_origin():
    from bwtmi import merge_groups
    from bwtmi.select import merge_groups as same
    assert merge_groups is same
    c = lambda score, qs, qe: (0, score, qs, qe, 0, qe - qs, [(qs, 0, qe - qs)])      # noqa: E731
    r0 = _result([[c(10, 0, 5), c(11, 1, 6)], [], [c(12, 2, 7)], []])
    r1 = _result([[], [], [c(20, 0, 9), c(21, 1, 9), c(22, 2, 9)], []])
    r2 = _result([[c(30, 3, 4)], [c(31, 4, 5)], [c(32, 5, 6)], []])
    m = merge_groups([r0, r1, r2])
    assert m["chain_off"].tolist() == [0, 3, 4, 9, 9] and m["chain_off"].dtype == np.int64
    assert m["score"].tolist() == [10, 11, 30, 31, 12, 20, 21, 22, 32] and m["score"].dtype == np.int32
    assert m["qstart"].tolist() == [0, 1, 3, 4, 2, 0, 1, 2, 5] and m["qend"].tolist() == [5, 6, 4, 5, 7, 9, 9, 9, 6]
    assert m["origin"].tolist() == [[0, 0], [0, 1], [2, 0], [2, 1], [0, 2], [1, 0], [1, 1], [1, 2], [2, 2]]
    for k, (i, j) in enumerate(m["origin"].tolist()):              # origin round-trips
        r = (r0, r1, r2)[i]
        assert (m["score"][k], m["qstart"][k], m["qend"][k]) == (r.score[j], r.qstart[j], r.qend[j])
    for i, r in enumerate((r0, r1, r2)):                            # every chain once, a result's chains in order
        assert m["origin"][m["origin"][:, 0] == i, 1].tolist() == list(range(r.score.size))
    one = merge_groups([r1])
    assert one["chain_off"].tolist() == r1.offsets.tolist() and one["origin"][:, 1].tolist() == [0, 1, 2]
    none = merge_groups([_result([[], []]), _result([[], []])])
    assert none["chain_off"].tolist() == [0, 0, 0] and none["origin"].shape == (0, 2)
    with pytest.raises(ValueError, match="queries"):
        merge_groups([r0, _result([[c(1, 0, 1)]])])
    with pytest.raises(ValueError):
        merge_groups([])


def test_map_rows_with_a_selection():
    from bwtmi.map import map_rows
    from bwtmi.select import Selection
    res = _hand_made()
    names, qlens = ["r0", "r1", "r2", "r3"], [100, 77, 30, 30]
    plain = map_rows("chr1", 5000, names, qlens, res)
    assert plain[0] == "r0\t100\t5\t100\t+\tchr1\t5000\t1000\t1089\t89\t95\t255\ts1:i:88\tcm:i:2\tdl:i:6\n"
    assert map_rows("chr1", 5000, names, qlens, res, None, None) == plain and all("tp:A:" not in r for r in plain)
    sel = Selection(np.array([1, 0, 1, 1, 0], bool), np.array([13, 0, 60, 24, 0], np.uint8), np.array([70, 0, 0, 25, 0]),
                    np.ones(5, bool), np.zeros(5, np.int32), np.array([0, 0, 2, 3, 3]))
    rows = map_rows("chr1", 5000, names, qlens, res, sel=sel)
    assert [r.split("\t")[11] for r in rows] == ["13", "0", "60", "24", "0"]
    assert [r.rstrip("\n").split("\t")[12:] for r in rows][0] == ["s1:i:88", "cm:i:2", "dl:i:6", "tp:A:P"]
    assert [r.rstrip("\n").split("\t")[15] for r in rows] == ["tp:A:P", "tp:A:S", "tp:A:P", "tp:A:P", "tp:A:S"]
    for a, b in zip(plain, rows):                                   # nothing else moves
        a, b = a.rstrip("\n").split("\t"), b.rstrip("\n").split("\t")
        assert a[:11] == b[:11] and a[12:] == b[12:15] and len(b) == 16
    # with an alignment the tag stands between dl:i: and NM:i:
    aln = SimpleNamespace(qstart=res.qstart, qend=res.qend, rstart=res.rstart, rend=res.rend,
                          n_eq=np.array([89, 75, 40, 30, 25]), cols=np.array([95, 85, 40, 30, 25]),
                          nm=np.array([6, 10, 0, 0, 0]), cigar_string=lambda k: f"{k}=")
    both = map_rows("chr1", 5000, names, qlens, res, aln, sel)
    assert both[1].rstrip("\n").split("\t")[11:] == ["0", "s1:i:70", "cm:i:3", "dl:i:0", "tp:A:S", "NM:i:10", "cg:Z:1="]
    assert [r.replace("\ttp:A:P", "").replace("\ttp:A:S", "").split("\t")[:11] for r in both] == \
        [r.split("\t")[:11] for r in map_rows("chr1", 5000, names, qlens, res, aln)]
    # the rows of a cut selection go with the cut result
    keep = [1, 0, 0, 1, 1]
    cut = map_rows("chr1", 5000, names, qlens, res.take(keep), sel=sel.take(keep))
    assert cut == [rows[0], rows[3], rows[4]]


def test_map_parser_select_flags():
    from bwtmi import map as mapcli
    a = mapcli.build_parser().parse_args(["in.fa", "reads.txt", "-o", "o"])
    assert (a.select, a.mask_level, a.pri_ratio, a.best_n, a.mapq_full) == (False, None, None, None, None)
    a = mapcli.build_parser().parse_args(["in.fa", "reads.txt", "--select", "--mask-level", "40", "--pri-ratio", "70",
                                          "--best-n", "0", "--mapq-full", "250", "-o", "o"])
    assert (a.select, a.mask_level, a.pri_ratio, a.best_n, a.mapq_full) == (True, 40, 70, 0, 250)
