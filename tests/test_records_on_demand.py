"""Records on demand: postprocess keeps the fold's survivors and the writers
read those; Recs are built by the first reader that asks for records (the
record view, the string getters, export), once, whoever asks and from whichever
thread, and before anything that changes them."""
import threading

import pytest

import oracle
from oracle import post

TRIM = 30


@pytest.fixture(scope="module")
def contig():
    from bwtmi import synth
    seq = synth.generate_contig(200_000, 8, 0.02)
    return seq, oracle.strict_scan(seq[TRIM:len(seq) - TRIM], 1, 1000, 0, 3)


def _job(contig, threads=4, name="c8"):
    from bwtmi.records import Job
    seq, hits = contig
    j = Job(min_copies=3, show_progress=True, threads=threads)
    j.add_contig(name, seq, TRIM, TRIM)
    j.add_hits(0, hits)
    j.postprocess()
    return j


@pytest.fixture(scope="module")
def want(contig):
    """The oracle's records and the export of a job nobody wrote from."""
    seq, hits = contig
    s = seq[TRIM:len(seq) - TRIM].decode()
    p = post.Pipeline({"c8": s}, {"c8": seq.decode()}, {"c8": TRIM}, 3)
    recs = p.run(post.worker_records("c8", s, hits))
    return p, recs, _job(contig).export()


def test_count_is_known_before_any_record_is_built(contig, want, built_lib):
    p, recs, blob = want
    j = _job(contig)
    assert j.count() == len(recs) > 500
    assert j.stage_ms()[5] == 0.0                  # nothing was built inside postprocess
    assert list(j.unit_rows()) == [len(recs)]
    got = j.records()
    assert len(got) == len(recs)
    for k in (0, 1, len(recs) // 2, len(recs) - 1):
        a, b = got[k], recs[k]
        assert (a.start, a.end, a.motif, a.copies, a.mismatch_rate, a.variations, a.actual_sequence, a.score) == \
               (b.start, b.end, b.motif, b.copies, b.mismatch_rate, b.variations, b.actual_sequence, b.score), k


def test_records_are_the_same_whenever_they_are_asked_for(contig, want, tmp_path, built_lib):
    p, recs, blob = want
    before = _job(contig)
    assert before.export() == blob
    text = before.render("strfinder")
    assert text.decode() == post.render(p, recs, "strfinder")
    after_one = _job(contig)
    after_one.write("strfinder", str(tmp_path / "a.tab"))
    assert after_one.export() == blob and (tmp_path / "a.tab").read_bytes() == text
    after_two = _job(contig)
    after_two.write("bed", str(tmp_path / "b.bed"))
    after_two.write("strfinder", str(tmp_path / "b.tab"))
    assert after_two.export() == blob and (tmp_path / "b.tab").read_bytes() == text
    # the writers give the same text once the records exist
    assert after_two.render("strfinder") == text


def test_views_of_records_and_of_survivors_give_the_same_text(contig, want, built_lib):
    """The writers read the survivors while the job holds them and Recs after
    that: a job whose records were built and taken over (import of nothing
    releases the survivors) against one that still holds its survivors, and the
    oracle, in every format."""
    import struct
    p, recs, blob = want
    held, owned = _job(contig), _job(contig)
    owned.import_records(struct.pack("<q", 0))
    assert owned.count() == held.count() == len(recs) and owned.export() == blob
    for fmt in ("strfinder", "bed", "vcf", "trf_table", "trf_dat"):
        text = owned.render(fmt)
        assert text == held.render(fmt), fmt
        assert text.decode() == post.render(p, recs, fmt), fmt


def test_two_threads_ask_at_once(contig, want, built_lib):
    p, recs, blob = want
    j = _job(contig)
    got, errs = [None, None], []

    def ask(k):
        try:
            got[k] = j.export() if k else [(r.start, r.end, r.motif, r.variations) for r in j.records()]
        except Exception as e:                      # noqa: BLE001
            errs.append(e)
    ts = [threading.Thread(target=ask, args=(k,)) for k in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs
    assert got[1] == blob
    assert got[0] == [(r.start, r.end, r.motif, r.variations) for r in recs]


def test_set_and_import_records_after_postprocess(contig, want, built_lib):
    from bwtmi.records import Job
    p, recs, blob = want
    seq = contig[0]
    j = _job(contig)
    kept = [r for r in j.records() if r.copies >= 5]
    j.set_records(kept, {"c8": seq.decode()})
    assert j.count() == len(kept) < len(recs)
    assert j.render("bed").decode() == post.render(p, [r for r in recs if r.copies >= 5], "bed")
    # import appends to what the job holds and keeps the order
    a, b = _job(contig), Job(min_copies=3, show_progress=True, threads=2)
    b.add_contig("c8", seq, TRIM, TRIM)
    b.import_records(blob)
    assert b.count() == len(recs) and b.export() == blob and b.render("vcf") == a.render("vcf")
    a.import_records(blob)                          # after postprocess: the survivors' records first
    assert a.count() == 2 * len(recs)
    starts = [r.start for r in a.records()]
    assert starts == sorted(starts) and starts[0::2] == starts[1::2] == [r.start for r in recs]


def test_reset_leaves_no_records(contig, built_lib):
    j = _job(contig)
    j.reset()
    assert j.count() == 0 and len(j.records()) == 0
    assert j.render("bed").count(b"\n") == 2        # the header
    j2 = _job(contig)
    assert len(j2.records()) > 0
    j2.reset()
    assert j2.count() == 0 and len(j2.records()) == 0


def test_background_write_then_reset_and_a_new_load(contig, want, tmp_path, built_lib):
    from bwtmi import synth
    p, recs, blob = want
    fa = str(tmp_path / "one.fa")
    seq = contig[0]
    with open(fa, "wb") as f:
        f.write(b">c8\n" + seq + b"\n")
    other = str(tmp_path / "other.fa")
    synth.write_fasta(other, [150_000], 0.0, first_index=3)
    from bwtmi.records import Job
    j = Job(min_copies=3, show_progress=True, threads=4)
    j.load_fasta(fa, TRIM)
    j.add_hits(0, contig[1])
    j.postprocess()
    out = tmp_path / "bg.tab"
    j.write("strfinder", str(out), background=True)
    j.reset()
    j.load_fasta(other, TRIM)
    j.write_join()
    assert out.read_text() == post.render(p, recs, "strfinder")
    assert j.count() == 0


def test_a_failure_building_the_records_is_reported_and_leaves_them_pending(contig, want, built_lib):
    from bwtmi import _lib
    p, recs, blob = want
    j = _job(contig)
    with _lib.knobs(FAIL_MATERIALISE=1):
        with pytest.raises(_lib.BwtmiError, match="injected failure"):
            j.export()
        with pytest.raises(_lib.BwtmiError, match="injected failure"):
            j.records()
        assert j.count() == len(recs)
    assert j.export() == blob
    assert j.render("strfinder").decode() == post.render(p, recs, "strfinder")
