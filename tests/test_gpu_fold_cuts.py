"""The cut bit of the device screen (nested.hip) and the one pass over cut
segments that reads it (post.cpp fold_cuts): with BWTMI_FOLD_CUTS=1 (the
default) a device-screened contig gives the same records as with
BWTMI_FOLD_CUTS=0 (the same pass with the bits ignored: one segment, the serial
fold), whatever the screen's other switches, in both download layouts, and the
device's bits are the host's (BWTMI_DEVICE_CHECKS=1)."""
import pytest

pytestmark = pytest.mark.gpu


def _scan_render(contigs, mc=3, max_unit_len=120, fmt="strfinder"):
    from bwtmi import _lib
    from bwtmi.records import Job
    j = Job(min_copies=mc, max_unit_len=max_unit_len, show_progress=True)
    for name, seq in contigs:
        j.add_contig(name, seq, 30, 30)
    j.scan(_lib.ctx())
    j.postprocess()
    return j.render(fmt)


@pytest.fixture(scope="module")
def contigs():
    from bwtmi import synth
    return {
        "plain": [("c1", synth.generate_contig(1_500_000, 71, 0.0))],
        "gaps": [("c2", synth.generate_contig(1_200_000, 72, 0.0, gaps="n2"))],
        "imperfect": [("c3", synth.generate_contig(1_000_000, 73, 0.02))],
    }


@pytest.fixture(scope="module")
def general_path(gpu_ctx, contigs):
    """The records without cuts (FOLD_CUTS=0: one segment), computed once."""
    from bwtmi import _lib
    with _lib.knobs(FOLD_CUTS=0):
        return {k: _scan_render(v) for k, v in contigs.items()}


@pytest.mark.parametrize("switches", [{}, {"SCREEN_DROP": 0}, {"SCREEN_WIDE": 1}, {"DEVICE_CHECKS": 1},
                                      {"DEVICE_CHECKS": 1, "SCREEN_DROP": 0}, {"FOLD_CHUNK": 64}],
                         ids=lambda d: "-".join(f"{k}{v}" for k, v in d.items()) or "default")
@pytest.mark.parametrize("case", ["plain", "gaps", "imperfect"])
def test_device_cut_bits_one_pass_matches_general_path(gpu_ctx, contigs, general_path, case, switches):
    from bwtmi import _lib
    with _lib.knobs(FOLD_CUTS=1, **switches):
        got = _scan_render(contigs[case])
    assert got == general_path[case]
    assert got.count(b"\n") > 100


def test_one_pass_runs_and_cuts_are_frequent(gpu_ctx, contigs, capfd):
    """The stage line of the one pass on device-screened hits: about half the hits
    are cuts on the generator's contigs."""
    import re
    from bwtmi import _lib
    capfd.readouterr()
    with _lib.knobs(FOLD_CUTS=1, STATS=1):
        _scan_render(contigs["plain"])
    err = capfd.readouterr().err
    m = re.search(r"one pass .*?(\d+) hits, (\d+) cuts", err)
    assert m, err[-800:]
    assert int(m.group(1)) > 1000 and int(m.group(2)) * 5 > int(m.group(1)), err[-800:]


def test_single_base_contig_takes_the_wide_layout(gpu_ctx):
    """A 2.2 Mbp contig of one base with max_unit_len 2000: the longest span needs
    22 bits and the longest motif 11, so the cut bit has no room in one word and
    the records come down in two."""
    from bwtmi import _lib
    seq = b"ACGTTGCA" * 8 + b"A" * 2_200_000 + b"TGCAACGT" * 8
    out = []
    for cuts in (0, 1):
        with _lib.knobs(FOLD_CUTS=cuts, DEVICE_CHECKS=cuts):
            out.append(_scan_render([("a", seq)], max_unit_len=2000))
    assert out[0] == out[1] and out[0].count(b"\n") >= 2


def test_c4_shape_several_one_contig_units(gpu_ctx):
    """The C4 shape with 200 kbp contigs: eight contigs, each a fold unit of its own."""
    from bwtmi import _lib, synth
    cs = [(f"contig{k}", synth.generate_contig(200_000, k, 0.0)) for k in range(1, 9)]
    out = []
    for cuts in (0, 1):
        with _lib.knobs(FOLD_CUTS=cuts):
            out.append(_scan_render(cs))
    assert out[0] == out[1] and out[0].count(b"\n") > 1000


def test_unit_of_device_screened_contigs_with_two_trim_offsets(gpu_ctx, tmp_path):
    """chr01 / CHR1 / chr1 in one fold unit (chr1 at offset 0) next to chr2, a unit
    of its own, through the device scan and screen: the unit of several screened
    contigs, and with FOLD_CUTS=0 chr2's screened hits with their bits ignored,
    against the reference post-processing."""
    from oracle import post
    from bwtmi import TandemRepeatFinder, _lib
    from test_fold_cuts import COLLIDING, write_colliding_fasta
    fa = str(tmp_path / "colliding.fa")
    write_colliding_fasta(fa)
    want = post.run_file(fa, "bed")
    for name in COLLIDING + ("chr2",):
        assert "\n" + name + "\t" in "\n" + want, name
    for cuts in (0, 1):
        with _lib.knobs(FOLD_CUTS=cuts):
            f = TandemRepeatFinder(fa)
            f.load_reference()
            reps = f.find_tandem_repeats_parallel()
            out = tmp_path / f"cuts{cuts}.bed"
            f.save_results(reps, str(out), "bed")
        assert out.read_text() == want, cuts
