"""bench.py's own options: --steps sets the timed steps and the line carries
ms_per_step, a plain run leaves the legs with runs of their own to --full,
and --dump-outputs writes the last timed step's outputs, the same from run to
run.  Small contigs (--contig-bp): the options, not the speed, are under test."""
import hashlib
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")
SMALL = ["--gpus", "1", "--contig-bp", "300000"]


def _bench_mod():
    spec = importlib.util.spec_from_file_location("bench_mod", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _run(args, tmp):
    env = dict(os.environ, TMPDIR=str(tmp))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, BENCH] + list(args), capture_output=True, text=True, env=env, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_sample_rows_is_fixed_and_bounded():
    bench = _bench_mod()
    a = np.arange(1000 * 9, dtype=np.float64).reshape(1000, 9)
    assert bench.sample_rows(a, a.nbytes) is a                 # fits: the array itself
    s1, s2 = bench.sample_rows(a, 10_000), bench.sample_rows(a.copy(), 10_000)
    assert s1.shape == (10_000 // 72, 9) and s1.nbytes <= 10_000
    assert (s1 == s2).all()                                    # the same rows every time
    assert (np.diff(s1[:, 0]) > 0).all()                       # rows of a, in a's order, none twice
    b = np.arange(50, dtype=np.uint8)
    assert bench.sample_rows(b, 20).shape == (20,)
    assert bench.sample_rows(a[:0], 100).shape == (0, 9)
    assert sum(bench.DUMP_BUDGET.values()) <= 64_000_000 - 3 * 4096


def test_bench_rejects_zero_steps():
    p = subprocess.run([sys.executable, BENCH, "--steps", "0"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and "--steps" in p.stderr


@pytest.fixture(scope="module")
def plain_run(gpu_ctx, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("bench_plain")
    out = tmp / "dump"
    line = _run(SMALL + ["--steps", "3", "--warmup", "1", "--dump-outputs", str(out)], tmp)
    return line, str(out), tmp


@pytest.mark.gpu
def test_plain_run_line_and_dump(plain_run):
    line, out, _ = plain_run
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
    assert line["ms_per_step"] > 0 and line["unit"] == "Mbp/s" and line["higher_is_better"] is True
    # value is the bases of one step over ms_per_step (both rounded to 3 decimals in the line)
    assert line["value"] == pytest.approx(0.3 / (line["ms_per_step"] / 1e3), rel=5e-3)
    assert line["calls_ms_per_step"]["scan"] > 0
    # the legs with runs of their own are left to --full
    assert line["cpu_baseline"] is None and line["fm_all_motifs_1_10"] is None and line["cli_drop_in"] is None
    arrs = _load(out)
    assert sorted(arrs) == ["records_float", "records_int", "repeat_tab_bytes"]
    assert {k: list(v.shape) for k, v in arrs.items()} == line["dumped_outputs"]
    assert arrs["records_int"].dtype == np.float64 and arrs["records_float"].dtype == np.float64
    assert arrs["repeat_tab_bytes"].dtype == np.float32
    assert sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out)) <= 64_000_000
    n = arrs["records_int"].shape[0]
    assert n > 0 and arrs["records_int"].shape == (n, 9) and arrs["records_float"].shape == (n, 5)
    # small output: nothing sampled, so the dump is the file the line hashed
    data = arrs["repeat_tab_bytes"].astype(np.uint8).tobytes()
    assert hashlib.sha256(data).hexdigest() == line["output_sha256"]
    assert data.count(b"\n") - 1 == line["rows"]
    ints = arrs["records_int"]
    assert (ints == np.floor(ints)).all() and (ints[:, 1] > ints[:, 0]).all()      # end > start


@pytest.mark.gpu
def test_dump_is_the_same_from_run_to_run(plain_run):
    line, out, tmp = plain_run
    out2 = tmp / "dump2"
    line2 = _run(SMALL + ["--steps", "3", "--warmup", "1", "--dump-outputs", str(out2)], tmp)
    assert line2["output_sha256"] == line["output_sha256"]
    a, b = _load(out), _load(str(out2))
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].shape == b[k].shape and (a[k] == b[k]).all(), k


@pytest.mark.gpu
def test_full_run_adds_the_other_legs(plain_run):
    line, _, tmp = plain_run
    full = _run(SMALL + ["--steps", "1", "--warmup", "1", "--full", "--cpu-sample-bp", "100000"], tmp)
    assert full["full"] is True and full["steps"] == 1 and full["dumped_outputs"] is None
    assert full["output_sha256"] == line["output_sha256"]
    assert full["cpu_baseline"]["value"] > 0 and full["cpu_baseline"]["kind"] == "port"
    assert full["fm_all_motifs_1_10"]["patterns"] == 145338 and full["fm_all_motifs_1_10"]["found"] > 0
    assert full["cli_drop_in"]["output_sha256"] == line["output_sha256"]
    assert len(full["cli_drop_in"]["wall_s"]) == 2
