"""bench.py's own contract: --steps sets the timed steps, --dump-outputs writes the last step's k-NN lists (float64, at
most 64 MB, the same seeded rows every run), and a plain run times the headline only while --full adds the rest.

CPU side: the dump's row sample and size bound, and argument checks that fail before any device is touched.  GPU side:
a small workload run plain twice (same files both times, equal to the oracle) and once with --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
import oracle
from nabo_amd._synth import pca_like

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(d):
    return {name: np.load(os.path.join(d, name + ".npy")) for name in ("rows", "indices", "distances")}


def test_dump_outputs_writes_every_row_when_it_fits(tmp_path):
    rng = np.random.default_rng(3)
    gi = rng.integers(0, 1 << 40, size=(1000, 7))
    gd = np.sort(rng.random((1000, 7)), axis=1)
    bench.dump_outputs(str(tmp_path), gi, gd)
    out = _load(str(tmp_path))
    assert all(a.dtype == np.float64 for a in out.values())
    assert np.array_equal(out["rows"], np.arange(1000))
    assert np.array_equal(out["indices"].astype(np.int64), gi) and np.array_equal(out["distances"], gd)


def test_dump_outputs_samples_the_same_rows_within_the_size_bound(tmp_path):
    m, k = 300000, 15                   # 300k x 15 x (indices + distances) in float64 = 72 MB: more than the bound
    gi = np.arange(m * k, dtype=np.int64).reshape(m, k)
    gd = gi * 0.5
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, gi, gd)
    bench.dump_outputs(b, gi, gd)
    total = sum(os.path.getsize(os.path.join(a, f)) for f in os.listdir(a))
    assert 60 * 10**6 < total <= 64 * 10**6
    oa, ob = _load(a), _load(b)
    rows = oa["rows"].astype(np.int64)
    assert len(rows) < m and (np.diff(rows) > 0).all() and rows[0] >= 0 and rows[-1] < m
    assert all(np.array_equal(oa[key], ob[key]) for key in oa)
    assert np.array_equal(oa["indices"].astype(np.int64), gi[rows]) and np.array_equal(oa["distances"], gd[rows])


@pytest.mark.parametrize("args", [["--steps", "0"], ["--warmup", "-1"]])
def test_bench_refuses_a_run_without_timed_steps(args):
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + args, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, universal_newlines=True, timeout=120, cwd=REPO)
    assert r.returncode != 0 and "--steps must be >= 1" in r.stderr and not r.stdout.strip()


def _bench(args):
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--targets", "20001", "--refs", "50000"] + args
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=600, cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_plain_run_dumps_the_last_step_and_full_run_adds_the_rest(gpu_lib, tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    line = _bench(["--steps", "3", "--warmup", "1", "--dump-outputs", a])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line, key
    assert line["steps"] == 3 and line["warmup"] == 1 and line["higher_is_better"] is True
    assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(20001 * 50000 / (line["ms_per_step"] * 1e-3))
    assert line["sampled_rows_equal_oracle"] is None
    assert not {"cpu_baseline", "alt", "alt_f16x3", "canberra", "config4_one_gpu"} & set(line)
    _bench(["--steps", "1", "--warmup", "0", "--dump-outputs", b])
    oa, ob = _load(a), _load(b)
    assert all(np.array_equal(oa[key], ob[key]) for key in oa)             # same inputs, same bits, run to run
    assert np.array_equal(oa["rows"], np.arange(20001))
    # the dump is what the step computed: the oracle's lists on a row sample (bench.py's inputs, regenerated)
    X, Y = pca_like(20001, 50, seed=2003), pca_like(50000, 50, seed=1003)
    rows = np.random.default_rng(5).choice(20001, 64, replace=False)
    oi, od = oracle.knn(X[rows], Y, 15, oracle.EUCLIDEAN, 0.25, nthreads=8)
    assert np.array_equal(oa["indices"][rows], oi) and np.array_equal(oa["distances"][rows], od)

    full = _bench(["--steps", "1", "--warmup", "1", "--full", "--no-cpu-baseline"])
    assert full["sampled_rows_equal_oracle"] is True and full["alt"]["same_bits_as_headline_path"] is True
