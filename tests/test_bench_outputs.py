"""`bench.py --dump-outputs DIR` and the plain / `--full` split of the line.  The writer is checked on the host (size limit, the
sample is the same from call to call); the GPU tests run the benchmark itself at a small size, once plain and once with `--full`,
and compare what it wrote with the oracle on the same seeded inputs (tolerances of BASELINE.md section 5)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")

TOL_MEAN = 1e-9       # relative to max |mean|
TOL_VAR = 1e-9        # absolute, times sf^2
TOL_LML = 1e-11       # relative

HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus")
FULL_ONLY_KEYS = ("roofline", "cholesky", "gram", "e2e_ms_per_step", "mfma_f64_probe_tflops", "c3_sharded", "cpu_baseline", "cpu_opt_baseline")


def _bench():
    sys.path.insert(0, ROOT)
    import importlib
    return importlib.import_module("bench")


def test_dump_writes_float64_npy_files(tmp_path):
    bench = _bench()
    a = np.arange(12, dtype=np.float32).reshape(3, 4)
    b = np.array([1.5])
    bench.dump_outputs(str(tmp_path / "new" / "dir"), {"a": a, "b": b})
    ra, rb = np.load(tmp_path / "new" / "dir" / "a.npy"), np.load(tmp_path / "new" / "dir" / "b.npy")
    assert ra.dtype == np.float64 and rb.dtype == np.float64
    assert np.array_equal(ra, a) and np.array_equal(rb, b)


def test_dump_stays_within_the_limit_with_a_fixed_sample(tmp_path, monkeypatch):
    bench = _bench()
    assert bench.DUMP_BYTES_MAX == 64 << 20
    monkeypatch.setattr(bench, "DUMP_BYTES_MAX", 1 << 16)             # the rule, at a size a test can afford
    big = np.sin(np.arange(50000, dtype=np.float64))                    # 400 kB: over its share
    small = np.arange(100, dtype=np.float64)                            # under it: written whole
    for d in ("one", "two"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    files = [tmp_path / "one" / f for f in ("big.npy", "small.npy")]
    assert sum(os.path.getsize(f) for f in files) <= 1 << 16
    got = np.load(files[0])
    assert np.array_equal(np.load(files[1]), small)
    assert got.ndim == 1 and 1000 < got.size < big.size
    assert np.all(np.isin(got, big)) and np.unique(got).size > got.size // 2       # elements of the array, not a constant
    assert np.array_equal(got, np.load(tmp_path / "two" / "big.npy"))   # the same elements every time


def test_a_current_library_is_loaded_without_going_through_build(monkeypatch):
    """The benchmark also runs as a user who cannot write into the tree somebody else built: build() opens its lock file for
    writing, so a library that is newer than its sources must be loaded without it; a stale one still goes to build()."""
    bench = _bench()
    import __graft_entry__ as entry
    entry.build()
    calls = []
    monkeypatch.setattr(entry, "build", lambda *a, **k: calls.append(1))
    bench.ensure_built()
    assert not calls
    monkeypatch.setattr(entry, "_stale", lambda target, deps: True)
    bench.ensure_built()
    assert calls == [1]


def _run(extra, out_dir):
    n, d, m = 300, 3, 700          # no multiple of a 128 tile in either direction, more than one tile each
    cmd = [sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--train-n", str(n), "--dim", str(d),
           "--test-points", str(m), "--dump-outputs", str(out_dir)] + extra
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return (n, d, m), lines[0], {k: np.load(os.path.join(out_dir, k + ".npy")) for k in ("mean", "var", "lml")}


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    return _run([], tmp_path_factory.mktemp("plain"))


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_posterior_of_the_seeded_inputs(plain_run):
    from gp_algos_amd import synth
    from oracle import gp_oracle as orc
    (n, d, m), plain, got = plain_run
    assert all(k in plain for k in HEADLINE_KEYS) and not any(k in plain for k in FULL_ONLY_KEYS)
    assert plain["steps"] == 3 and plain["warmup"] == 1 and plain["unit"] == "points/s" and plain["dtype"] == "f64"
    assert plain["higher_is_better"] is True and plain["ms_per_step"] > 0
    assert abs(plain["value"] - m / (plain["ms_per_step"] * 1e-3)) <= 1e-9 * plain["value"]      # points/s of one timed step
    p = synth.config_c2(n, d, m)
    Lo, alpha = orc.fit(p["X"], p["y"], p["theta"])
    omean, ovar, _, _ = orc.predict(p["X"], p["theta"], Lo, alpha, p["Xs"])
    olml = orc.lml(Lo, alpha, p["y"])
    for a in got.values():
        assert a.dtype == np.float64
    assert got["mean"].shape == (m,) and got["var"].shape == (m,) and got["lml"].shape == (1,)
    assert np.max(np.abs(got["mean"] - omean)) <= TOL_MEAN * np.max(np.abs(omean))
    assert np.max(np.abs(got["var"] - ovar)) <= TOL_VAR * p["theta"][0] ** 2
    assert abs(got["lml"][0] - olml) <= TOL_LML * abs(olml)


@pytest.mark.gpu
def test_full_run_adds_to_the_headline_and_dumps_the_same_arrays(plain_run, tmp_path):
    """The same command with --full: the same headline fields plus the rest, and the same arrays bit for bit (same seeded inputs,
    same path; the HIP events that --full records around the launches do not touch the arithmetic)."""
    _, plain, got = plain_run
    _, full, got_full = _run(["--full", "--no-cpu-baseline", "--no-c3"], tmp_path / "full")
    assert all(k in full for k in HEADLINE_KEYS) and all(k in full for k in ("roofline", "cholesky", "gram", "e2e_ms_per_step"))
    assert all(full[k] == plain[k] for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup"))
    for k in got:
        assert np.array_equal(got[k], got_full[k]), k
