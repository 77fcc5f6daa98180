"""bench.py's command line: the plain run, --full and --dump-outputs.

The CPU tests check the dump format (sample size, determinism, exact values);
the ``gpu`` test runs a tiny plain benchmark in a child process and checks its
result line and that the dumped rows are the oracle's fwd_mul of the seeded
inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench
import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P27, P62 = bench.P27, bench.P62


def _load_dump(d, name, q):
    if q <= (1 << 53):
        a = np.load(os.path.join(d, f"{name}.npy"))
        assert a.dtype == np.float64
        return a.astype(np.uint64)
    lo, hi = np.load(os.path.join(d, f"{name}_lo32.npy")), np.load(os.path.join(d, f"{name}_hi32.npy"))
    assert lo.dtype == np.float64 and hi.dtype == np.float64
    return (hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)


def test_dump_sample_is_fixed_and_within_64_mb():
    for q, parts in ((P27, 1), (P62, 2)):
        rows = bench.dump_sample(65536, 16384, q)  # the default workload
        assert (rows == bench.dump_sample(65536, 16384, q)).all()
        assert len(set(rows.tolist())) == len(rows) > 64 and rows.min() >= 0 and rows.max() < 65536
        assert (np.diff(rows) > 0).all()
        assert parts * len(rows) * 16384 * 8 + 2 * 128 <= 64e6
    # a small output is written whole
    assert (bench.dump_sample(5, 64, P27) == np.arange(5)).all()


@pytest.mark.parametrize("q", [P27, P62])
def test_dump_rows_values_are_exact(tmp_path, q):
    x = oracle.splitmix_fill(9, q, 7 * 64).reshape(7, 64).copy()
    x[0, 0], x[6, 63] = q - 1, 0
    bench.dump_rows(str(tmp_path), "fwd_mul", torch.from_numpy(x.view(np.int64)), q)
    assert (_load_dump(str(tmp_path), "fwd_mul", q) == x).all()
    assert len(os.listdir(tmp_path)) == (1 if q == P27 else 2)


def test_parse_plain_and_full(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()


@pytest.mark.gpu
@pytest.mark.parametrize("q", [P27, P62])
def test_plain_run_line_and_dump_vs_oracle(tmp_path, q):
    """A plain run times --steps steps of C3 and nothing else; the dump is
    the fwd_mul of the seeded inputs, bit-exact vs the oracle."""
    n, batch, steps = 1024, 96, 2
    d = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "1", "--n", str(n), "--batch", str(batch), "--q", str(q), "--dump-outputs", d],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["warmup"] == 1 and line["full"] is False
    assert line["unit"] == "NTTs/s" and line["higher_is_better"] is True and line["ms_per_step"] > 0
    assert abs(line["value"] - batch / (line["ms_per_step"] * 1e-3)) <= 1e-9 * line["value"]
    for side in ("cpu_baseline", "polymuls_per_s", "q62", "negacyclic", "cipher", "host_resident", "engine_chain"):
        assert side not in line, side
    # the inputs bench.py generates (rank 0), regenerated here
    g = torch.Generator(device="cuda").manual_seed(1234)
    a = torch.randint(0, q, (batch, n), device="cuda", dtype=torch.int64, generator=g).cpu().numpy().view(np.uint64)
    b = torch.randint(0, q, (batch, n), device="cuda", dtype=torch.int64, generator=g).cpu().numpy().view(np.uint64)
    got = _load_dump(d, "fwd_mul", q)
    assert got.shape == (batch, n)
    assert (got == oracle.NTT(n, q).fwd_mul(a, b)).all()
