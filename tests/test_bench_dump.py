"""CPU: bench.py's --dump-outputs writer and its --steps / --warmup check (the GPU side: tests/test_gpu_bench.py)."""
import os
import subprocess
import sys

import numpy as np

from test_bench_launcher import _bench
from conftest import ROOT


def test_dump_writes_float64_arrays(tmp_path):
    b = _bench()
    spec = np.linspace(0.0, 1.0, 1000)
    b.dump_outputs(str(tmp_path / "d"), {"dN_pTdpTdphidy": spec, "ids": np.arange(1000, dtype=np.int64)})
    got = np.load(str(tmp_path / "d" / "dN_pTdpTdphidy.npy"))
    assert got.dtype == np.float64 and np.array_equal(got, spec)
    ids = np.load(str(tmp_path / "d" / "ids.npy"))
    assert ids.dtype == np.float64 and np.array_equal(ids, np.arange(1000))
    assert not os.path.exists(str(tmp_path / "d" / "row_index.npy"))


def test_dump_over_the_limit_writes_the_same_seeded_rows(tmp_path, monkeypatch):
    b = _bench()
    monkeypatch.setattr(b, "DUMP_LIMIT_BYTES", 8000)
    n = 5000
    rows = {"E": np.arange(n) * 0.5, "species": np.arange(n, dtype=np.int32) % 7}
    for d in ("a", "b"):
        b.dump_outputs(str(tmp_path / d), rows)
    for name in ("E", "species", "row_index"):
        a1, a2 = np.load(str(tmp_path / "a" / (name + ".npy"))), np.load(str(tmp_path / "b" / (name + ".npy")))
        assert a1.dtype == np.float64 and np.array_equal(a1, a2), name
    assert sorted(os.listdir(str(tmp_path / "a"))) == ["E.npy", "row_index.npy", "species.npy"]
    total = sum(os.path.getsize(str(tmp_path / "a" / f)) for f in os.listdir(str(tmp_path / "a")))
    idx = np.load(str(tmp_path / "a" / "row_index.npy")).astype(np.int64)
    assert total <= 8000 and len(idx) > 0 and np.all(np.diff(idx) > 0)
    assert np.array_equal(np.load(str(tmp_path / "a" / "E.npy")), rows["E"][idx])


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--steps" in r.stderr and not r.stdout.strip()
