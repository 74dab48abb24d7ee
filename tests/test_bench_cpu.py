"""CPU, no device: bench.py's option checks and the --dump-outputs writer (dump_heads) on a stand-in network."""
import os
import subprocess
import sys

import numpy as np

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Heads:
    """Stand-in for netapi.DkNet: three YOLO layers (type 17) among plain layers, batch 2."""
    n = 8
    sizes = {3: 255 * 16 * 16, 5: 255 * 8 * 8, 7: 255 * 4 * 4}

    def info(self, i):
        return {"type": 17 if i in self.sizes else 0, "batch": 2, "outputs": self.sizes.get(i, 1)}

    def output(self, i):
        return np.random.default_rng(i).standard_normal((2, self.sizes[i])).astype(np.float32)


def _dump(d):
    return {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_whole_heads_under_budget(tmp_path):
    bench.dump_heads(_Heads(), str(tmp_path))
    got = _dump(str(tmp_path))
    assert sorted(got) == ["head_3.npy", "head_5.npy", "head_7.npy"]
    for i in (3, 5, 7):
        a = got["head_%d.npy" % i]
        assert a.dtype == np.float32 and np.array_equal(a, _Heads().output(i))


def test_dump_outputs_seeded_sample_over_budget(tmp_path, monkeypatch):
    total = 4 * 2 * sum(_Heads.sizes.values())
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", total // 4)
    bench.dump_heads(_Heads(), str(tmp_path / "a"))
    bench.dump_heads(_Heads(), str(tmp_path / "b"))
    a, b = _dump(str(tmp_path / "a")), _dump(str(tmp_path / "b"))
    assert sum(x.nbytes for x in a.values()) <= total // 4
    for f in a:
        assert a[f].dtype == np.float32 and a[f].ndim == 1 and np.array_equal(a[f], b[f])
        full = _Heads().output(int(f[5:-4])).ravel()
        assert a[f].size == int(full.size * 0.25)
        assert np.isin(a[f], full).all()


def test_bench_rejects_zero_steps():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 2 and b"--steps" in r.stderr
