"""bench.py --dump-outputs (no GPU): what the last timed step returned, float64, within the 64 MB cap,
and the same rows from run to run when only a sample fits."""
import os
import sys
import types

import numpy as np
import pytest

import bench


class FakeGraph:
    def __init__(self, n):
        self.states = np.random.default_rng(n).standard_normal((n, 8))

    def get_vertices(self):
        return self.states.copy()


LAST = types.SimpleNamespace(chi2_before=2.5, chi2_after=1.5, lambda_=1e-3)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_writes_every_estimate_and_the_last_step(tmp_path):
    G = FakeGraph(1000)
    bench.dump_outputs(str(tmp_path / "out"), G, [types.SimpleNamespace(chi2_before=9.0, chi2_after=8.0,
                                                                        lambda_=1.0), LAST])
    out = _load(tmp_path / "out")
    assert sorted(out) == ["lm_last_step", "vertices"]
    assert all(a.dtype == np.float64 for a in out.values())
    assert np.array_equal(out["vertices"], G.states)
    assert out["lm_last_step"].tolist() == [2.5, 1.5, 1e-3]


def test_dump_above_the_cap_is_a_fixed_sample(tmp_path):
    G = FakeGraph(1_200_000)  # 76.8 MB of estimates
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), G, [LAST])
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 64_000_000
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == ["lm_last_step", "vertices_sample", "vertices_sample_rows"]
    assert all(np.array_equal(a[k], b[k]) for k in a)
    rows = a["vertices_sample_rows"].astype(np.int64)
    assert np.all(np.diff(rows) > 0) and rows[-1] < len(G.states)
    assert np.array_equal(a["vertices_sample"], G.states[rows])


def test_steps_sets_the_timed_steps(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "5", "--dump-outputs", "d"])
    args = bench.parse()
    assert args.steps == 5 and args.dump_outputs == "d"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()


def test_full_is_opt_in(monkeypatch):
    # a plain run does only what the headline needs; the legs of their own run behind --full
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"])
    args = bench.parse()
    assert not args.full and (args.steps, args.warmup) == (20, 5)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full"])
    assert bench.parse().full
