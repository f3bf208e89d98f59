"""Writes tests/golden/single_process_ranks_huber_oracle.npz: the CPU oracle's four LM iterations (exact LDL^T) on the
1500-vertex Manhattan graph with dense information matrices and Huber kernels (delta = 0.5) -- the set-up of
test_distributed_gpu.test_partitioned_multigrid_with_information_and_huber_matches_oracle, which runs the oracle live
(a minute of CPU time); tests/test_gpu_single_process_ranks.py reads this record of it instead.
    python tests/golden/make_single_process_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import oracle as O  # noqa: E402
from sim3opt_amd import synth  # noqa: E402


def inputs():
    synth.DRIFT_TARGET = 0.05
    g = synth.manhattan(1500, 15000, dims=(12, 12, 10))
    rng = np.random.default_rng(21)
    M = rng.standard_normal((len(g["v0"]), 7, 7)) * 0.3
    return g, np.einsum("kij,klj->kil", M, M) + np.eye(7)


def fingerprint(g, inf):
    return np.array([g["states"].sum(), g["meas"].sum(), inf.sum()])


if __name__ == "__main__":
    g, inf = inputs()
    OG = O.Graph(g["states"], g["fixed"], g["v0"], g["v1"], g["meas"],
                 info=inf.transpose(0, 2, 1).reshape(-1, 49), kernel=1, kdelta=0.5)
    it, tr = OG.optimize(4, O.default_options(fix_small_angle_b=1, fd_delta=1e-6, threads=8))
    np.savez_compressed(os.path.join(HERE, "single_process_ranks_huber_oracle.npz"), states=OG.states,
                        trials=np.array([t.trials for t in tr], dtype=np.int32),
                        chi2_after=np.array([t.chi2_after for t in tr]), iterations=np.int32(it),
                        inputs_sum=fingerprint(g, inf))
