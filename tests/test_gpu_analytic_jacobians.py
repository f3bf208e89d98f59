"""GPU tests of the closed-form Jacobians (options.jacobians = 1, k_linearize_analytic; -m gpu).  Everything runs with
fix_small_angle_b = 1, which the mode requires.

Where the analytic and the numeric linearisations must disagree: the library's log uses theta = 0 coefficients of W
for residual rotations theta < ~4.5e-3; central differences of that residual differ from the derivatives of the exact
map by ~0.12 theta^2 relative there (tests/test_analytic_jacobians.py).  The H / b comparisons below leave out the
edges in 1e-4 < theta < 5e-3 (and say how many); everywhere else the tolerance is the numeric path's own at
delta = 1e-6 (1e-7 of max |H|)."""
import json
import os

import numpy as np
import pytest

from oracle import oracle as O
from sim3opt_amd import lib as L, synth
import dist_helpers as H
import kitti_graph as K

pytestmark = pytest.mark.gpu
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "oracle_golden.json")))
ANALYTIC = dict(fix_small_angle_b=1, jacobians=1)


def mk(g, info=None, kernel=0, kdelta=0.0, **opts):
    G = L.Graph(**opts)
    G.add_vertices(g["states"], g["fixed"])
    G.add_edges(g["v0"], g["v1"], g["meas"], info=info, kernel=kernel, kernel_delta=kdelta)
    G.initialize()
    return G


def oracle_of(g, info=None, kernel=0, kdelta=0.0):
    inf = None if info is None else np.asarray(info).transpose(0, 2, 1).reshape(-1, 49)
    return O.Graph(g["states"], g["fixed"], g["v0"], g["v1"], g["meas"], info=inf, kernel=kernel, kdelta=kdelta)


def small(seed=0, V=60, E=400, drift=0.05):
    synth.DRIFT_TARGET = drift
    return synth.manhattan(V, E, dims=(4, 4, 3), per_cell=4, seed_graph=300 + seed, seed_noise=400 + seed)


def spd_info(m, seed):
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((m, 7, 7)) * 0.3
    return np.einsum("kij,klj->kil", M, M) + np.eye(7)


def outside_log_band(g):
    """(graph without the edges whose residual rotation lies in log's small-angle band, number left out)"""
    G = mk(g, fix_small_angle_b=1)
    th = np.linalg.norm(G.edge_errors()[:, :3], axis=1)
    G.close()
    keep = (th <= 1e-4) | (th >= 5e-3)
    out = dict(g)
    for k in ("v0", "v1", "meas"):
        out[k] = np.ascontiguousarray(g[k][keep])
    return out, keep, int((~keep).sum())


def test_device_jacobians_equal_host():
    for g, kitti in ((small(1), False), (K.build_direct_graph(False), True)):
        G = mk(g, **ANALYTIC)
        e, J = G.edge_jacobians()
        assert np.abs(e - G.edge_errors()).max() <= 1e-15 * max(1.0, np.abs(e).max())
        worst = 0.0
        for k in range(G.num_edges):
            eh, Jh = L.edge_jacobian_host(g["meas"][k], g["states"][g["v0"][k]], g["states"][g["v1"][k]])
            assert np.abs(e[k] - eh).max() <= 1e-13 * max(1.0, np.abs(eh).max())
            worst = max(worst, np.abs(J[k] - Jh).max() / np.abs(Jh).max())
        assert worst <= 1e-13, worst
        if kitti:  # KITTI-00, 118 loops: the loop residuals reach |e| ~ 111
            assert np.linalg.norm(e, axis=1).max() > 100
        G.close()


@pytest.mark.parametrize("info,kernel", [(False, 0), (True, 0), (False, 1), (True, 1)])
def test_linearisation_matches_numeric_and_oracle(info, kernel):
    g, keep, _ = outside_log_band(small(1))
    inf = spd_info(keep.size, 5)[keep] if info else None
    kd = 0.08 if kernel else 0.0
    Ga = mk(g, info=inf, kernel=kernel, kdelta=kd, **ANALYTIC)
    Gn = mk(g, info=inf, kernel=kernel, kdelta=kd, fix_small_angle_b=1, fd_delta=1e-6)
    Ga.linearize()
    Gn.linearize()
    Ha, ba = Ga.dense_system()
    Hn, bn = Gn.dense_system()
    Ho, bo = oracle_of(g, info=inf, kernel=kernel, kdelta=kd).build_dense(
        O.default_options(fd_delta=1e-6, fix_small_angle_b=1))
    assert np.abs(Ha - Ha.T).max() == 0.0
    for Hr, br in ((Hn, bn), (Ho, bo)):
        assert np.abs(Ha - Hr).max() < 1e-7 * np.abs(Hr).max()
        assert np.abs(ba - br).max() < 1e-7 * max(1.0, np.abs(br).max())


@pytest.mark.parametrize("one,mask", [(True, 127), (False, 127), (False, 0x78)])
def test_kitti_linearisation_matches_oracle(one, mask):
    g, _, _ = outside_log_band(K.build_direct_graph(one))
    G = mk(g, dof_mask=mask, **ANALYTIC)
    G.linearize()
    Ha, ba = G.dense_system()
    Ho, bo = oracle_of(g).build_dense(O.default_options(fd_delta=1e-6, fix_small_angle_b=1, dof_mask=mask))
    assert np.abs(Ha - Ho).max() < 1e-7 * np.abs(Ho).max()
    assert np.abs(ba - bo).max() < 1e-7 * max(1.0, np.abs(bo).max())
    if mask != 127:
        frozen = np.concatenate([[(mask >> d) & 1 == 0 for d in range(7)]] * (Ha.shape[0] // 7))
        assert not Ha[frozen].any() and not ba[frozen].any()


@pytest.mark.parametrize("world", [2, 4])
def test_partitioned_rows_bit_identical(world):
    synth.DRIFT_TARGET = 0.05
    g = synth.manhattan(1500, 12000, dims=(12, 12, 10))
    R = mk(g, device=0, row_order=1, **ANALYTIC)
    R.linearize()
    rp, ci, blocks, b = R.get_system()
    tg = H.ThreadGroup(world)

    def rank_body(rank):
        G = L.Graph(device=0, **ANALYTIC)
        G.add_vertices(g["states"], g["fixed"])
        G.add_edges(g["v0"], g["v1"], g["meas"])
        tg.attach(G, rank)
        G.initialize()
        G.linearize()
        lo, hi = G.local_rows()
        rowptr, colidx, bl, bb = G.get_system()
        out = dict(lo=lo, hi=hi, rowptr=rowptr, colidx=colidx, blocks=bl[rowptr[lo]:rowptr[hi]].copy(),
                   b=bb[7 * lo:7 * hi].copy())
        G.close()
        return out

    res = tg.run(rank_body)
    assert res[0]["lo"] == 0 and res[-1]["hi"] == rp.size - 1
    for r in res:
        lo, hi = r["lo"], r["hi"]
        assert np.array_equal(r["rowptr"], rp) and np.array_equal(r["colidx"], ci)
        assert np.array_equal(r["blocks"], blocks[rp[lo]:rp[hi]])
        assert np.array_equal(r["b"], b[7 * lo:7 * hi])


@pytest.mark.parametrize("name", ["manhattan_120", "chain_150"])
def test_lm_reaches_golden(name):
    gold = GOLD["synthetic_fixb"][name]["fd1e6"]
    synth.DRIFT_TARGET = 0.05
    g = (synth.manhattan(120, 1000, dims=(6, 6, 3), per_cell=4) if name == "manhattan_120"
         else synth.chain_loop(150, 300))
    G = mk(g, pcg_rel_tol=1e-12, **ANALYTIC)
    assert abs(G.chi2() - gold["chi2_0"]) < 1e-9 * gold["chi2_0"]
    n = G.optimize(15)
    st = G.stats()
    assert 3 <= n <= 15
    assert abs(st[-1].chi2_after - gold["chi2_final"]) < 1e-6 * gold["chi2_final"]
    pos = synth.positions(G.get_vertices())
    rm = np.sqrt(((pos - np.array(gold["positions"])) ** 2).sum(1).mean())
    assert rm < 1e-4, rm
    assert np.abs(G.get_vertices()[:, 7] - np.array(gold["scales"])).max() < 1e-4


def test_kitti_one_loop_lm_matches_oracle():
    """As test_kitti_wellposed_arithmetic_pose_parity, in analytic mode against the oracle's central differences
    (delta = 1e-6): one trial per iteration and the trajectory within 1e-4 m RMSE (the north-star bar).  The chi2
    trace: iteration 1 linearises at the loader's estimates, where every odometry residual is zero (outside log's
    small-angle band), and agrees to 1e-6 (measured: 4e-10); from then on the odometry residuals move into the band
    (1e-4 < theta < 5e-3; 641 of 770 after 10 iterations), where the oracle differentiates log's theta = 0
    coefficients and the two Jacobians differ by up to 0.2 theta^2 < 5e-6 relative -- the trace is held to that
    (measured: 2.1e-6 at most, at iteration 6)."""
    g = K.build_direct_graph(True)
    G = mk(g, pcg_rel_tol=1e-13, pcg_max_iters=40000, **ANALYTIC)
    OG = oracle_of(g)
    n = G.optimize(10)
    it, tr = OG.optimize(10, O.default_options(fix_small_angle_b=1, fd_delta=1e-6))
    st = G.stats()
    assert n == it == 10
    assert [s.trials for s in st] == [t.trials for t in tr] == [1] * 10
    rel = [abs(st[k].chi2_after - tr[k].chi2_after) / tr[k].chi2_after for k in range(10)]
    print("chi2 trace, relative gap to the oracle:", " ".join("%.2e" % r for r in rel))
    assert rel[0] < 1e-6, rel
    assert max(rel) < 0.2 * 5e-3 ** 2, rel
    th = np.linalg.norm(G.edge_errors()[1:, :3], axis=1)  # (edge 0 is the loop)
    print("odometry residual rotations after 10 iterations: max %.2e, %d of %d in the band"
          % (th.max(), int(((th > 1e-4) & (th < 5e-3)).sum()), th.size))
    assert synth.rmse(G.get_vertices(), OG.states) < 1e-4
