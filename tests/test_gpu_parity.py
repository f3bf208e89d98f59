"""GPU parity tests (-m gpu): every call goes through the C-ABI of libsim3opt.so and is compared
with the CPU oracle on the same seeded inputs, with the committed golden vectors, and -- at
BASELINE.json's full sizes, where the oracle's exact Cholesky is impractical -- through
size-independent properties.

Tolerances (FP64 throughout):
  residuals e ............... 1e-11 absolute (same formulae, different libm)
  J^T J, J^T e, delta=1e-9 .. 2e-4 relative: central differences with g2o's step carry ~1e-7/|e|
                              noise per entry (see DESIGN.md "finite-difference noise")
  same with delta=1e-6 ...... 1e-7 relative
  PCG solution .............. 1e-6 relative vs dense LU of the same matrix
  LM, well-posed graphs ..... trajectory RMSE < 1e-4 (north_star), final chi2 1e-6 relative
"""
import json
import os

import numpy as np
import pytest

from oracle import oracle as O
from sim3opt_amd import lib as L, sim3np as S3, synth
import kitti_graph as K

pytestmark = pytest.mark.gpu
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "oracle_golden.json")))


def mk(g, info=None, kernel=0, kdelta=0.0, ids=None, **opts):
    G = L.Graph(**opts)
    G.add_vertices(g["states"], g["fixed"], ids)
    v0, v1 = g["v0"], g["v1"]
    if ids is not None:
        v0, v1 = np.asarray(ids)[v0], np.asarray(ids)[v1]
    G.add_edges(v0, v1, g["meas"], info=info, kernel=kernel, kernel_delta=kdelta)
    G.initialize()
    return G


def oracle_of(g, info=None, kernel=0, kdelta=0.0):
    inf = None if info is None else np.asarray(info).transpose(0, 2, 1).reshape(-1, 49)
    return O.Graph(g["states"], g["fixed"], g["v0"], g["v1"], g["meas"], info=inf, kernel=kernel,
                   kdelta=kdelta)


def small(seed=0, V=60, E=400, drift=0.05):
    synth.DRIFT_TARGET = drift
    return synth.manhattan(V, E, dims=(4, 4, 3), per_cell=4, seed_graph=300 + seed,
                           seed_noise=400 + seed)


def spd_info(m, seed):
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((m, 7, 7)) * 0.3
    return np.einsum("kij,klj->kil", M, M) + np.eye(7)


# ------------------------------------------------------------------ residuals / chi2
@pytest.mark.parametrize("one", [True, False])
def test_kitti_residuals_and_chi2(one):
    g = K.build_direct_graph(one)
    G, OG = mk(g), oracle_of(g)
    e = G.edge_errors()
    assert np.abs(e - OG.errors()).max() < 1e-11
    gold = GOLD["kitti"]["one_loop" if one else "all_loops"]
    assert np.abs(e[gold["edge_sel"]] - np.array(gold["e_sel"])).max() < 1e-11
    assert abs(G.chi2() - gold["chi2_0"]) < 1e-10 * gold["chi2_0"]
    assert abs(e[0, 6] - np.log(5.32393351)) < 1e-12
    assert np.abs(e[(1 if one else 118):]).max() < 1e-11  # odometry edges: zero by construction


def test_cxx_loader_feeds_same_graph():
    G = L.Graph()
    G.load_kitti_direct(K.FIXTURE, False)
    G.initialize()
    assert abs(G.chi2() - GOLD["kitti"]["all_loops"]["chi2_0"]) < 1e-6


@pytest.mark.parametrize("fixb", [0, 1])
def test_residuals_all_branches(fixb):
    """Edges whose error lands on each exp/log branch, incl. the as-written small-angle B."""
    xi = np.array(GOLD["explog"]["xi"])
    m = xi.shape[0]
    rng = np.random.default_rng(11)
    S0 = S3.exp(np.concatenate([rng.standard_normal((m, 3)), rng.standard_normal((m, 3)) * 3,
                                rng.uniform(-0.3, 0.3, (m, 1))], axis=1))
    Cm = S3.exp(np.concatenate([rng.standard_normal((m, 3)) * 0.5, rng.standard_normal((m, 3)),
                                rng.uniform(-0.2, 0.2, (m, 1))], axis=1))
    S1 = S3.mul(S3.inv(S3.exp(xi)), S3.mul(Cm, S0))  # e = log(C S0 S1^-1) = xi
    states = np.concatenate([S0, S1])
    g = dict(states=states, fixed=np.zeros(2 * m, np.uint8), v0=np.arange(m, dtype=np.int32),
             v1=np.arange(m, 2 * m, dtype=np.int32), meas=Cm)
    g["fixed"][0] = 1
    G = mk(g, fix_small_angle_b=fixb)
    e = G.edge_errors()
    eo = oracle_of(g).errors(O.default_options(fix_small_angle_b=fixb))
    # Near the 1e-5 thresholds the reference formulae cancel catastrophically ((s-1)/sigma,
    # ((sigma-1)s+1)/sigma^2, the 1/theta^2 of B) and, as written, B ~ 1/sigma^3 makes W
    # ill-conditioned (cond up to 1e10 in this table): last-bit libm differences between device and
    # host are amplified to ~1e-6.  Away from the thresholds agreement is at rounding level.
    err = np.abs(e - eo) / (1 + np.abs(eo))
    assert err.max() < 1e-5
    generic = (np.abs(xi[:, 6]) >= 1e-3) & (np.linalg.norm(xi[:, :3], axis=1) >= 0.3)
    assert generic.sum() >= 6 and err[generic].max() < 1e-12


# ------------------------------------------------------------------ linearisation
@pytest.mark.parametrize("info,kernel", [(False, 0), (True, 0), (False, 1), (True, 1)])
@pytest.mark.parametrize("delta,tol", [(1e-9, 2e-4), (1e-6, 1e-7)])
def test_linearisation_matches_oracle(info, kernel, delta, tol):
    g = small(1)
    inf = spd_info(g["v0"].shape[0], 5) if info else None
    kd = 0.08 if kernel else 0.0
    G = mk(g, info=inf, kernel=kernel, kdelta=kd, fd_delta=delta)
    OG = oracle_of(g, info=inf, kernel=kernel, kdelta=kd)
    o = O.default_options(fd_delta=delta)
    assert abs(G.chi2() - OG.chi2(o)) < 1e-10 * OG.chi2(o)
    G.linearize()
    H, b = G.dense_system()
    Ho, bo = OG.build_dense(o)
    assert np.abs(H - H.T).max() == 0.0  # both triangles come from one Gram matrix
    assert np.abs(H - Ho).max() < tol * np.abs(Ho).max()
    assert np.abs(b - bo).max() < tol * max(1.0, np.abs(bo).max())


def test_kitti_linearisation_and_block_structure():
    g = K.build_direct_graph(False)
    G, OG = mk(g, fd_delta=1e-6), oracle_of(g)
    G.linearize()
    rowptr, colidx, blocks, b = G.get_system()
    nb, nnzb = G.system_dims()
    assert nb == 770 and nnzb == 770 + 2 * 887  # only edge (1,0) touches the fixed vertex
    assert np.all(colidx[rowptr[:-1]] == np.arange(nb))  # diagonal block first in every row
    H, b = G.dense_system()
    Ho, bo = OG.build_dense(O.default_options(fd_delta=1e-6))
    assert np.abs(H - Ho).max() < 1e-7 * np.abs(Ho).max()
    assert np.abs(b - bo).max() < 1e-7 * np.abs(bo).max()


def test_ids_fixed_vertices_and_parallel_edges():
    g = small(2)
    g["fixed"][[0, 7, 31]] = 1
    # an edge between two fixed vertices (counts in chi2 only) and a duplicated edge
    g["v0"] = np.concatenate([g["v0"], [7, g["v0"][3]]]).astype(np.int32)
    g["v1"] = np.concatenate([g["v1"], [31, g["v1"][3]]]).astype(np.int32)
    g["meas"] = np.concatenate([g["meas"], g["meas"][:1], g["meas"][3:4]])
    ids = (np.arange(g["states"].shape[0]) * 13 - 100).astype(np.int32)  # arbitrary, incl. negative
    G = mk(g, ids=ids, fd_delta=1e-6)
    OG = oracle_of(g)
    o = O.default_options(fd_delta=1e-6)
    assert abs(G.chi2() - OG.chi2(o)) < 1e-10 * OG.chi2(o)
    G.linearize()
    H, b = G.dense_system()
    Ho, bo = OG.build_dense(o)
    assert H.shape == Ho.shape
    assert np.abs(H - Ho).max() < 1e-7 * np.abs(Ho).max()
    assert np.abs(b - bo).max() < 1e-7 * np.abs(bo).max()
    assert np.array_equal(G.get_vertex(int(ids[5])), g["states"][5])


# ------------------------------------------------------------------ linear solve
def test_pcg_matches_dense_and_oracle_ldlt():
    g = small(3, V=120, E=900)
    G, OG = mk(g, fd_delta=1e-6, pcg_rel_tol=1e-12, linear_solver=0), oracle_of(g)
    G.linearize()
    H, b = G.dense_system()
    lam = 1e-5 * np.abs(np.diag(H)).max()
    x, it, rr = G.solve(lam)
    assert rr <= 1e-12 and 0 < it <= 7 * 119
    xd = np.linalg.solve(H + lam * np.eye(H.shape[0]), b)
    assert np.abs(x - xd).max() < 1e-6 * np.abs(xd).max()
    ok, xo, _ = OG.solve_once(lam, O.default_options(fd_delta=1e-6))
    assert ok and np.abs(x - xo).max() < 1e-5 * np.abs(xo).max()
    # independent residual check of the reported convergence
    r = b - (H @ x + lam * x)
    assert np.linalg.norm(r) < 1e-9 * np.linalg.norm(b)


def test_chain_segment_preconditioner_on_kitti():
    """Block-tridiagonal chain segments (option `preconditioner`): same solution as block-Jacobi,
    an order of magnitude fewer PCG iterations on the one-loop KITTI chain (the automatic rule now
    prefers the multigrid hierarchy there)."""
    g = K.build_direct_graph(True)
    sol = {}
    for pre in (0, 1, -1):
        G = mk(g, fix_small_angle_b=1, fd_delta=1e-6, pcg_rel_tol=1e-12, pcg_max_iters=40000,
               preconditioner=pre, linear_solver=0)  # (automatic solver choice here: the exact one)
        G.linearize()
        H, b = G.dense_system()
        lam = 1e-5 * np.abs(np.diag(H)).max()
        x, it, rr = G.solve(lam)
        xd = np.linalg.solve(H + lam * np.eye(H.shape[0]), b)
        assert np.abs(x - xd).max() < 1e-7 * np.abs(xd).max()
        sol[pre] = it
        assert G.preconditioner_in_use() == (2 if pre < 0 else pre)
    # chain segments: an order of magnitude fewer iterations; so does the automatic choice on this
    # 770-row graph, the two-level multigrid (770 -> 96 rows, dense) -- with parallel kernels where
    # the chain apply is a sequential sweep (100 LM iterations: 0.7 s against 2.7 s)
    assert sol[1] * 10 < sol[0] and sol[-1] * 10 < sol[0]
    # with all 118 loops the chain argument is gone, the hierarchy is not
    g = K.build_direct_graph(False)
    its = {}
    for pre in (0, -1):
        G = mk(g, fix_small_angle_b=1, fd_delta=1e-6, pcg_rel_tol=1e-10, preconditioner=pre,
               pcg_max_iters=40000, linear_solver=0)
        G.linearize()
        its[pre] = G.solve(1.0)[1]
    assert its[-1] < its[0]  # (over a whole LM run: 15 404 against 781 311 iterations)
    # LM through the chain preconditioner reaches the oracle's answer
    g = K.build_direct_graph(True)
    G = mk(g, fix_small_angle_b=1, fd_delta=1e-6, pcg_rel_tol=1e-13, preconditioner=1,
           pcg_max_iters=40000)
    OG = oracle_of(g)
    G.optimize(10)
    OG.optimize(10, O.default_options(fix_small_angle_b=1, fd_delta=1e-6))
    assert synth.rmse(G.get_vertices(), OG.states) < 1e-4


def _true_relres(G, x, lam):
    import scipy.sparse as sp
    rowptr, colidx, blocks, b = G.get_system()
    A = sp.bsr_matrix((blocks, colidx, rowptr), shape=(b.size, b.size))
    return np.linalg.norm(b - (A @ x + lam * x)) / np.linalg.norm(b)


def test_multigrid_preconditioner_solution_and_iterations(monkeypatch):
    """Aggregation multigrid (`preconditioner = 2`, amg.cpp / amg_kernels.hpp): the PCG solution
    agrees with the dense solve and with block-Jacobi PCG; on a loop-rich Manhattan graph it needs
    several times fewer iterations; V-, W- and additive-level-0 cycles are all valid preconditioners; the
    automatic rule picks it exactly for graphs that coarsen well."""
    synth.DRIFT_TARGET = 0.05
    g = synth.manhattan(400, 4000, dims=(6, 6, 10))
    G = mk(g, fix_small_angle_b=1, fd_delta=1e-6, pcg_rel_tol=1e-12, preconditioner=2)
    rows, blocks, _ = G.amg_hierarchy()
    assert len(rows) >= 2 and rows[-1] <= 256
    assert G.preconditioner_in_use() == 2
    # automatic rule: this graph coarsens well -> multigrid; <= 256 rows -> no hierarchy; config 2
    # (random long-range loops: an expander, level-1 blocks 0.47 of level 0) -> block-Jacobi
    assert mk(g, fix_small_angle_b=1).preconditioner_in_use() == 2
    assert mk(small(3, V=120, E=900), fix_small_angle_b=1, linear_solver=0).preconditioner_in_use() == 0
    assert mk(synth.chain_loop(3000, 6000), fix_small_angle_b=1).preconditioner_in_use() == 0
    assert mk(g).preconditioner_in_use() == 2  # the same rule in the reference's as-written arithmetic (round 3)
    G.linearize()
    H, b = G.dense_system()
    for lam_rel in (1e-3, 1e-7):
        lam = lam_rel * np.abs(np.diag(H)).max()
        x, it, rr = G.solve(lam)
        xd = np.linalg.solve(H + lam * np.eye(H.shape[0]), b)
        assert rr <= 1e-12 and np.abs(x - xd).max() < 1e-7 * np.abs(xd).max()
    g = synth.manhattan(3000, 30000, dims=(17, 17, 10))
    res = {}
    for tag, pre, env in (("bj", 0, {}), ("auto", -1, {}), ("default", 2, {}),
                          ("w", 2, {"SIM3OPT_AMG_ADDITIVE": "0", "SIM3OPT_AMG_CYCLE": "2"}),
                          ("v", 2, {"SIM3OPT_AMG_ADDITIVE": "0", "SIM3OPT_AMG_CYCLE": "1"}),
                          ("add", 2, {"SIM3OPT_AMG_ADDITIVE": "1", "SIM3OPT_AMG_CYCLE": "122"})):
        for k in ("SIM3OPT_AMG_CYCLE", "SIM3OPT_AMG_ADDITIVE"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        G = mk(g, fix_small_angle_b=1, pcg_rel_tol=1e-10, pcg_max_iters=20000, preconditioner=pre)
        G.linearize()
        for lam in (10.0, 1e-2):
            x, it, rr = G.solve(lam)
            assert rr <= 1e-10 and _true_relres(G, x, lam) < 1e-8
            res[(tag, lam)] = (x, it)
    for lam in (10.0, 1e-2):
        xb, itb = res[("bj", lam)]
        # >= 2000 loop-rich rows: the automatic choice is the hierarchy -- except that a damping-dominated
        # solve (lambda of the order of the diagonal of H: here 10) starts with block-Jacobi, which
        # finishes it (round 3, Engine::adaptive_prec)
        assert res[("auto", lam)][1] == res[("default" if lam < 1 else "bj", lam)][1]
        for tag in ("default", "w", "v", "add"):
            x, it = res[(tag, lam)]
            assert np.abs(x - xb).max() < 1e-6 * np.abs(xb).max()
        assert res[("w", lam)][1] <= res[("v", lam)][1] <= itb
        if lam < 1:  # light damping: block-Jacobi sees only neighbours, the hierarchy the whole map
            assert res[("w", lam)][1] * 3 < itb and res[("v", lam)][1] * 2 < itb
            assert res[("default", lam)][1] * 2 < itb and res[("add", lam)][1] * 2 < itb


def test_multigrid_lm_matches_oracle():
    """LM driven through the multigrid-preconditioned PCG reaches the oracle's (exact LDL^T) poses;
    two runs are bit-identical (fixed-order Galerkin products, no atomics)."""
    synth.DRIFT_TARGET = 0.05
    g = synth.manhattan(400, 4000, dims=(6, 6, 10))
    OG = oracle_of(g)
    OG.optimize(8, O.default_options(fix_small_angle_b=1, fd_delta=1e-6))
    out = []
    for rep in range(2):
        G = mk(g, fix_small_angle_b=1, fd_delta=1e-6, pcg_rel_tol=1e-12, preconditioner=2)
        assert G.optimize(8) == 8
        out.append(G.get_vertices())
        assert all(s.pcg_rel_res <= 1e-12 for s in G.stats())
    assert synth.rmse(out[0], OG.states) < 1e-4
    assert np.array_equal(out[0], out[1])
    # a graph that does not coarsen (star) silently keeps block-Jacobi
    n = 300
    S = L.Graph(fix_small_angle_b=1, preconditioner=2)
    st = S3.identity(n)
    st[:, 4] = np.arange(n) * 0.1
    S.add_vertices(st, [1] + [0] * (n - 1))
    S.add_edges(np.full(n - 1, 0), np.arange(1, n), np.tile(S3.identity(), (n - 1, 1)))
    S.add_edges(np.full(n - 2, 1), np.arange(2, n), np.tile(S3.identity(), (n - 2, 1)))
    S.initialize()
    assert S.optimize(3) >= 1


def test_pcg_reports_breakdown_on_indefinite_system():
    g = small(3)
    G = mk(g, linear_solver=0)
    G.linearize()
    with pytest.raises(L.Sim3OptError):
        G.solve(-1e12)
    # through the multigrid path: its set-up meets non-positive pivots, the solve falls back to
    # block-Jacobi, which reports the breakdown; the next (definite) solve is unaffected
    synth.DRIFT_TARGET = 0.05
    g = synth.manhattan(400, 4000, dims=(6, 6, 10))
    G = mk(g, fix_small_angle_b=1, pcg_rel_tol=1e-10)
    assert G.preconditioner_in_use() == 2
    G.linearize()
    x0, it0, _ = G.solve(1.0)
    with pytest.raises(L.Sim3OptError):
        G.solve(-1e12)
    x1, it1, rr = G.solve(1.0)
    assert it1 == it0 and rr <= 1e-10 and np.array_equal(x0, x1)


# ------------------------------------------------------------------ Levenberg-Marquardt
def test_kitti_wellposed_arithmetic_pose_parity():
    """KITTI-00 direct PGO (config 1) with the exact small-angle B coefficient and delta = 1e-6:
    here LM behaves (chi2 169.93 -> 13.63 -> 0.373 -> ...; the vertex scales grow to 5.27, the loop's
    scale ratio 5.32) and the run is reproducible, so the north_star tolerance applies:
    trajectory RMSE vs the oracle < 1e-4, chi2 trace to 1e-6."""
    g = K.build_direct_graph(True)
    G = mk(g, fix_small_angle_b=1, fd_delta=1e-6, pcg_rel_tol=1e-13, pcg_max_iters=40000)
    OG = oracle_of(g)
    n = G.optimize(10)
    it, tr = OG.optimize(10, O.default_options(fix_small_angle_b=1, fd_delta=1e-6))
    st = G.stats()
    assert n == it == 10
    for k in range(10):
        assert st[k].trials == tr[k].trials == 1
        assert abs(st[k].chi2_after - tr[k].chi2_after) < 1e-6 * tr[k].chi2_after
    assert abs(st[0].chi2_after - 13.63306) < 1e-4
    assert synth.rmse(G.get_vertices(), OG.states) < 1e-4
    assert abs(G.get_vertices()[:, 7].max() - OG.states[:, 7].max()) < 1e-5


def test_kitti_all_loops_evaluation_vs_ground_truth():
    """Config 1 with all 118 loops + the evaluation harness (kitti_surf.cpp:1427-1463): RMSE of
    the optimised keyframe trajectory against KITTI-00 ground truth after Umeyama alignment.
    Un-optimised VO map: 130.2 m.  Oracle, 100 iterations: exact-B arithmetic 15.5 m, the
    reference's as-written arithmetic 116.6 m.  Here 25 iterations (~90 m, convergence is slow)
    and GPU vs oracle through the same harness."""
    gt = np.loadtxt(os.path.join(K.FIXTURE, "gt_kf.txt"), comments="%")[:, [4, 8, 12]]
    g = K.build_direct_graph(False)
    G = mk(g, fix_small_angle_b=1, fd_delta=1e-6, pcg_rel_tol=1e-12, pcg_max_iters=40000)
    OG = oracle_of(g)
    n = G.optimize(25)
    OG.optimize(25, O.default_options(fix_small_angle_b=1, fd_delta=1e-6))
    _, rm_gpu, _ = L.align_trajectory(synth.positions(G.get_vertices()), gt)
    _, rm_cpu, _ = L.align_trajectory(synth.positions(OG.states), gt)
    assert n == 25
    assert rm_gpu < 130.0 and abs(rm_gpu - rm_cpu) < 0.02 * rm_cpu
    assert synth.rmse(G.get_vertices(), OG.states) < 5e-2  # flat valley: chi2 agrees far tighter
    assert abs(G.stats()[-1].chi2_after - OG.chi2(O.default_options(fix_small_angle_b=1))) \
        < 1e-4 * G.stats()[-1].chi2_after


def test_stepwise_pipeline_kitti():
    """testStepwiseSim3Optimization (kitti_surf.cpp:713-1086): scales by the null vector (stage 1,
    host), scale+translation LM with rotations frozen (stage 2, dof_mask 0x78), Sim3 LM warm-started
    from it (stage 3).  vio_g2o's G2oEdgeScaleTrans is unavailable; stage 2 uses the (upsilon, sigma)
    rows of the Sim3 residual.  In the reference's as-written arithmetic this is what
    rescues the result: RMSE vs KITTI ground truth 13.5 m, against 116.6 m for the direct run."""
    gt = np.loadtxt(os.path.join(K.FIXTURE, "gt_kf.txt"), comments="%")[:, [4, 8, 12]]
    g = K.build_direct_graph(False)
    # stage 1 against an independent dense SVD (what the reference calls)
    A = np.zeros((g["v0"].shape[0], 771))
    for k, (a, b) in enumerate(zip(g["v0"], g["v1"])):
        A[k, a] = g["meas"][k, 7]
        A[k, b] = -1
    v = np.linalg.svd(A, full_matrices=False)[2][-1]
    v = v / v[0]
    G = L.Graph(pcg_rel_tol=1e-12, pcg_max_iters=40000)  # reference arithmetic (as written)
    G.add_vertices(g["states"], g["fixed"])
    G.add_edges(g["v0"], g["v1"], g["meas"])
    G.stepwise_scale_init()
    assert np.abs(G.get_vertices()[:, 7] - v).max() < 1e-8
    assert np.array_equal(G.get_vertices()[:, :7], g["states"][:, :7])
    st0 = g["states"].copy()
    st0[:, 7] = v
    OG = O.Graph(st0, g["fixed"], g["v0"], g["v1"], g["meas"])
    # stage 2: rotations frozen
    G.set_options(dof_mask=0x78)
    G.initialize()
    q_before = G.get_vertices()[:, :4].copy()
    n2 = G.optimize(12)
    it2, tr2 = OG.optimize(12, O.default_options(dof_mask=0x78))
    assert n2 == it2 == 12
    assert np.array_equal(G.get_vertices()[:, :4], q_before)  # no rotation moved
    st = G.stats()
    for k in range(6):
        assert abs(st[k].chi2_after - tr2[k].chi2_after) < 1e-4 * tr2[k].chi2_after
    assert st[-1].chi2_after < 1e-3 * st[0].chi2_before
    # stage 3: full Sim3, warm start (kitti_surf.cpp:1028-1047)
    G.set_options(dof_mask=127)
    n3 = G.optimize(5)
    it3, tr3 = OG.optimize(5, O.default_options())
    assert n3 == it3 == 5
    _, rm_gpu, _ = L.align_trajectory(synth.positions(G.get_vertices()), gt)
    _, rm_cpu, _ = L.align_trajectory(synth.positions(OG.states), gt)
    # after only 12 + 5 iterations the pipeline is part-way (100 + 100: 13.5 m; direct: ~117 m)
    assert rm_gpu < 100.0 and abs(rm_gpu - rm_cpu) < 0.05 * rm_cpu


def test_incremental_loop_closures_warm_start():
    """BASELINE.json config 5 (b): loop closures added one at a time, LM warm-started from the
    previous solution after each (g2o: addEdge + initializeOptimization + optimize again)."""
    full = K.build_direct_graph(False)
    nl = 118
    odo = dict(full, v0=full["v0"][nl:], v1=full["v1"][nl:], meas=full["meas"][nl:])
    G = L.Graph(fix_small_angle_b=1, fd_delta=1e-6, pcg_rel_tol=1e-13, pcg_max_iters=40000)
    G.add_vertices(odo["states"], odo["fixed"])
    G.add_edges(odo["v0"], odo["v1"], odo["meas"])
    G.initialize()
    assert G.chi2() < 1e-18
    states = full["states"].copy()
    o = O.default_options(fix_small_angle_b=1, fd_delta=1e-6)
    for k in range(3):
        G.add_edge(int(full["v0"][k]), int(full["v1"][k]), full["meas"][k])
        with pytest.raises(L.Sim3OptError):  # graph changed: must re-initialize first
            G.chi2()
        G.initialize()
        n = G.optimize(6)
        v0 = np.concatenate([full["v0"][:k + 1], odo["v0"]])
        v1 = np.concatenate([full["v1"][:k + 1], odo["v1"]])
        meas = np.concatenate([full["meas"][:k + 1], odo["meas"]])
        OG = O.Graph(states, full["fixed"], v0, v1, meas)
        it, tr = OG.optimize(6, o)
        states = OG.states.copy()
        assert n == it == 6
        assert abs(G.stats()[-1].chi2_after - tr[-1].chi2_after) < 1e-5 * max(tr[-1].chi2_after, 1e-3)
        assert synth.rmse(G.get_vertices(), states) < 1e-4
    assert G.num_edges == 770 + 3


@pytest.mark.parametrize("name", ["manhattan_120", "chain_150"])
@pytest.mark.parametrize("tag,fd,tol", [("fd1e6", 1e-6, 1e-4), ("fd1e9", 1e-9, 1e-3)])
def test_lm_wellposed_pose_parity(name, tag, fd, tol):
    """Well-posed graphs (exact small-angle B): GPU and oracle converge to the same optimum.
    With a finite-difference step of 1e-6 the Jacobian noise is ~1e-10 and the trajectories must
    agree to < 1e-4 RMSE (north_star tolerance; measured ~1e-7).  With g2o's 1e-9 the oracle's own
    answer moves by 1.1e-4 (chain_150) between the two steps, so only 1e-3 is asserted there."""
    gold = GOLD["synthetic_fixb"][name][tag]
    synth.DRIFT_TARGET = 0.05
    g = (synth.manhattan(120, 1000, dims=(6, 6, 3), per_cell=4) if name == "manhattan_120"
         else synth.chain_loop(150, 300))
    G = mk(g, fix_small_angle_b=1, pcg_rel_tol=1e-12, fd_delta=fd)
    assert abs(G.chi2() - gold["chi2_0"]) < 1e-9 * gold["chi2_0"]
    n = G.optimize(15)
    st = G.stats()
    assert 3 <= n <= 15  # after convergence LM may Terminate on 10 rejected trials (g2o rule)
    assert abs(st[-1].chi2_after - gold["chi2_final"]) < 1e-6 * gold["chi2_final"]
    pos = synth.positions(G.get_vertices())
    rm = np.sqrt(((pos - np.array(gold["positions"])) ** 2).sum(1).mean())
    assert rm < tol, rm
    assert np.abs(G.get_vertices()[:, 7] - np.array(gold["scales"])).max() < tol
    assert abs(G.chi2() - st[-1].chi2_after) < 1e-9 * st[-1].chi2_after


def test_lm_policy_trace_matches_oracle_wellposed():
    g = small(4, V=100, E=700)
    G, OG = mk(g, fix_small_angle_b=1, pcg_rel_tol=1e-12, fd_delta=1e-6), oracle_of(g)
    G.optimize(6)
    _, tr = OG.optimize(6, O.default_options(fix_small_angle_b=1, fd_delta=1e-6))
    st = G.stats()
    for k in range(3):  # before the finite-difference noise floor
        assert st[k].trials == tr[k].trials
        assert abs(st[k].chi2_after - tr[k].chi2_after) < 1e-5 * tr[k].chi2_after
        assert abs(st[k].lambda_ - tr[k].lambda_) < 1e-3 * tr[k].lambda_
    assert synth.rmse(G.get_vertices(), OG.states) < 1e-4


def test_huber_and_information_lm():
    g = small(5)
    inf = spd_info(g["v0"].shape[0], 9)
    G = mk(g, info=inf, kernel=L.KERNEL_HUBER, kdelta=0.1, fix_small_angle_b=1,
           pcg_rel_tol=1e-12, fd_delta=1e-6)
    OG = oracle_of(g, info=inf, kernel=1, kdelta=0.1)
    G.optimize(5)
    _, tr = OG.optimize(5, O.default_options(fix_small_angle_b=1, fd_delta=1e-6))
    assert abs(G.stats()[-1].chi2_after - tr[-1].chi2_after) < 1e-5 * tr[-1].chi2_after
    assert synth.rmse(G.get_vertices(), OG.states) < 1e-4


def test_three_level_multigrid_lm_matches_exact_oracle(monkeypatch):
    """An LM run whose PCG goes through a THREE-level cycle, against the oracle (missing #3): a
    Manhattan graph of 1500 vertices / 15 000 edges (1499 -> 174 -> 20 rows with the
    dense level capped at 64 rows), so that level 1 runs the residual pass, the fused
    prolongation + smoothing pass (`k_spmv_span<..., 3, float>`), the coarse restriction
    (`k_amg_restrict`), FP32 block copies and over-correction -- everything config 3's four-level
    cycle runs below level 0 -- while the oracle's exact LDL^T still finishes in ~25 s.  What this pins is the
    SYSTEM being solved and the LM around it: CG reaches the same x with any symmetric positive definite M^-1, so a
    coarse-level kernel that is subtly wrong only costs iterations here.  The kernels themselves are compared with a
    long-double restatement, operator by operator, in test_gpu_preconditioners.py.  delta = 1e-6,
    PCG tolerance 1e-12: chi2 trace equal to 1e-8 relative, identical trial counts, trajectory RMSE
    < 1e-4 (measured 9e-6 on the 3000-vertex run of scripts/gpu_parity_3000.py)."""
    monkeypatch.setenv("SIM3OPT_AMG_COARSEST", "64")
    synth.DRIFT_TARGET = 0.05
    g = synth.manhattan(1500, 15000, dims=(14, 14, 8))
    G = mk(g, fix_small_angle_b=1, fd_delta=1e-6, pcg_rel_tol=1e-12)
    rows = [int(r) for r in G.amg_hierarchy()[0]]
    assert G.preconditioner_in_use() == 2 and len(rows) == 3 and rows[0] == 1499 and rows[2] <= 64, rows
    assert G.optimize(4) == 4
    st = G.stats()
    assert all(s.pcg_rel_res <= 1e-12 for s in st)
    OG = oracle_of(g)
    it, tr = OG.optimize(4, O.default_options(fix_small_angle_b=1, fd_delta=1e-6, threads=8))
    assert it == 4 and [s.trials for s in st] == [t.trials for t in tr]
    for s, t in zip(st, tr):
        assert abs(s.chi2_after - t.chi2_after) < 1e-8 * t.chi2_after, (s.chi2_after, t.chi2_after)
    assert synth.rmse(G.get_vertices(), OG.states) < 1e-4
    # the same run without the FP32 copies and the over-correction: the same answer (they change
    # the preconditioner, not the system)
    monkeypatch.setenv("SIM3OPT_AMG_FP32", "0")
    monkeypatch.setenv("SIM3OPT_AMG_OVER", "1.0")
    G2 = mk(g, fix_small_angle_b=1, fd_delta=1e-6, pcg_rel_tol=1e-12)
    assert G2.optimize(4) == 4
    for s, t in zip(G2.stats(), tr):
        assert abs(s.chi2_after - t.chi2_after) < 1e-8 * t.chi2_after
    # (two preconditioners, the same systems solved to pcg_rel_tol = 1e-12: steps differ by up to ~ tol * cond;
    # measured cond(H + lambda I) of this graph after 4 LM iterations: 4.8e5 -- lambda 6.1e-5, eig(H) in
    # [4.3e-4, 238], profiles/r4_condition_numbers.json --; measured RMSE 4.8e-6)
    assert synth.rmse(G2.get_vertices(), G.get_vertices()) < 2e-5


def test_multigrid_in_the_reference_arithmetic_matches_oracle():
    """a9 as written: with the small-angle coefficient of sim3_rv.h:166 / :290 (the default) the
    multigrid hierarchy is the automatic choice too, sets up without a failing pivot and its PCG
    reaches the exact solve of the oracle's LDL^T: lock-step over four LM iterations from the
    oracle's own states (the configuration amplifies last-bit differences, so iterates are compared
    one iteration at a time; delta = 1e-6 keeps the finite-difference noise out of the comparison)."""
    synth.DRIFT_TARGET = 0.05
    g = synth.manhattan(400, 4000, dims=(6, 6, 10))
    G = mk(g, fd_delta=1e-6, pcg_rel_tol=1e-12)
    assert G.options().fix_small_angle_b == 0 and G.preconditioner_in_use() == 2
    OG = oracle_of(g)
    lam = 0.0
    for k in range(4):
        G.set_vertices(OG.states)
        G.set_options(user_lambda_init=lam)
        assert G.optimize(1) == 1
        s = G.stats()[0]
        it, tr = OG.optimize(1, O.default_options(fd_delta=1e-6, user_lambda_init=lam))
        t = tr[0]
        assert s.trials == t.trials, (k, s.trials, t.trials)
        assert s.pcg_rel_res <= 1e-12
        assert abs(s.chi2_after - t.chi2_after) < 1e-6 * t.chi2_after, (k, s.chi2_after, t.chi2_after)
        assert abs(s.lambda_ - t.lambda_) < 1e-5 * t.lambda_
        assert synth.rmse(G.get_vertices(), OG.states) < 1e-6
        lam = t.lambda_


def test_damping_dominated_solves_start_with_block_jacobi(monkeypatch):
    """Engine::adaptive_prec (round 3): with the automatic preconditioner a solve whose lambda is of the
    order of the diagonal of H starts with block-Jacobi (a few cheap iterations instead of a multigrid
    set-up); the rule changes which preconditioner runs, never what is solved: the LM trace with the
    rule equals the trace without it, and a lightly damped run never takes the shortcut."""
    synth.DRIFT_TARGET = 0.05
    g = synth.manhattan(3000, 30000, dims=(17, 17, 10))
    runs = {}
    for tag, adaptive, lam0 in (("on", "1", 50.0), ("off", "0", 50.0), ("on_light", "1", 0.0), ("off_light", "0", 0.0)):
        monkeypatch.setenv("SIM3OPT_ADAPTIVE_PREC", adaptive)
        G = mk(g, fix_small_angle_b=1, fd_delta=1e-6, pcg_rel_tol=1e-12, user_lambda_init=lam0)
        assert G.preconditioner_in_use() == 2
        assert G.optimize(4) == 4
        runs[tag] = ([s.chi2_after for s in G.stats()], [s.pcg_iters for s in G.stats()],
                     [s.trials for s in G.stats()], G.get_vertices(), [s.pcg_rel_res for s in G.stats()])
    for a, b in (("on", "off"), ("on_light", "off_light")):
        assert runs[a][2] == runs[b][2]
        assert np.allclose(runs[a][0], runs[b][0], rtol=1e-9, atol=0)
        assert synth.rmse(runs[a][3], runs[b][3]) < 1e-7
        assert max(runs[a][4]) <= 1e-12
    # heavily damped (lambda_0 = 50 against mean |H_dd| of a few hundred): other iteration counts, i.e.
    # the other preconditioner ran; lightly damped (g2o's lambda_0 = 1e-5 max |H_dd|): the same solves
    assert runs["on"][1] != runs["off"][1]
    assert runs["on_light"][1] == runs["off_light"][1]


def test_huber_and_information_lm_through_multigrid():
    """Robust weights and dense information matrices only change the numbers of H: the multigrid
    hierarchy (Galerkin products of whatever the linearisation wrote) must follow."""
    synth.DRIFT_TARGET = 0.05
    g = synth.manhattan(400, 4000, dims=(6, 6, 10))
    inf = spd_info(g["v0"].shape[0], 11)
    G = mk(g, info=inf, kernel=L.KERNEL_HUBER, kdelta=0.5, fix_small_angle_b=1,
           pcg_rel_tol=1e-12, fd_delta=1e-6)
    assert G.preconditioner_in_use() == 2
    OG = oracle_of(g, info=inf, kernel=1, kdelta=0.5)
    G.optimize(6)
    _, tr = OG.optimize(6, O.default_options(fix_small_angle_b=1, fd_delta=1e-6))
    assert all(s.pcg_rel_res <= 1e-12 for s in G.stats())
    assert abs(G.stats()[-1].chi2_after - tr[-1].chi2_after) < 1e-5 * tr[-1].chi2_after
    assert synth.rmse(G.get_vertices(), OG.states) < 1e-4


def test_determinism_and_warm_start():
    g = small(6)
    A = mk(g)
    B = mk(g)
    A.optimize(4)
    B.optimize(4)
    assert np.array_equal(A.get_vertices(), B.get_vertices())  # bitwise: no atomics, fixed orders
    # warm start (kitti_surf.cpp:1028-1039): continuing == restarting from the same estimates
    C = mk(dict(g, states=A.get_vertices()))
    A.optimize(2)
    C.optimize(2)
    assert np.array_equal(A.get_vertices(), C.get_vertices())
    D = mk(g)
    D.set_vertices(B.get_vertices())
    D.optimize(2)
    assert np.array_equal(D.get_vertices(), C.get_vertices())


def test_optimize_return_conventions():
    g = small(7)
    G = mk(g)
    assert G.optimize(3) == 3 and len(G.stats()) == 3
    assert G._L.sim3opt_optimize(G._g, 0) == 0


# ------------------------------------------------------------------ full-size properties
def _bsr_matvec(rowptr, colidx, blocks, x):
    import scipy.sparse as sp
    M = sp.bsr_matrix((blocks, colidx, rowptr), blocksize=(7, 7))
    return M @ x


def test_config2_chain_loop_full_size_properties():
    """10k vertices / 20k edges (BASELINE.json config 2)."""
    synth.DRIFT_TARGET = 0.05
    g = synth.chain_loop(10000, 20000)
    G = mk(g, fix_small_angle_b=1, pcg_rel_tol=1e-10)
    chi0 = G.chi2()
    e = G.edge_errors()
    assert abs(np.sum(e * e) - chi0) < 1e-9 * chi0  # checksum of checksums
    assert np.abs(e[g["n_loop"]:]).max() < 1e-9      # odometry residuals vanish at the init
    G.linearize()
    rowptr, colidx, blocks, b = G.get_system()
    nb, nnzb = G.system_dims()
    both_free = int(((g["v0"] != 0) & (g["v1"] != 0)).sum())
    assert nb == 9999 and nnzb == 9999 + 2 * both_free
    # symmetry of the stored pattern and values: H_ij == H_ji^T via an SpMV identity
    rng = np.random.default_rng(0)
    u, v = rng.standard_normal(7 * nb), rng.standard_normal(7 * nb)
    Hu, Hv = _bsr_matvec(rowptr, colidx, blocks, u), _bsr_matvec(rowptr, colidx, blocks, v)
    assert abs(v @ Hu - u @ Hv) < 1e-9 * abs(v @ Hu)
    # the PCG answer solves the system the kernels built
    lam = 1e-5 * max(np.abs(blocks[rowptr[:-1], d, d]).max() for d in range(7))
    x, it, rr = G.solve(lam)
    r = b - (_bsr_matvec(rowptr, colidx, blocks, x) + lam * x)
    assert np.linalg.norm(r) < 1e-7 * np.linalg.norm(b)
    # linearising again gives bit-identical output (idempotence / determinism)
    G.linearize()
    assert np.array_equal(G.get_system()[3], b)
    n = G.optimize(8)
    st = G.stats()
    assert n == 8 and st[-1].chi2_after < 0.05 * chi0
    assert all(s.chi2_after <= s.chi2_before for s in st)


def test_config3_manhattan_full_size_properties():
    """100k vertices / 1M edges (BASELINE.json config 3): properties only."""
    synth.DRIFT_TARGET = 0.05
    g = synth.manhattan()
    assert g["states"].shape[0] == 100000 and g["v0"].shape[0] == 1000000
    assert len({(a, b) for a, b in zip(g["v0"].tolist(), g["v1"].tolist())}) == 1000000
    G = mk(g, fix_small_angle_b=1, pcg_rel_tol=1e-8)
    chi0 = G.chi2()
    nb, nnzb = G.system_dims()
    both_free = int(((g["v0"] != 0) & (g["v1"] != 0)).sum())
    assert nb == 99999 and nnzb == 99999 + 2 * both_free
    n = G.optimize(3)
    st = G.stats()
    assert n == 3
    assert all(s.chi2_after <= s.chi2_before for s in st)
    assert st[-1].chi2_after < 0.2 * chi0
    # the automatic rule picks the multigrid preconditioner here: every solve converges (block-Jacobi
    # stops at the 1000-iteration cap from the third LM iteration on)
    assert all(s.pcg_rel_res <= 1e-8 and 0 < s.pcg_iters < 400 for s in st)
    assert abs(G.chi2() - st[-1].chi2_after) < 1e-9 * st[-1].chi2_after
    assert synth.rmse(G.get_vertices(), g["gt"]) < synth.rmse(g["states"], g["gt"])


@pytest.mark.parametrize("graph,slice_blocks", [("manhattan", None), ("manhattan", 0), ("kitti", None)])
def test_batched_rejected_trials_equal_sequential_solves(monkeypatch, graph, slice_blocks):
    """After a rejected LM trial the dampings of the next trials are known (g2o: lambda *= nu, nu *= 2), so their
    systems are solved together -- one pass over the blocks for up to four vectors (Engine::pcg_batch) -- and the
    trials evaluated in g2o's order.  Same trial counts, same lambda, same chi2, same estimates as solving them
    one after the other (options.pcg_batch = 1): bit for bit -- per system the batched kernels perform the
    one-system kernels' operations in the same order.  delta = 1e-9: LM reaches the noise floor of the
    numeric Jacobians after a few iterations and rejects trials in bursts (what the benchmark window shows).
    Three cases: a three-level hierarchy with the coarse levels run one system per grid slice (the default for
    levels whose blocks stay in cache) and with four systems per wavefront (slice_blocks = 0: the path the large
    levels of config 3 take); KITTI-00 with all 118 loops through a two-level hierarchy (restriction straight
    into the dense level)."""
    if slice_blocks is not None:
        monkeypatch.setenv("SIM3OPT_BATCH_SLICE_BLOCKS", str(slice_blocks))
    if graph == "kitti":
        g, iters = K.build_direct_graph(False), 40
    else:
        synth.DRIFT_TARGET = 0.05
        g, iters = synth.manhattan(3000, 30000, dims=(17, 17, 10)), 30
    runs = []
    for batch in (1, 0):
        G = mk(g, fix_small_angle_b=1, pcg_rel_tol=1e-8, preconditioner=2, pcg_batch=batch)
        assert G.preconditioner_in_use() == 2
        n = G.optimize(iters)
        st = G.stats()
        kt = G.kernel_times()
        runs.append(dict(n=n, trials=[s.trials for s in st], lam=[s.lambda_ for s in st], chi=[s.chi2_after for s in st],
                         pcg=[s.pcg_iters for s in st], states=G.get_vertices(), batches=int(kt.n_batches),
                         solves=int(kt.n_batched_solves)))
    seq, bat = runs
    print("trials", seq["trials"], "batches", bat["batches"], "systems in batches", bat["solves"])
    assert seq["batches"] == 0 and bat["batches"] >= 2 and bat["solves"] >= 2 * bat["batches"]
    assert max(seq["trials"]) >= 3  # (there were bursts of rejected trials to batch)
    assert seq["n"] == bat["n"] and seq["trials"] == bat["trials"] and seq["pcg"] == bat["pcg"]
    assert seq["lam"] == bat["lam"] and seq["chi"] == bat["chi"]
    assert np.array_equal(seq["states"], bat["states"])


def test_overcorrected_cycle_falls_back_instead_of_failing_the_trial(monkeypatch):
    """The multigrid cycle scales its coarse corrections by 1.8 / 1.6, which is safe
    only while the inexact coarse solves stay within (0, 2) of the exact ones.  Forced beyond that
    (1.9 / 1.7 breaks the PCG down on this graph) the solver must notice and solve again with the
    plain cycle -- not report a failed solve, which would make LM reject a good trial."""
    synth.DRIFT_TARGET = 0.05
    g = synth.manhattan()
    ref = mk(g, fix_small_angle_b=1, pcg_rel_tol=1e-8)
    assert ref.optimize(3) == 3
    monkeypatch.setenv("SIM3OPT_AMG_OVER", "1.9,1.7")
    G = mk(g, fix_small_angle_b=1, pcg_rel_tol=1e-8)
    assert G.optimize(3) == 3
    st, sr = G.stats(), ref.stats()
    assert [s.trials for s in st] == [s.trials for s in sr] == [1, 1, 1]
    for a, b in zip(st, sr):
        assert abs(a.chi2_after - b.chi2_after) < 1e-5 * b.chi2_after
        assert a.pcg_rel_res <= 1e-8


# ------------------------------------------------------------------ edge cases
def test_minimal_and_degenerate_graphs():
    I8 = np.array([0, 0, 0, 1, 0, 0, 0, 1.0])
    # two vertices, one edge, exact solution after one step in the well-posed arithmetic
    C = S3.exp(np.array([0.1, -0.2, 0.05, 1.0, 2.0, -1.0, 0.3]), fix_b=True)
    g = dict(states=np.stack([I8, I8]), fixed=np.array([1, 0], np.uint8),
             v0=np.array([0], np.int32), v1=np.array([1], np.int32), meas=C[None])
    G, OG = mk(g, fix_small_angle_b=1, fd_delta=1e-6, pcg_rel_tol=1e-14), oracle_of(g)
    n = G.optimize(8)
    it, tr = OG.optimize(8, O.default_options(fix_small_angle_b=1, fd_delta=1e-6))
    assert n >= 1 and G.stats()[-1].chi2_after < 1e-12
    assert np.abs(G.get_vertex(1) - C).max() < 1e-6          # S1 = C * S0
    assert synth.rmse(G.get_vertices(), OG.states) < 1e-6
    # already optimal graph (residual at rounding level): nothing moves, nothing blows up
    g0 = dict(g, states=np.stack([I8, C]))
    G0 = mk(g0)
    assert G0.chi2() < 1e-20
    assert 1 <= G0.optimize(5) <= 5 and G0.chi2() < 1e-20
    assert np.abs(G0.get_vertex(1) - C).max() < 1e-9
    # a component without any fixed vertex (gauge free): lambda keeps the system SPD, nothing blows up
    h = small(8, V=40, E=200)
    extra = np.stack([I8, S3.exp(np.array([0, 0, 0.2, 1, 0, 0, 0.0]), fix_b=True)])
    h2 = dict(states=np.concatenate([h["states"], extra]),
              fixed=np.concatenate([h["fixed"], [0, 0]]).astype(np.uint8),
              v0=np.concatenate([h["v0"], [40]]).astype(np.int32),
              v1=np.concatenate([h["v1"], [41]]).astype(np.int32),
              meas=np.concatenate([h["meas"], I8[None]]))
    G2, OG2 = mk(h2, fix_small_angle_b=1, fd_delta=1e-6, pcg_rel_tol=1e-12), oracle_of(h2)
    n2 = G2.optimize(5)
    OG2.optimize(5, O.default_options(fix_small_angle_b=1, fd_delta=1e-6))
    assert n2 == 5 and np.isfinite(G2.get_vertices()).all()
    assert abs(G2.stats()[-1].chi2_after - OG2.chi2(O.default_options(fix_small_angle_b=1))) \
        < 1e-6 * max(G2.stats()[-1].chi2_after, 1e-6)


def test_negative_w_quaternions_and_reinitialize():
    g = small(9)
    flip = g["states"].copy()
    flip[::2, :4] *= -1.0  # q and -q are the same rotation
    mflip = g["meas"].copy()
    mflip[1::2, :4] *= -1.0
    A = mk(g, fix_small_angle_b=1, fd_delta=1e-6)
    B = mk(dict(g, states=flip, meas=mflip), fix_small_angle_b=1, fd_delta=1e-6)
    assert abs(A.chi2() - B.chi2()) < 1e-9 * A.chi2()
    A.optimize(4)
    B.optimize(4)
    assert synth.rmse(A.get_vertices(), B.get_vertices()) < 1e-7
    # initializeOptimization() again keeps the current estimates (g2o semantics)
    before = A.get_vertices()
    A.initialize()
    assert np.array_equal(A.get_vertices(), before)
    assert abs(A.chi2() - A.stats()[-1].chi2_after if A.stats() else 0) >= 0
