"""GPU tests (-m gpu) of the marginal covariances (g2o's SparseOptimizer::computeMarginals): blocks of
(H + lambda I)^-1 by the block selected inversion on the exact factor's pattern (selinv_kernels.hpp),
against a dense inverse of the system the library itself linearised, on the graphs of the exact-solver
tests plus the Huber / information / two-fixed-vertex chain under both linear solvers."""
import numpy as np
import pytest

from sim3opt_amd import lib as L, synth
import kitti_graph as K

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps


def mk(g, ids=None, info=None, kernel=0, kdelta=0.0, fixed=None, **opts):
    G = L.Graph(**opts)
    ids = np.arange(g["states"].shape[0], dtype=np.int32) if ids is None else ids
    G.add_vertices(g["states"], g["fixed"] if fixed is None else fixed, ids)
    if info is None:
        G.add_edges(ids[g["v0"]], ids[g["v1"]], g["meas"])
    else:
        G.add_edges(ids[g["v0"]], ids[g["v1"]], g["meas"], info=info, kernel=kernel, kernel_delta=kdelta)
    G.initialize()
    return G, ids


def huber_chain():
    """tests/test_gpu_direct.py's chain: information matrices, Huber, parallel edges, two fixed vertices"""
    g = synth.chain_loop(300, 340)
    rng = np.random.default_rng(5)
    dup = rng.choice(g["v0"].shape[0], 25, replace=False)
    g = dict(g)
    g["v0"] = np.concatenate([g["v0"], g["v0"][dup]]).astype(np.int32)
    g["v1"] = np.concatenate([g["v1"], g["v1"][dup]]).astype(np.int32)
    g["meas"] = np.concatenate([g["meas"], g["meas"][dup]])
    g["fixed"] = g["fixed"].copy()
    g["fixed"][150] = 1
    M = rng.standard_normal((g["v0"].shape[0], 7, 7)) * 0.3
    info = np.einsum("kij,klj->kil", M, M) + np.eye(7)
    ids = (np.arange(300) * 7 + 3).astype(np.int32)
    return g, dict(ids=ids, info=info, kernel=L.KERNEL_HUBER, kdelta=0.3)


CASES = {
    "kitti_one_loop": (lambda: (K.build_direct_graph(True), {}), {}),
    "kitti_all_loops": (lambda: (K.build_direct_graph(False), {}), {}),
    "chain_200": (lambda: (synth.chain_loop(200, 230), {}), {}),
    "tiny_5": (lambda: (synth.chain_loop(5, 6, min_gap=2), {}), {}),
    "manhattan_300": (lambda: (synth.manhattan(300, 1500, dims=(8, 8, 3)), {}), dict(linear_solver=1)),
    "huber_chain_auto": (huber_chain, dict(fd_delta=1e-6)),
    "huber_chain_pcg": (huber_chain, dict(fd_delta=1e-6, linear_solver=0)),
}


def pairs_of(g, ids):
    """every free vertex with itself, then every edge between two free vertices; and their block rows"""
    free = np.flatnonzero(g["fixed"] == 0)
    row = np.full(g["fixed"].shape[0], -1)
    row[free] = np.arange(free.size)  # one rank: block rows in insertion order (g2o's hessianIndex)
    keep = (row[g["v0"]] >= 0) & (row[g["v1"]] >= 0)
    va, vb = g["v0"][keep], g["v1"][keep]
    pairs = np.stack([ids[va], ids[vb]], axis=1)
    return free, row, pairs, row[va], row[vb]


def blocks(Z, ra, rb):
    return np.stack([Z[7 * a:7 * a + 7, 7 * b:7 * b + 7] for a, b in zip(ra, rb)])


@pytest.mark.parametrize("name", sorted(CASES))
def test_marginals_match_dense_inverse(name):
    make, opts = CASES[name]
    g, extra = make()
    G, ids = mk(g, fix_small_angle_b=1, **extra, **opts)
    if name == "huber_chain_pcg":
        assert G.linear_solver_in_use() == 0
    elif name != "huber_chain_auto":
        assert G.linear_solver_in_use() == 1
    free, row, pairs, ra, rb = pairs_of(g, ids)
    G.linearize()
    H, _ = G.dense_system()
    n = H.shape[0]
    for lam in (0.0, 1e-2, 1.0):
        A = H + lam * np.eye(n)
        ev = np.linalg.eigvalsh(A)
        cond = ev[-1] / ev[0]
        Zr = np.linalg.inv(A)
        D = G.marginal_covariances(lam)
        E = G.marginals(pairs, lam)
        assert D.shape == (free.size, 7, 7) and E.shape == (pairs.shape[0], 7, 7)
        Dr = blocks(Zr, np.arange(free.size), np.arange(free.size))
        Er = blocks(Zr, ra, rb)
        scale = max(np.abs(Dr).max(), np.abs(Er).max())
        tol = max(1e-10, 1e3 * n * EPS * cond) * scale
        err = max(np.abs(D - Dr).max(), np.abs(E - Er).max())
        print(f"{name} lambda={lam:g}: cond2 {cond:.3e}, max|err| / max|ref| {err / scale:.2e} (bound {tol / scale:.2e})")
        assert err <= tol, (lam, cond, err / scale)
        # diagonal blocks exactly symmetric and positive definite
        assert np.array_equal(D, D.transpose(0, 2, 1))
        for d in D:
            np.linalg.cholesky(d)
        # the self pairs of marginals() are the same numbers as marginal_covariances()
        self_pairs = np.stack([ids[free], ids[free]], axis=1)
        assert np.array_equal(G.marginals(self_pairs, lam), D)
        # and the transposed pairs the transposed blocks
        assert np.array_equal(G.marginals(pairs[:, ::-1], lam), E.transpose(0, 2, 1))
    # bit-reproducible
    assert np.array_equal(G.marginal_covariances(1e-2), G.marginal_covariances(1e-2))
    G.close()


def test_marginals_do_not_depend_on_the_schedule(monkeypatch):
    """Bottom-subtree size and wavefronts per bottom group change which workgroup inverts what, never the
    order of summation: the same bits under every schedule."""
    g = K.build_direct_graph(False)
    _, _, pairs, _, _ = pairs_of(g, np.arange(g["states"].shape[0], dtype=np.int32))
    ref, groups = None, set()
    for subtree, wg in (("16", "256"), ("48", "512"), ("128", "384"), ("8", "64")):
        monkeypatch.setenv("SIM3OPT_DIRECT_SUBTREE", subtree)
        monkeypatch.setenv("SIM3OPT_DIRECT_WG_SUB", wg)
        G, _ = mk(g)
        groups.add(G.marginal_plan()["ngroups"])
        cur = (G.marginal_covariances(1e-2), G.marginals(pairs, 0.0))
        G.close()
        if ref is None:
            ref = cur
            continue
        assert np.array_equal(cur[0], ref[0]) and np.array_equal(cur[1], ref[1])
    assert len(groups) > 1


def test_marginals_error_paths():
    g = synth.chain_loop(200, 230)
    # no fixed vertex: H is singular (the gauge) -- an error at lambda = 0, never NaN / garbage
    for opts in (dict(), dict(linear_solver=0)):
        G, _ = mk(g, fixed=np.zeros_like(g["fixed"]), fix_small_angle_b=1, **opts)
        with pytest.raises(L.Sim3OptError) as e:
            G.marginal_covariances(0.0)
        assert e.value.code == L.ERR_STATE
        assert np.isfinite(G.marginal_covariances(1.0)).all()  # damped: well posed
        G.close()
    # a cleared dof_mask bit: zero rows in H
    G, _ = mk(g, fix_small_angle_b=1, dof_mask=0x3F)
    with pytest.raises(L.Sim3OptError) as e:
        G.marginal_covariances(0.0)
    assert e.value.code == L.ERR_STATE
    G.close()
    G, ids = mk(g, fix_small_angle_b=1)
    fixed_id = int(ids[np.flatnonzero(g["fixed"])[0]])
    with pytest.raises(L.Sim3OptError) as e:
        G.marginals([(fixed_id, 1)])
    assert e.value.code == L.ERR_ARG
    # a pair outside the factor's pattern (from the plan)
    P = G.marginal_plan()
    stored = set(zip(P["lrow"].tolist(), np.repeat(np.arange(P["nb"]), np.diff(P["colptr"])).tolist()))
    free = np.flatnonzero(g["fixed"] == 0)
    pos = np.empty(P["nb"], dtype=np.int64)
    pos[P["perm"]] = np.arange(P["nb"])
    out = next((a, b) for a in range(P["nb"]) for b in range(a) if (max(pos[a], pos[b]), min(pos[a], pos[b])) not in stored)
    with pytest.raises(L.Sim3OptError) as e:
        G.marginals([(int(ids[free[out[0]]]), int(ids[free[out[1]]]))])
    assert e.value.code == L.ERR_ARG
    assert np.isfinite(G.marginals([(int(ids[free[0]]), int(ids[free[0]]))])).all()  # still usable
    G.close()


@pytest.mark.parametrize("name", ["kitti_direct", "chain_200_pcg"])
def test_marginals_between_optimize_calls_change_nothing(name):
    """optimize(5); marginals; optimize(5) is bit-identical to optimize(5); optimize(5)"""
    if name == "kitti_direct":
        g, opts = K.build_direct_graph(True), {}
    else:
        g, opts = synth.chain_loop(200, 230), dict(linear_solver=0, fix_small_angle_b=1)
    runs = []
    for with_call in (False, True):
        G, _ = mk(g, **opts)
        assert G.linear_solver_in_use() == (1 if name == "kitti_direct" else 0)
        n1 = G.optimize(5)
        s1 = [(s.trials, s.chi2_before, s.chi2_after, s.lambda_, s.pcg_iters) for s in G.stats()]
        if with_call:
            assert np.isfinite(G.marginal_covariances(1e-2)).all()
            try:  # (KITTI-00 in the reference's arithmetic, at its noise floor: H may be numerically singular --
                G.marginal_covariances(0.0)  # a failing call must not interfere either)
            except L.Sim3OptError as e:
                assert e.code == L.ERR_STATE
            G.marginals([(1, 1)], 1.0)
        n2 = G.optimize(5)
        s2 = [(s.trials, s.chi2_before, s.chi2_after, s.lambda_, s.pcg_iters) for s in G.stats()]
        runs.append((n1, s1, n2, s2, np.array(G.get_vertices(), copy=True), G.chi2()))
        G.close()
    a, b = runs
    assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2] and a[3] == b[3]
    assert np.array_equal(a[4], b[4]) and a[5] == b[5]
