"""GPU tests (-m gpu) of options.cov_solver: sim3opt_covariances and sim3opt_gate_edges with the blocks of
(H + lambda I)^-1 taken from columns of the inverse, solved by the PCG the graph was initialised with
(engine_columns.hip, col_kernels.hpp) -- the path for graphs whose exact factorisation is refused.

Accuracy contract under test.  Every solved column y of a unit right-hand side g has ||g - (H + lambda I) y||_2 <=
cov_rel_tol (checked on the device by the SpMV), so ||y - y*||_2 <= cov_rel_tol / lambda_min(H + lambda I): every entry
of a returned block is within cov_rel_tol / (ev_min + lambda) of the true one.  Against a dense numpy inverse the
reference's own inversion error n eps cond2 max|ref| is added."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import oracle as O
from sim3opt_amd import lib as L, synth
import cov_ref as R
import pcg_ref as P
import test_gpu_covariances as TG

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
BASE = dict(fix_small_angle_b=1, fd_delta=1e-6, linear_solver=0, cov_solver=1)


@functools.lru_cache(maxsize=None)
def manhattan_400():
    return synth.manhattan(400, 4000, dims=(6, 6, 10))


@functools.lru_cache(maxsize=None)
def manhattan_3000():
    return synth.manhattan(3000, 30000, dims=(17, 17, 10))


@functools.lru_cache(maxsize=None)
def huber_chain():
    return TG.huber_chain()


def columns_request(T):
    """300 seeded pairs (plus the strata of cov_ref.seeded_pairs) and one full block column: every free vertex against
    the deepest vertex of the elimination tree, as test_gpu_covariances.request builds it"""
    ra, rb = R.seeded_pairs(T, 300, 17)
    row_of = np.empty(T.nb, dtype=np.int64)
    row_of[T.pos] = np.arange(T.nb)
    deep = row_of[int(np.argmax(T.depth))]
    return np.concatenate([ra, np.arange(T.nb)]), np.concatenate([rb, np.full(T.nb, deep)])


# name -> (graph and the arguments of mk, preconditioner, further options, dampings).  The chain preconditioner runs with
# segments of 32 rows instead of 256: ten segments instead of two on this 298-row chain, and a third of the time (its
# apply is one wavefront walking a segment; the iteration count is the same to 15 %).
DENSE = {
    "manhattan_400_multigrid": (lambda: (manhattan_400(), {}), 2, {}, (0.0, 1e-2, 1.0)),
    "huber_chain_block_jacobi": (huber_chain, 0, {}, (1e-2, 1.0)),
    "huber_chain_chain_segments": (huber_chain, 1, dict(chain_segment=32), (1e-2, 1.0)),
}


@pytest.mark.parametrize("name", sorted(DENSE))
def test_columns_match_dense_inverse(name):
    make, prec, more, lams = DENSE[name]
    g, extra = make()
    G, ids = TG.mk(g, preconditioner=prec, **more, **extra, **BASE)
    assert G.linear_solver_in_use() == 0 and G.preconditioner_in_use() == prec
    fid = TG.free_ids(g, ids)
    T = R.Tree(G.marginal_plan())
    ra, rb = columns_request(T)
    pairs = TG.pairs_of(fid, ra, rb)
    plan = G.covariance_columns_plan(pairs)
    G.linearize()
    H, _ = G.dense_system()
    n = H.shape[0]
    if name.startswith("manhattan"):
        assert n == 2793
    ev = np.linalg.eigvalsh(H)
    tol = G.options().cov_rel_tol
    assert tol == 1e-8
    diag = ra == rb
    assert diag.any()
    for lam in lams:
        cond = (ev[-1] + lam) / (ev[0] + lam)
        ref = TG.blocks(np.linalg.inv(H + lam * np.eye(n)), ra, rb)
        Z = G.covariances(pairs, lam)
        st = G.covariance_columns_stats()
        assert Z.shape == ref.shape
        bound = tol / (ev[0] + lam) + n * EPS * cond * np.abs(ref).max()
        err = np.abs(Z - ref).max()
        print(f"{name} lambda={lam:g}: cond2 {cond:.3e}, ev_min {ev[0]:.3e}, {st['vertices']} vertices, "
              f"{st['columns']} columns, {st['pcg_iters']} PCG iterations, {st['batches']} batches, "
              f"{st['refinements']} refinement rounds, worst residual {st['max_rel_residual']:.2e}; max|err| {err:.3e}, "
              f"bound {bound:.3e} (first term {tol / (ev[0] + lam):.3e})")
        assert err <= bound, (lam, err, bound)
        assert st["vertices"] == plan.size and st["columns"] == 7 * plan.size
        assert st["max_rel_residual"] <= tol and st["cov_rel_tol"] == tol
        assert st["batches"] == ((7 * plan.size + 3) // 4 if prec == 2 else 7 * plan.size)
        assert all(v == 0 for v in G.covariance_stats().values())  # the exact path's counters
        assert np.array_equal(Z[diag], Z[diag].transpose(0, 2, 1))  # diagonal blocks: exactly symmetric
        if lam == 1e-2:
            # the reversed request is the exact transpose, duplicates are identical: on a part of the request (seeded
            # pairs, a diagonal pair, a piece of the block column), whose cover is its own -- a request, its reverse
            # and its copy with duplicates have the same unordered pairs, hence the same cover and the same bits
            part = np.concatenate([np.arange(16), np.flatnonzero(diag)[:1], np.arange(ra.size - 8, ra.size)])
            Zp = G.covariances(pairs[part], lam)
            assert np.abs(Zp - ref[part]).max() <= bound
            assert np.array_equal(G.covariances(pairs[part][:, ::-1], lam), Zp.transpose(0, 2, 1))
            dup = np.concatenate([np.arange(10), np.arange(part.size), np.arange(10)[::-1]])
            assert np.array_equal(G.covariances(pairs[part][dup], lam), Zp[dup])
    G.close()


def test_refinement_reaches_the_tolerance(monkeypatch):
    """The PCG's own stopping test is in the norm of the preconditioner.  With the first pass stopped AT cov_rel_tol in
    that norm (the tuning knob SIM3OPT_COLS_FIRST_PASS = 1; two digits below it by default) the true residual of most
    columns is above the bound and the refinement has to bring it below: it does, and both runs are within
    cov_rel_tol / (lambda_min + lambda) <= cov_rel_tol of the true blocks at lambda = 1."""
    g, extra = huber_chain()
    lam, out = 1.0, []
    for first_pass in (None, "1"):
        if first_pass:
            monkeypatch.setenv("SIM3OPT_COLS_FIRST_PASS", first_pass)
        G, ids = TG.mk(g, preconditioner=1, chain_segment=32, **extra, **BASE)
        fid = TG.free_ids(g, ids)
        pairs = [(int(fid[3]), int(fid[200])), (int(fid[7]), int(fid[7])), (int(fid[250]), int(fid[40]))]
        out.append(G.covariances(pairs, lam))
        st = G.covariance_columns_stats()
        print(f"first pass {first_pass}: {st}")
        assert st["max_rel_residual"] <= st["cov_rel_tol"] == 1e-8
        assert (st["refinements"] > 0) == bool(first_pass)
        G.close()
    assert np.abs(out[0] - out[1]).max() <= 2e-8


def test_columns_where_the_exact_path_refuses():
    """Manhattan 3000 / 30000: the marginal plan is refused; one full block column by columns of the inverse, checked
    column by column as ||e_c - (H + lambda I) y_c||_2 <= cov_rel_tol + ||gamma(7 m_i + 3) (|A||y| + lambda |y|)_i||_2
    in numpy (m_i: stored blocks of row i; the second term is the rounding of numpy's own product)."""
    g = manhattan_3000()
    G, ids = TG.mk(g, preconditioner=2, **dict(BASE, cov_solver=0))
    assert G.linear_solver_in_use() == 0 and G.preconditioner_in_use() == 2
    fid = TG.free_ids(g, ids)
    nb = fid.size
    b = nb // 2
    pairs = np.stack([fid, np.full(nb, fid[b])], axis=1)
    lam = 1e-2
    with pytest.raises(L.Sim3OptError) as e:
        G.covariances(pairs, lam)
    assert e.value.code == L.ERR_STATE
    tol = G.options().cov_rel_tol
    G.linearize()
    rp, ci, blk, _ = G.get_system()
    A = sp.bsr_matrix((blk, ci, rp), shape=(7 * nb, 7 * nb)).tocsr()
    absA = abs(A)
    gam = np.asarray(P.gamma_k(7 * P.blocks_per_row(rp).astype(np.longdouble) + 3), dtype=float)
    for solver in (2, 1):
        G.set_options(cov_solver=solver)
        Z = G.covariances(pairs, lam)
        st = G.covariance_columns_stats()
        assert st["vertices"] == 1 and st["columns"] == 7 and st["batches"] == 2
        assert all(v == 0 for v in G.covariance_stats().values())
        Y = Z.reshape(7 * nb, 7)  # block (a, b) is rows a of the columns of b
        worst = 0.0
        for c in range(7):
            rhs = np.zeros(7 * nb)
            rhs[7 * b + c] = 1.0
            res = np.linalg.norm(rhs - (A @ Y[:, c] + lam * Y[:, c]))
            bound = tol + np.linalg.norm(gam * (absA @ np.abs(Y[:, c]) + lam * np.abs(Y[:, c])))
            worst = max(worst, res / bound)
            assert res <= bound, (solver, c, res, bound)
        print(f"manhattan_3000 cov_solver={solver}: {st['pcg_iters']} PCG iterations over 7 columns, "
              f"{st['refinements']} refinement rounds, library's worst residual {st['max_rel_residual']:.2e}, "
              f"numpy's worst residual / bound {worst:.2e}")
    G.close()


def test_column_bits_do_not_depend_on_batch_partners_or_schedule():
    g = manhattan_400()
    lam = 1e-2
    a, b, c = 250, 11, 120  # a's block row is the highest: with (b, b) and (c, c) its columns move to other batches
    ref = None
    for opts in (dict(), dict(pcg_batch=1), dict(pcg_check_every=1, pcg_graph=0)):
        G, _ = TG.mk(g, preconditioner=2, **opts, **BASE)
        Z1 = G.covariances([(a, a)], lam)
        s1 = G.covariance_columns_stats()
        Z3 = G.covariances([(a, a), (b, b), (c, c)], lam)
        s3 = G.covariance_columns_stats()
        assert G.covariance_columns_plan([(a, a), (b, b), (c, c)]).tolist() == [b, c, a]
        width = 1 if opts.get("pcg_batch") == 1 else 4
        assert s1["batches"] == -(-7 // width) and s3["batches"] == -(-21 // width)
        assert np.array_equal(Z3[0], Z1[0])
        if ref is None:
            ref = Z1[0]
        assert np.array_equal(Z1[0], ref), opts
        G.close()


def test_multigrid_graph_that_admits_no_batch_solves_one_column_at_a_time():
    """amg_fp32 = 0: the K-system passes exist for the FP32 cycle only, so the columns go through the one-system PCG with
    the FP64 cycle -- another preconditioner, the same contract: both within cov_rel_tol / (lambda_min + 1) of the truth"""
    g = manhattan_400()
    pairs, lam, out = [(250, 11), (120, 120), (11, 300)], 1.0, []
    for opts in (dict(), dict(amg_fp32=0)):
        G, _ = TG.mk(g, preconditioner=2, **opts, **BASE)
        out.append(G.covariances(pairs, lam))
        st = G.covariance_columns_stats()
        assert st["max_rel_residual"] <= st["cov_rel_tol"] == 1e-8
        assert st["batches"] == (-(-st["columns"] // 4) if not opts else st["columns"])
        G.close()
    assert np.abs(out[0] - out[1]).max() <= 2e-8 and np.abs(out[0]).max() > 1e-3


@pytest.mark.parametrize("name", ["manhattan_400_multigrid", "chain_200_block_jacobi"])
def test_column_calls_between_optimize_calls_change_nothing(name):
    """optimize(5); covariances + gate_edges; optimize(5) is bit-identical to optimize(5); optimize(5)"""
    if name.startswith("manhattan"):
        g, prec = manhattan_400(), 2
    else:
        g, prec = synth.chain_loop(200, 230), 0
    runs = []
    for with_call in (False, True):
        G, _ = TG.mk(g, preconditioner=prec, **BASE)
        assert G.linear_solver_in_use() == 0 and G.preconditioner_in_use() == prec
        fields = ("trials", "chi2_before", "chi2_after", "lambda_", "rho", "pcg_iters", "pcg_rel_res")
        n1 = G.optimize(5)
        s1 = [tuple(getattr(s, f) for f in fields) for s in G.stats()]
        if with_call:
            assert np.isfinite(G.covariances([(1, 150), (150, 1), (2, 2), (1, 2)], 1e-2)).all()
            assert G.covariance_columns_stats()["columns"] > 0
            meas = np.tile(np.array([0, 0, 0, 1, 0.5, 0, 0, 1.0]), (3, 1))
            _, _, d2 = G.gate_edges([1, 3, 0], [150, 90, 60], meas, lam=1e-2)  # (vertex 0 is fixed)
            assert np.isfinite(d2).all() and (d2 > 0).all()
        sched = G.pcg_schedule_stats()
        n2 = G.optimize(5)
        s2 = [tuple(getattr(s, f) for f in fields) for s in G.stats()]
        runs.append((n1, s1, n2, s2, sched, G.pcg_schedule_stats(), np.array(G.get_vertices(), copy=True), G.chi2()))
        G.close()
    a, b = runs
    assert a[:6] == b[:6]
    assert np.array_equal(a[6], b[6]) and a[7] == b[7]


def test_gate_by_columns_matches_numpy_restatement():
    """test_gpu_covariances.test_gate_matches_numpy_restatement's restatement and candidates at lambda = 1e-2 on a
    multigrid graph, closed-form Jacobians; its bound on S with the covariance term replaced by this path's:
    dSigma = 14 (cov_rel_tol / (ev_min + lambda) + n eps cond2 max|Sigma|)."""
    lam = 1e-2
    g = manhattan_400()
    G, _ = TG.mk(g, preconditioner=2, jacobians=1, **BASE)
    G.optimize(3)
    states = np.array(G.get_vertices(), copy=True)
    v0, v1, meas = TG.gate_candidates(g, states)
    m = v0.size
    half = m // 2
    rng = np.random.default_rng(43)
    M = rng.standard_normal((m - half, 7, 7)) * 0.3
    info = np.einsum("kij,klj->kil", M, M) + np.eye(7)
    e, S, d2 = (np.concatenate(x) for x in zip(G.gate_edges(v0[:half], v1[:half], meas[:half], lam=lam),
                                               G.gate_edges(v0[half:], v1[half:], meas[half:], info=info, lam=lam)))
    assert G.covariance_columns_stats()["columns"] > 0 and all(v == 0 for v in G.covariance_stats().values())
    eI, SI, dI = G.gate_edges(v0[:half], v1[:half], meas[:half], info=np.tile(np.eye(7), (half, 1, 1)), lam=lam)
    assert np.array_equal(eI, e[:half]) and np.array_equal(SI, S[:half]) and np.array_equal(dI, d2[:half])
    G.linearize()
    H, _ = G.dense_system()
    n = H.shape[0]
    ev = np.linalg.eigvalsh(H)
    cond = (ev[-1] + lam) / (ev[0] + lam)
    Zr = np.linalg.inv(H + lam * np.eye(n))
    row = np.full(g["fixed"].shape[0], -1)
    row[g["fixed"] == 0] = np.arange(n // 7)
    oopt = O.default_options(fix_small_angle_b=1, fd_delta=1e-6)
    Sig = np.zeros((m, 14, 14))
    for k in range(m):
        r = (row[v0[k]], row[v1[k]])
        for i in range(2):
            for j in range(2):
                if r[i] >= 0 and r[j] >= 0:
                    Sig[k, 7 * i:7 * i + 7, 7 * j:7 * j + 7] = Zr[7 * r[i]:7 * r[i] + 7, 7 * r[j]:7 * r[j] + 7]
    tol = G.options().cov_rel_tol
    dSigma = 14 * (tol / (ev[0] + lam) + n * EPS * cond * np.abs(Sig).max())
    dJ = TG.JAC_MARGIN * TG.JAC_REFS_DISAGREE
    worst = dict(S=0.0, d2=0.0, e=0.0)
    fails = []
    for k in range(m):
        s0, s1 = states[v0[k]], states[v1[k]]
        er = O.edge_error(meas[k], s0, s1, oopt)
        A, B = O.edge_jacobians(meas[k], s0, s1, oopt)
        J = np.hstack([A, B])
        Oi = np.eye(7) if k < half else np.linalg.inv(info[k - half])
        Sr = J @ Sig[k] @ J.T + Oi
        x = np.linalg.solve(Sr, er)
        dr = float(er @ x)
        nJ2 = np.linalg.norm(J, 2) ** 2
        tS = nJ2 * dSigma + (2 * dJ + dJ * dJ) * nJ2 * np.linalg.norm(Sig[k], 2) + 1e-13 * np.linalg.norm(Oi, 2)
        de = 1e-13 * max(1.0, np.linalg.norm(er))
        td = np.linalg.norm(x) ** 2 * tS + 2 * np.linalg.norm(x) * de
        errS, errd, erre = np.linalg.norm(S[k] - Sr, 2), abs(d2[k] - dr), np.abs(e[k] - er).max()
        worst["S"] = max(worst["S"], errS / tS)
        worst["d2"] = max(worst["d2"], errd / td if td > 0 else 0.0)
        worst["e"] = max(worst["e"], erre / de)
        if not (errS <= tS and erre <= de):
            fails.append(("S / e", k, errS, tS, erre, de))
        if k % 3 == 0:  # no perturbation: e and d2 vanish
            if not (np.linalg.norm(e[k]) <= 1e-12 and d2[k] <= 1e-20):
                fails.append(("zero", k, np.linalg.norm(e[k]), d2[k]))
        elif not errd <= td:
            fails.append(("d2", k, errd, td))
        assert np.array_equal(S[k], S[k].T)
    print(f"gate by columns: cond2 {cond:.3e}, dSigma {dSigma:.2e}; worst error / bound: S {worst['S']:.2e}, "
          f"d2 {worst['d2']:.2e}, e {worst['e']:.2e}; d2 in [{d2.min():.2e}, {d2.max():.2e}]")
    assert not fails, fails[:5]
    assert np.all(d2[2::3] > d2[1::3]) and np.all(d2[1::3] > d2[0::3])  # the same pair, farther off
    # cov_solver = 2 on a graph whose marginal plan is accepted: the exact path, bit for bit
    G.set_options(cov_solver=0)
    exact = G.gate_edges(v0[:half], v1[:half], meas[:half], lam=lam)
    assert G.covariance_stats()["selinv"] + G.covariance_stats()["chunks"] >= 1
    G.set_options(cov_solver=2)
    auto = G.gate_edges(v0[:half], v1[:half], meas[:half], lam=lam)
    assert G.covariance_stats()["selinv"] + G.covariance_stats()["chunks"] >= 1
    assert all(np.array_equal(x, y) for x, y in zip(exact, auto))
    G.close()


def test_columns_of_a_disconnected_graph():
    g = R.two_chains()
    G, ids = TG.mk(g, preconditioner=0, **BASE)
    fid = TG.free_ids(g, ids)
    nb = fid.size
    ra, rb = (x.ravel() for x in np.meshgrid(np.arange(nb), np.arange(nb)))
    Z = G.covariances(TG.pairs_of(fid, ra, rb), 1e-2)
    first = int((np.asarray(g["fixed"])[:30] == 0).sum())  # block rows of the first chain
    cross = (ra < first) != (rb < first)
    assert cross.any() and not cross.all()
    assert np.all(Z[cross] == 0.0)
    assert np.all(np.abs(Z[~cross]).reshape(-1, 49).max(axis=1) > 0.0)
    G.close()


def test_column_error_paths():
    # a graph on the exact LM solver has no PCG to solve columns with
    g = R.GRAPHS["chain_40"]()
    G, ids = TG.mk(g, **dict(BASE, linear_solver=1))
    assert G.linear_solver_in_use() == 1
    with pytest.raises(L.Sim3OptError) as e:
        G.covariances([(3, 20)], 1e-2)
    assert e.value.code == L.ERR_STATE
    G.close()
    # cond2 = 3.5e11 at lambda = 0 and 50 iterations per solve: the tolerance is out of reach -- an error that names
    # the vertex, outputs untouched, and the graph works afterwards
    g, extra = huber_chain()
    G, ids = TG.mk(g, preconditioner=0, pcg_max_iters=50, **extra, **BASE)
    fid = TG.free_ids(g, ids)
    pairs = np.array([(fid[3], fid[200]), (fid[7], fid[7])], dtype=np.int32)
    cov = np.full((2, 49), np.nan)
    a, b = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    rc = G._L.sim3opt_covariances(G._g, 0.0, 2, a.ctypes.data_as(ip), b.ctypes.data_as(ip), cov.ctypes.data_as(dp))
    assert rc == L.ERR_STATE
    msg = G._L.sim3opt_last_error(G._g).decode()
    assert "vertex id" in msg and "cov_rel_tol" in msg, msg
    assert np.isnan(cov).all()
    assert G.covariance_columns_stats()["max_rel_residual"] > 1e-8
    meas = np.tile(np.array([0, 0, 0, 1, 0.5, 0, 0, 1.0]), (2, 1))
    out = (np.full((2, 7), np.nan), np.full((2, 49), np.nan), np.full(2, np.nan))
    with pytest.raises(L.Sim3OptError) as e:
        G.gate_edges(pairs[:, 0], [int(fid[100]), int(fid[150])], meas, lam=0.0, out=out)
    assert e.value.code == L.ERR_STATE
    assert all(np.isnan(o).all() for o in out)
    G.set_options(pcg_max_iters=0)
    assert np.isfinite(G.covariances(pairs, 1.0)).all()
    assert G.optimize(2) == 2
    # a fixed vertex in a pair is refused before anything is launched
    fixed_id = int(ids[np.flatnonzero(g["fixed"])[0]])
    for bad in ([(fixed_id, int(fid[5]))], [(int(fid[5]), fixed_id)], [(int(fid[5]), 5)]):
        with pytest.raises(L.Sim3OptError) as e:
            G.covariances(bad, 1e-2)
        assert e.value.code == L.ERR_ARG
    G.close()
