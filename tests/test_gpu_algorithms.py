"""Gauss-Newton and Powell's dogleg on the GPU (options.algorithm = 1 / 2) against the numpy restatement
of their rules in tests/algorithms_ref.py (CPU oracle: H and b, chi2, Sim(3) exp / mul; a dense Cholesky solve).

Graphs: a 240-vertex chain with 481 loop closures (cond(H) ~ 1e8 at the start), dense information matrices, the well-posed arithmetic
(fix_small_angle_b = 1) and central differences with delta = 1e-4 on both sides: the two linearisations evaluate the
same difference quotient, so they differ by the rounding of exp / log amplified by 1 / delta -- with delta = 1e-6 that
alone left the chi2 of a step 4e-9 apart (the exact and the PCG solve on the device agreed with each other).  The dogleg runs start far from the optimum with a small trust radius, so that the
steepest-descent, dogleg and Gauss-Newton steps all occur, and stop before the noise floor, where accept / reject
decisions are made by rounding."""
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from sim3opt_amd import lib as L, synth
import algorithms_ref as R
import dist_helpers as H
import kitti_graph as K

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = dict(fix_small_angle_b=1, fd_delta=1e-4)
SOLVERS = {"exact": dict(linear_solver=1),
           "pcg": dict(linear_solver=0, preconditioner=0, pcg_rel_tol=1e-12, pcg_max_iters=20000)}


def chain_graph(isolated=False):
    synth.DRIFT_TARGET = 0.6
    g = synth.chain_loop(240, 720, seed_graph=7101, seed_noise=7102, min_gap=5)
    rng = np.random.default_rng(31)
    M = rng.standard_normal((len(g["v0"]), 7, 7)) * 0.3
    g["info"] = np.einsum("kij,klj->kil", M, M) + np.eye(7)
    if isolated:  # a free vertex no edge touches: a zero block row of H (the factorisation's pivot is 0)
        g["states"] = np.vstack([g["states"], [0, 0, 0, 1, 1.0, 2.0, 3.0, 1.0]])
        g["fixed"] = np.append(g["fixed"], 0).astype(np.uint8)
    return g


def mk(g, **opts):
    G = L.Graph(**opts)
    G.add_vertices(g["states"], g["fixed"])
    G.add_edges(g["v0"], g["v1"], g["meas"], info=g.get("info"))
    G.initialize()
    return G


def oracle_of(g):
    inf = g.get("info")
    return O.Graph(g["states"], g["fixed"], g["v0"], g["v1"], g["meas"],
                   info=None if inf is None else np.asarray(inf).transpose(0, 2, 1).reshape(-1, 49))


def rel(a, b):
    return abs(a - b) / abs(b)


def states_close(a, b, tol):
    return np.abs(a - b).max() <= tol * max(1.0, np.abs(b).max())


# chi2 of the dogleg runs: measured to 2.9e-9 of the restatement (iteration 9, a GN step that divides chi2 by 48 and
# so magnifies the step's relative difference as much); every discrete decision -- trials, step type, delta -- equal
DL_CHI_TOL = 5e-9


def check_dogleg(G, n, tr, chi_tol=DL_CHI_TOL):
    st, ts = G.stats(), G.trust_region_stats()
    assert n == len(tr) == len(st) == len(ts)
    for k, (s, t, r) in enumerate(zip(st, ts, tr)):
        assert s.trials == r["trials"], (k, s.trials, r["trials"])
        assert t.step == r["step"], (k, t.step, r["step"])
        assert rel(t.delta_before, r["delta_before"]) < 1e-9 and rel(t.delta_after, r["delta_after"]) < 1e-9, k
        assert rel(s.chi2_before, r["chi2_before"]) < chi_tol, (k, rel(s.chi2_before, r["chi2_before"]))
        assert rel(s.chi2_after, r["chi2_after"]) < chi_tol, (k, rel(s.chi2_after, r["chi2_after"]))
        assert t.was_pd == int(r["was_pd"]) and s.lambda_ == pytest.approx(r["lambda_"], rel=1e-12, abs=0.0), k
        assert rel(t.alpha, r["alpha"]) < 1e-7 and rel(t.norm_sd, r["norm_sd"]) < 1e-7, k
        assert rel(t.norm_gn, r["norm_gn"]) < 1e-7 and rel(t.norm_dl, r["norm_dl"]) < 1e-7, k


# ------------------------------------------------------------------ 1. Gauss-Newton
@pytest.mark.parametrize("solver", ["exact", "pcg"])
def test_gauss_newton_matches_restatement(solver):
    g = chain_graph()
    G = mk(g, algorithm=L.ALGORITHM_GAUSS_NEWTON, **BASE, **SOLVERS[solver])
    assert G.linear_solver_in_use() == (1 if solver == "exact" else 0)
    OG = oracle_of(g)
    n_ref, tr = R.gauss_newton(OG, 6, O.default_options(**BASE))
    assert G.optimize(6) == n_ref == 6
    st = G.stats()
    assert [s.trials for s in st] == [1] * 6 and all(s.lambda_ == 0.0 for s in st)
    for k, (s, r) in enumerate(zip(st, tr)):
        assert rel(s.chi2_before, r["chi2_before"]) < 1e-9, (k, rel(s.chi2_before, r["chi2_before"]))
        assert rel(s.chi2_after, r["chi2_after"]) < 1e-9, (k, rel(s.chi2_after, r["chi2_after"]))
    assert st[-1].chi2_after < 1e-3 * st[0].chi2_before
    assert states_close(G.get_vertices(), OG.states, 1e-9)
    if solver == "pcg":
        assert all(s.pcg_iters > 0 and s.pcg_capped == 0 for s in st)
    G.close()


# ------------------------------------------------------------------ 2. dogleg
@pytest.mark.parametrize("solver", ["exact", "pcg"])
def test_dogleg_matches_restatement(solver):
    g = chain_graph()
    G = mk(g, algorithm=L.ALGORITHM_DOGLEG, dl_delta_init=0.1, **BASE, **SOLVERS[solver])
    OG = oracle_of(g)
    n, tr = R.dogleg(OG, 11, O.default_options(**BASE), delta_init=0.1)
    assert G.optimize(11) == n == 11
    check_dogleg(G, n, tr)
    steps = [t.step for t in G.trust_region_stats()]
    assert {L.STEP_SD, L.STEP_DL, L.STEP_GN} <= set(steps), steps
    assert all(t.was_pd == 1 for t in G.trust_region_stats())
    assert all(s.pcg_capped == 0 for s in G.stats())
    assert states_close(G.get_vertices(), OG.states, 1e-9)
    G.close()


# ------------------------------------------------------------------ 3. H not positive definite
def test_dogleg_damps_a_singular_system_like_the_restatement():
    g = chain_graph(isolated=True)
    G = mk(g, algorithm=L.ALGORITHM_DOGLEG, dl_delta_init=0.1, **BASE, **SOLVERS["exact"])
    OG = oracle_of(g)
    n, tr = R.dogleg(OG, 6, O.default_options(**BASE), delta_init=0.1)
    assert G.optimize(6) == n == 6
    check_dogleg(G, n, tr)
    st, ts = G.stats(), G.trust_region_stats()
    # the first solve fails, the damped one at lambda_init x factor succeeds, lambda_c then shrinks by factor / 2
    assert st[0].lambda_ == pytest.approx(1e-6, rel=1e-15) and st[1].lambda_ == pytest.approx(2e-7, rel=1e-15)
    assert all(s.lambda_ > 0 for s in st) and all(t.was_pd == 0 for t in ts)
    assert np.array_equal(G.get_vertices()[-1], g["states"][-1])  # (b is 0 there: the vertex stays)
    G.close()


def test_gauss_newton_fails_on_a_singular_system():
    g = chain_graph(isolated=True)
    G = mk(g, algorithm=L.ALGORITHM_GAUSS_NEWTON, **BASE, **SOLVERS["exact"])
    with pytest.raises(L.Sim3OptError):
        G.optimize(3)  # g2o's Fail: optimize() returns 0
    assert len(G.stats()) == 1 and np.array_equal(G.get_vertices(), g["states"])
    G.close()


# ------------------------------------------------------------------ 4. frozen rotations
def test_dogleg_with_frozen_rotations():
    g = chain_graph()
    opts = dict(BASE, dof_mask=0x78)
    G = mk(g, algorithm=L.ALGORITHM_DOGLEG, dl_delta_init=1.0, **opts, **SOLVERS["exact"])
    OG = oracle_of(g)
    n, tr = R.dogleg(OG, 6, O.default_options(**opts), delta_init=1.0)
    assert G.optimize(6) == n == 6
    check_dogleg(G, n, tr)
    assert G.trust_region_stats()[0].was_pd == 0  # frozen components: zero rows of H
    assert states_close(G.get_vertices(), OG.states, 1e-9)
    G.close()


# ------------------------------------------------------------------ 5. KITTI-00, one loop
def test_kitti_one_loop_dogleg_reaches_the_lm_minimum():
    g = K.build_direct_graph(True)
    res = {}
    for name, alg in (("lm", L.ALGORITHM_LM), ("dogleg", L.ALGORITHM_DOGLEG)):
        G = mk(g, fix_small_angle_b=1, algorithm=alg)
        assert G.optimize(100) > 0
        res[name] = (G.stats()[-1].chi2_after, G.get_vertices())
        G.close()
    (c_lm, s_lm), (c_dl, s_dl) = res["lm"], res["dogleg"]
    assert rel(c_dl, c_lm) < 1e-6, (c_dl, c_lm)
    assert synth.rmse(s_dl, s_lm) < 1e-4


# ------------------------------------------------------------------ 6. two ranks
def test_dogleg_two_ranks_match_one():
    g = chain_graph()
    opts = dict(device=0, algorithm=L.ALGORITHM_DOGLEG, dl_delta_init=0.1, **BASE, **SOLVERS["pcg"])
    tg = H.ThreadGroup(2)

    def rank_body(rank):
        G = L.Graph(**opts)
        G.add_vertices(g["states"], g["fixed"])
        G.add_edges(g["v0"], g["v1"], g["meas"], info=g["info"])
        tg.attach(G, rank)
        G.initialize()
        n = G.optimize(11)
        out = dict(n=n, states=G.get_vertices(), chi=[s.chi2_after for s in G.stats()],
                   trials=[s.trials for s in G.stats()], steps=[t.step for t in G.trust_region_stats()],
                   capped=sum(s.pcg_capped for s in G.stats()))
        G.close()
        return out

    res = tg.run(rank_body)
    G1 = mk(g, **opts)
    assert G1.optimize(11) == 11
    chi1 = [s.chi2_after for s in G1.stats()]
    for r in res:
        assert np.array_equal(r["states"], res[0]["states"]) and r["chi"] == res[0]["chi"]
        assert r["capped"] == 0 and r["n"] == 11 and r["trials"] == [s.trials for s in G1.stats()]
        assert r["steps"] == [t.step for t in G1.trust_region_stats()]
        # two PCG solves to 1e-12 in different summation orders: 1.7e-9 measured, at the same GN steps as above
        assert max(rel(a, b) for a, b in zip(r["chi"], chi1)) < DL_CHI_TOL
    G1.close()


# ------------------------------------------------------------------ 7. LM unchanged
def test_explicit_lm_is_bit_identical_to_the_default():
    g = chain_graph()
    A = mk(g, **BASE)
    B = mk(g, algorithm=L.ALGORITHM_LM, **BASE)
    assert A.optimize(5) == B.optimize(5) == 5
    assert np.array_equal(A.get_vertices(), B.get_vertices())
    assert [s.chi2_after for s in A.stats()] == [s.chi2_after for s in B.stats()]
    with pytest.raises(L.Sim3OptError):
        B.trust_region_stats()  # not a dogleg run
    A.close()
    B.close()


# ------------------------------------------------------------------ 8. the g2o-named shim
def test_algorithm_shim_gpu_part(tmp_path):
    exe = str(tmp_path / "algorithms_conformance")
    libdir = os.path.join(ROOT, "sim3opt_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-DSIM3OPT_G2O_NAMES",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "mock_eigen"),
                           os.path.join(ROOT, "tests", "cxx", "algorithms_conformance.cpp"), "-L" + libdir,
                           "-lsim3opt", "-Wl,-rpath," + libdir, "-o", exe])
    r = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout
