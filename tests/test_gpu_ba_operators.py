"""GPU tests (-m gpu) of the bundle-adjustment kernels as operators: the intermediates of one LM trial of
sim3opt_amd/csrc/ba.hip -- linearisation, point blocks, Z, the reduced camera system, the step of the exact solver and
the iterates of k_ba_pcg, back-substitution, the exp-map update, chi2 and the scale term -- are read out of the device
(lib.BundleAdjuster.debug_*) and compared with tests/ba_ref.py in long double.  An LM loop forgives a slightly wrong
g, a lost pair of a block's list or a wrong quaternion branch nobody visits; these tests do not (tests/test_ba_ref.py
asserts that each such defect moves the result by >= 1e4 x the tolerance used here).

Every case comes with the PATH CONDITION it exists for (tests/ba_cases.py), asserted here on the pattern and the
dimensions the DEVICE reports.

Three kinds of check:
  derived ...... the inputs are the device's own arrays bit for bit and the operation is sums of products:
                 |dev - ld| <= gamma(k) x (the same expression with absolute values), k = roundings on the longest path
                 to the entry for any summation order and any FMA contraction (the counts: ba_ref.K_Z ... k_sum, with
                 their reasons).  An entry whose bound is zero -- pad rows and columns, rows of fixed cameras -- must be
                 exact.
  measured ..... another formula order, an inverse, libm or an iteration: amg_ref.noise_and_tol (32 x |float64
                 restatement - long double|, floored at 4u).  Each case prints noise and the device's ratio (-s);
                 DESIGN.md 5c records the table.
  exact ........ read-outs change nothing; fixed cameras and a failed trial move nothing; g = 0 takes no iteration.
"""
import copy
import ctypes

import numpy as np
import pytest

from sim3opt_amd import lib as L
import amg_ref as R
import ba_cases as C
import ba_ref as BR

LD, U = R.LD, R.U
pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not R.longdouble_ok(), reason="np.longdouble has no 64-bit mantissa here")]

LAMBDA_REL = 1e-4  # damping of the derived checks, relative to the device's max diagonal entry
SOLVE_CASES = ("lists", "branches", "pcg_1", "pcg_16", "pcg_17", "pcg_146", "pcg_147", "tiny")
REDUCED_CASES = SOLVE_CASES + ("pcg_1030",)
ITERATE_CASES = ("lists",) + tuple(C.PCG_SIZES)


def new_adjuster(name, **opts):
    P = C.problem(name)
    b = L.BundleAdjuster(**opts)
    b.set_problem(P.cams, P.points, P.oc, P.op, P.uv, P.f, P.cx, P.cy)
    if P.fixed.any():
        b.set_fixed_cameras(P.fixed.astype(np.uint8))
    return b, P


_dev = {}


def device(name, solver=-1):
    """(adjuster, the case's problem with the DEVICE's estimate -- set_problem normalises the quaternions), once."""
    if (name, solver) not in _dev:
        b, P = new_adjuster(name, linear_solver=solver)
        Pd = copy.copy(P)
        Pd.cams, Pd.points = b.cameras(), b.points()
        _dev[(name, solver)] = (b, Pd)
    return _dev[(name, solver)]


def lam_of(b):
    return LAMBDA_REL * b.debug_reduced(1.0)["maxdiag"]


def report(name, what, noise, ratio):
    print(f"[ba-op] {name:9s} {what:22s} noise {noise:.2e}  device at {ratio:.3f} x tolerance")


def measured(name, what, dev, f64, ld):
    noise, tol = R.noise_and_tol(f64, ld)
    ratio = R.relerr(dev, ld) / tol
    report(name, what, noise, ratio)
    return ratio


# ------------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("name", C.CASES)
def test_every_case_meets_its_path_condition_on_the_device(name):
    b, P = device(name, 0 if name.startswith(("big_", "pcg_1030")) else -1)
    if name.startswith("big_chi_"):
        f = C.facts(P, None, None, b.dims())
    else:
        rptr, bcol = b.debug_pattern()
        f = C.facts(P, rptr, bcol, b.dims())  # (asserts that the device's pattern is the restated one)
    print(C.describe(name, f))
    C.check_path(name, f)


# ------------------------------------------------------------------------------------------------ derived bounds
def reduced_ratios(name, b, P, lam, big=False):
    """error / derived bound of every array of the reduced read-out at damping lam, pads and fixed cameras asserted
    exact; (ratios, the read-out).  big: S's magnitude by float64 pair sums (ba_ref.reduced_system, mag_dt)."""
    nc, npt, _ = b.dims()
    lin = b.debug_linearization()
    d = b.debug_reduced(lam)
    lists = BR.pair_lists(P.oc, P.op, nc)
    assert np.array_equal(lists["rptr"], d["rptr"]) and np.array_equal(lists["bcol"], d["bcol"])
    H, bp, bp_mag, m = BR.point_blocks(lin, P.op, npt, LD)
    ratios = dict(b_p=BR.derived_ratio(d["b_p"], bp, bp_mag, BR.k_bp(m)[:, None]))
    hd = H.diagonal(0, 1, 2).max(1)
    ratios["point_maxdiag"] = BR.derived_ratio(d["point_maxdiag"], hd, hd, BR.k_bp(m))
    ratios["Hpp_inv"], kappa = BR.inverse_residual_ratio(d["Hpp_inv"], H, lam, m)
    Z, Zmag = BR.z_blocks(lin, d["Hpp_inv"], P.op, LD)
    ratios["Z"] = BR.derived_ratio(d["Z"], Z, Zmag, BR.K_Z)
    ref = BR.reduced_system(lin, d["Z"], d["b_p"], P.oc, P.op, lists, P.fixed, lam, LD,
                            mag_dt=np.float64 if big else None)
    ratios["S"] = BR.derived_ratio(d["S"], ref["S"], ref["S_mag"], BR.s_counts(ref, lists, nc))
    nd = ref["nd"][:, None]
    ratios["b_c"] = BR.derived_ratio(d["b_c"], ref["b_c"], ref["bc_mag"], BR.k_bc(nd))
    ratios["cam_maxdiag"] = BR.derived_ratio(d["cam_maxdiag"], ref["cdmax"], ref["cdmax"], BR.k_bc(nd))
    ratios["g"] = BR.derived_ratio(d["g"], ref["g"], ref["g_mag"], BR.k_g(nd))
    print(f"[ba-op] {name}: lambda {lam:.3e}, kappa_1(H_pp + lambda I) <= {kappa:.2e}, error / derived bound: " +
          ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    # pads and fixed cameras, stated outright
    dg = lists["brow"] == lists["bcol"]
    assert (d["S"][:, 6, :6] == 0).all() and (d["S"][:, :6, 6] == 0).all() and np.array_equal(d["S"][:, 6, 6], dg * 1.0)
    assert (d["g"][:, 6] == 0).all() and (d["b_c"][:, 6] == 0).all() and (d["cam_maxdiag"][:, 6] == 0).all()
    fb = ref["fixed_block"]
    assert np.array_equal(d["S"][fb & dg], np.tile(np.eye(7), (int((fb & dg).sum()), 1, 1))) and (d["S"][fb & ~dg] == 0).all()
    assert (d["g"][P.fixed] == 0).all() and (d["b_c"][P.fixed] == 0).all()
    assert d["maxdiag"] == max(d["point_maxdiag"].max(), d["cam_maxdiag"].max())
    return ratios, d


@pytest.mark.parametrize("name", REDUCED_CASES)
def test_reduced_system_within_the_derived_bounds(name):
    """From the device's lin: b_p (k = 2 m), the largest diagonal entry of H_pp (2 m), Hpp_inv (H_pp + lambda I) - I
    (ba_ref.inverse_residual_ratio).  From lin and the device's Hpp_inv: Z (k = 5).  From lin, Z and b_p of the device:
    S (k = 3 pairs + 2 nd + 3), b_c and the cameras' diagonals (2 nd), g (5 nd + 1).  Pad rows / columns and fixed
    cameras exact (their bound is zero); the reduced scalar is the maximum of the two arrays bit for bit."""
    big = name == "pcg_1030"
    b, P = device(name, 0 if big else -1)
    ratios, _ = reduced_ratios(name, b, P, lam_of(b), big)
    assert max(ratios.values()) <= 1, ratios


def test_reduced_system_that_loses_definiteness_is_right_and_flagged():
    """pcg_1030_raw at RAW_LAMBDA_REL: points that start next to a camera make a camera's diagonal block of S cancel
    from 1e13 to lambda ~ 2e3, the relative error of the cofactor Hpp_inv (within its bound in kappa_1 ~ 7e7) decides
    the block's sign, and S is not positive definite.  Every array is still within its derived bound -- S is the right
    function of the device's Hpp_inv --, and k_ba_pcg (nc > 1024) reports it: a pivot of the device's diagonal blocks
    is not positive by the restated elimination either, `fail` is set, and the iteration runs on to its cap with the
    restatement's rel."""
    name = "pcg_1030_raw"
    b, P = device(name, 0)
    lam = C.RAW_LAMBDA_REL * b.debug_reduced(1.0)["maxdiag"]
    ratios, d = reduced_ratios(name, b, P, lam, big=True)
    assert max(ratios.values()) <= 1, ratios
    piv = BR.gj_pivots(d["S"][d["rptr"][:-1]])
    print(f"[ba-op] {name}: smallest pivot of a diagonal block {piv.min():.3e} (lambda {lam:.3e}), "
          f"{int((piv.min(1) <= 0).sum())} block(s) not positive")
    assert np.abs(piv.min()) > 1e-6 * lam  # (a sign the restatement and the device cannot disagree on)
    a = (d["rptr"], d["bcol"], d["S"], d["g"])
    ld, f64 = (BR.block_jacobi_cg(*a, C.PCG_CAP_MAX, C.PCG_REL_TOL, dt) for dt in (LD, np.float64))
    s = b.debug_step(lam, solver=0, pcg_max_iters=C.PCG_CAP_MAX, pcg_rel_tol=C.PCG_REL_TOL)
    assert ld["pivots_ok"] == bool((piv > 0).all()) and s["fail"] == int(ld["fail"]) and s["iters"] == ld["iters"]
    assert measured(name, "rel after 20", s["rel"], f64["rel"], ld["rel"]) <= 1


@pytest.mark.parametrize("name", SOLVE_CASES)
def test_exact_step_and_back_substitution(name):
    """dx_c of the block Cholesky against a long-double solve of the device's S, g (measured); dx_p from the device's
    Hpp_inv, b_p, Z and dx_c (derived, k = 6 m + 3); pads and fixed cameras exactly zero."""
    b, P = device(name)
    lam = lam_of(b)
    d = b.debug_reduced(lam)
    s = b.debug_step(lam, solver=1)
    assert s["fail"] == 0 and s["iters"] == 0
    a = (d["rptr"], d["bcol"], d["S"], d["g"])
    ratio = measured(name, "dx_c (block Cholesky)", s["dx_c"].ravel(), BR.dense_solve(*a, np.float64), BR.dense_solve(*a, LD))
    assert ratio <= 1
    assert (s["dx_c"][:, 6] == 0).all() and (s["dx_c"][P.fixed] == 0).all()
    want, mag, m = BR.backsub(d["Hpp_inv"], d["b_p"], d["Z"], s["dx_c"], P.oc, P.op, LD)
    r = BR.derived_ratio(s["dx_p"], want, mag, BR.k_dxp(m)[:, None])
    print(f"[ba-op] {name}: dx_p error / derived bound {r:.3f}")
    assert r <= 1


# ------------------------------------------------------------------------------------------------ measured
@pytest.mark.parametrize("name", ("lists", "branches", "pcg_17", "tiny"))
def test_linearisation_from_the_estimate(name):
    b, P = device(name)
    lin = b.debug_linearization()
    ld = BR.linearize(P, P.cams, P.points, LD)
    f64 = BR.linearize(P, P.cams, P.points, np.float64)
    _, inl = BR.rho_terms(P, P.cams, P.points, LD)
    if name in ("lists", "pcg_17"):
        assert inl.any() and not inl.all()  # both sides of the Huber kernel
    for what, sl in (("A", slice(0, 12)), ("B", slice(12, 18)), ("es", slice(18, 20))):
        assert measured(name, f"lin {what}", lin[:, sl], f64[:, sl], ld[:, sl]) <= 1


@pytest.mark.parametrize("name", ITERATE_CASES)
def test_pcg_iterates(name):
    """x_k of k_ba_pcg for the caps 1, 2, 5, 20 and its rel against the restated block-Jacobi CG on the device's S, g;
    the returned iteration count is the cap.  (One camera: block-Jacobi is the exact inverse, x_1 is the solution and
    what follows works on its rounding residue; only x_1 is compared there.)"""
    b, P = device(name, 0)
    lam = C.ITERATE_LAMBDA_REL * b.debug_reduced(1.0)["maxdiag"]
    d = b.debug_reduced(lam)
    a = (d["rptr"], d["bcol"], d["S"], d["g"])
    caps = (1,) if name == "pcg_1" else C.ITERATE_CAPS
    assert max(caps) <= C.PCG_CAP_MAX
    ld = BR.block_jacobi_cg(*a, max(caps), C.PCG_REL_TOL, LD)
    f64 = BR.block_jacobi_cg(*a, max(caps), C.PCG_REL_TOL, np.float64)
    assert ld["iters"] == max(caps) and not ld["fail"]
    if name != "pcg_1":
        assert float(ld["rel"]) > C.ITERATE_FLOOR
    for k in caps:
        s = b.debug_step(lam, solver=0, pcg_max_iters=k, pcg_rel_tol=C.PCG_REL_TOL)
        assert s["iters"] == k and s["fail"] == 0
        assert measured(name, f"x_{k}", s["dx_c"].ravel(), f64["x"][k - 1], ld["x"][k - 1]) <= 1
        assert (s["dx_c"][:, 6] == 0).all() and (s["dx_c"][P.fixed] == 0).all()
        if name == "pcg_1":  # rel is the rounding residue of an exact solve there: nothing to compare it with
            continue
        rk = [BR.block_jacobi_cg(*a, k, C.PCG_REL_TOL, dt)["rel"] for dt in (np.float64, LD)] if k < max(caps) else \
            [f64["rel"], ld["rel"]]
        assert measured(name, f"rel after {k}", s["rel"], rk[0], rk[1]) <= 1


def _expected_branch(P, step):
    """carry_<b>: the free cameras of the trace branch land on branch b; back: every free camera on the trace."""
    start = BR.quat_branch(P.cams)
    if step.startswith("carry_"):
        return (start == 3) & ~P.fixed, int(step[-1])
    if step == "back":
        return ~P.fixed, 3
    return None, None


def test_update_for_supplied_steps():
    """k_ba_update on `branches` for the steps of ba_cases.update_steps: cameras (quaternion, translation) and points
    against the long-double update (measured); the chi2 of that estimate (ba_ref.chi2_ratio) and scale = x.(lambda x +
    b) from the device's b_c, b_p (derived, k = n + 3: three roundings per term, n = 7 nc + 3 np terms summed); the
    branch of Eigen's rule every camera took, asserted on the host; fixed cameras bit for bit."""
    b, P = device("branches")
    nc, npt, _ = b.dims()
    lam = lam_of(b)
    d = b.debug_reduced(lam)
    seen, small = set(), set()
    for step, (xc, xp) in C.update_steps(P).items():
        out = b.debug_update(xc, xp, lam)
        ld = BR.update(P.cams, P.points, xc, xp, P.fixed, LD)
        f64 = BR.update(P.cams, P.points, xc, xp, P.fixed, np.float64)
        assert np.array_equal(ld["branch"], f64["branch"]) and np.array_equal(ld["small"], f64["small"])
        who, want = _expected_branch(P, step)
        if who is not None:
            assert who.any() and (ld["branch"][who] == want).all(), (step, ld["branch"])
        seen |= set(ld["branch"][~P.fixed].tolist())
        small |= set(ld["small"][~P.fixed].tolist())
        if step in ("omega0", "below"):  # the exp map's branch of every free camera
            assert ld["small"][~P.fixed].all(), step
        else:
            assert not ld["small"].any(), step
        for what, sl in (("q", slice(0, 4)), ("t", slice(4, 7))):
            assert measured("branches", f"{step} {what}", out["cams"][:, sl], f64["cams"][:, sl], ld["cams"][:, sl]) <= 1
        assert measured("branches", f"{step} points", out["points"], f64["points"], ld["points"]) <= 1
        assert np.array_equal(out["cams"][P.fixed], P.cams[P.fixed])
        r, _ = BR.chi2_ratio(out["chi2"], P, out["cams"], out["points"])
        t, mag = BR.scale_terms(np.concatenate([xc.ravel(), xp.ravel()]),
                                np.concatenate([d["b_c"].ravel(), d["b_p"].ravel()]), lam, LD)
        rs = BR.derived_ratio(out["scale"], t.sum(), mag.sum(), BR.k_sum(t.shape[0], 3))
        print(f"[ba-op] branches {step}: chi2 error / tolerance {r:.3f}, scale error / derived bound {rs:.3f}")
        assert r <= 1 and rs <= 1
    assert seen == {0, 1, 2, 3} and small == {True, False}
    # with the trial's fail flag set nothing moves, and the chi2 is the current estimate's, bit for bit
    xc, xp = C.update_steps(P)["mid"]
    out = b.debug_update(xc, xp, lam, fail=True)
    assert np.array_equal(out["cams"], P.cams) and np.array_equal(out["points"], P.points) and out["chi2"] == b.chi2()
    # and the estimate is where it was
    assert np.array_equal(b.debug_update(np.zeros((nc, 7)), np.zeros((npt, 3)), lam, fail=True)["cams"], P.cams)


def test_update_with_more_cameras_than_point_coordinates():
    b, P = device("tiny")
    nc, npt, _ = b.dims()
    assert nc > 3 * npt
    rng = np.random.default_rng(3)
    xc = np.concatenate([rng.standard_normal((nc, 6)) * 0.1, np.zeros((nc, 1))], axis=1)
    xp = rng.standard_normal((npt, 3)) * 0.1
    out = b.debug_update(xc, xp, 1.0)
    ld, f64 = (BR.update(P.cams, P.points, xc, xp, P.fixed, dt) for dt in (LD, np.float64))
    for what, sl in (("q", slice(0, 4)), ("t", slice(4, 7))):
        assert measured("tiny", f"update {what}", out["cams"][:, sl], f64["cams"][:, sl], ld["cams"][:, sl]) <= 1
    assert measured("tiny", "update points", out["points"], f64["points"], ld["points"]) <= 1


# ------------------------------------------------------------------------------------------------ the large sums
@pytest.mark.parametrize("name", ("big_chi_4", "big_chi_16"))
def test_chi2_of_many_observations(name):
    b, P = device(name, 0)
    r, inl = BR.chi2_ratio(b.chi2(), P, P.cams, P.points)
    print(f"[ba-op] {name}: {inl.shape[0]} observations, {int((~inl).sum())} Huber outliers, chi2 error / tolerance {r:.3f}")
    assert 0.02 * inl.shape[0] < (~inl).sum() < 0.98 * inl.shape[0]
    assert r <= 1


def test_scale_and_update_of_many_points():
    """3 np > 262 144: k_ba_scale's grid-stride loop and the point half of k_ba_update, through the update read-out
    with a supplied step (scale: derived, k = n + 3)."""
    b, P = device("big_scale", 0)
    nc, npt, _ = b.dims()
    lam = lam_of(b)
    d = b.debug_reduced(lam)
    rng = np.random.default_rng(11)
    xc = np.concatenate([rng.standard_normal((nc, 6)) * 1e-3, np.zeros((nc, 1))], axis=1)
    xp = rng.standard_normal((npt, 3)) * 0.05
    out = b.debug_update(xc, xp, lam)
    t, mag = BR.scale_terms(np.concatenate([xc.ravel(), xp.ravel()]),
                            np.concatenate([d["b_c"].ravel(), d["b_p"].ravel()]), lam, LD)
    rs = BR.derived_ratio(out["scale"], t.sum(), mag.sum(), BR.k_sum(t.shape[0], 3))
    ld, f64 = (BR.update(P.cams, P.points, xc, xp, P.fixed, dt) for dt in (LD, np.float64))
    rp = measured("big_scale", "update points", out["points"], f64["points"], ld["points"])
    rc, _ = BR.chi2_ratio(out["chi2"], P, out["cams"], out["points"])
    print(f"[ba-op] big_scale: scale error / derived bound {rs:.3f}, chi2 error / tolerance {rc:.3f}")
    assert rs <= 1 and rp <= 1 and rc <= 1


# ------------------------------------------------------------------------------------------------ exact
def _all_readouts(b, lam, solver):
    nc, npt, _ = b.dims()
    b.debug_pattern()
    b.debug_linearization()
    b.debug_reduced(lam)
    b.debug_step(lam, solver=0, pcg_max_iters=3)  # (leaves a pcg_rel of ~1e-1 behind: must not reach the statistics)
    if solver == 1:
        b.debug_step(lam, solver=1)
    rng = np.random.default_rng(0)
    b.debug_update(rng.standard_normal((nc, 7)) * 0.05, rng.standard_normal((npt, 3)) * 0.05, lam)
    b.debug_update(np.zeros((nc, 7)), np.zeros((npt, 3)), lam, fail=True)


@pytest.mark.parametrize("name,solver", [("branches", 1), ("pcg_17", 0)])
def test_readouts_change_nothing(name, solver):
    """optimize(5) after every read-out, then three times optimize(1) with every read-out in between: cameras, points,
    statistics and iteration counts are those of the same calls without read-outs, bit for bit.  With a plan
    (solver 1) the read-outs ask for the capped PCG as well as the block Cholesky."""
    plain, _ = new_adjuster(name, linear_solver=solver)
    probed, _ = new_adjuster(name, linear_solver=solver)
    lam = 0.37 * lam_of(probed)
    _all_readouts(probed, lam, solver)
    for n in (5, 1, 1, 1):
        assert plain.optimize(n) == probed.optimize(n)
        assert plain.stats() == probed.stats()
        assert np.array_equal(plain.cameras(), probed.cameras()) and np.array_equal(plain.points(), probed.points())
        _all_readouts(probed, lam, solver)
    assert plain.chi2() == probed.chi2()
    plain.close()
    probed.close()


def test_zero_right_hand_side_takes_no_iteration():
    """All cameras fixed: g = 0, so rz_0 = 0: no iteration, rel = 0, dx_c = 0, no fail."""
    b, P = new_adjuster("pcg_16", linear_solver=0)
    b.set_fixed_cameras(np.ones(b.dims()[0], dtype=np.uint8))
    lam = lam_of(b)
    assert (b.debug_reduced(lam)["g"] == 0).all()
    s = b.debug_step(lam, solver=0)
    assert s["iters"] == 0 and s["rel"] == 0 and s["fail"] == 0 and (s["dx_c"] == 0).all()
    b.close()


@pytest.mark.parametrize("solver", [0, 1])
def test_negative_damping_is_flagged_not_a_fault(solver):
    """lambda = -10 max diag makes every free diagonal block of S negative (the Schur term is at most a tenth of the
    camera's own diagonal then): both solvers report `fail`, and a regular step still works afterwards."""
    b, _ = new_adjuster("pcg_16", linear_solver=-1)
    md = b.debug_reduced(1.0)["maxdiag"]
    d = b.debug_reduced(-10.0 * md)
    assert (d["S"][d["rptr"][:-1]].diagonal(0, 1, 2)[:, :6] < 0).all()
    assert b.debug_step(-10.0 * md, solver=solver)["fail"] == 1
    assert b.debug_step(LAMBDA_REL * md, solver=solver)["fail"] == 0
    b.close()


@pytest.mark.parametrize("name", ("pcg_16", "branches"))
def test_indefinite_system_leaves_through_the_pq_test(name):
    """lambda = -min eig(H_pp) / 2 (pcg_16) or / 10 (branches): the point blocks and every diagonal block of S stay
    positive definite (all pivots positive: the `!spd` flag is not what fails), S as a whole is indefinite (its gauge
    directions turn negative), and k_ba_pcg meets p.q <= 0 after some iterations: `fail`, the iteration count and the
    iterate it stopped at are the restated CG's on the device's S."""
    b, P = device(name, 0)
    nc, npt, _ = b.dims()
    H, _, _, _ = BR.point_blocks(b.debug_linearization(), P.op, npt, np.float64)
    lam = -float(np.linalg.eigvalsh(H).min()) / (2 if name == "pcg_16" else 10)
    d = b.debug_reduced(lam)
    a = (d["rptr"], d["bcol"], d["S"], d["g"])
    cap = 20 * nc + 100
    ld, f64 = (BR.block_jacobi_cg(*a, cap, 1e-12, dt) for dt in (LD, np.float64))
    assert ld["pivots_ok"] and ld["fail"] and ld["left"] == "pq" and 0 < ld["iters"] == f64["iters"] < cap
    s = b.debug_step(lam, solver=0, pcg_max_iters=cap, pcg_rel_tol=1e-12)
    print(f"[ba-op] {name}: lambda {lam:.3e}, p.q <= 0 after {ld['iters']} iterations (device {s['iters']})")
    assert s["fail"] == 1 and s["iters"] == ld["iters"]
    assert measured(name, "x at the pq exit", s["dx_c"].ravel(), f64["x_last"], ld["x_last"]) <= 1


def test_refusals():
    lib = L.load()
    b = L.BundleAdjuster(linear_solver=0)
    n = ctypes.c_int32()
    assert lib.sim3opt_ba_debug_pattern(b._b, ctypes.byref(n), None, None) == L.ERR_STATE  # no problem set
    assert b"no problem" in lib.sim3opt_ba_last_error(b._b)
    with pytest.raises(L.Sim3OptError):
        b.debug_linearization()
    b.close()
    b, _ = new_adjuster("tiny", linear_solver=0)
    nc, npt, no = b.dims()
    with pytest.raises(L.Sim3OptError) as e:  # initialised without a plan
        b.debug_step(1.0, solver=1)
    assert e.value.code == L.ERR_STATE and "plan" in str(e.value)
    xc, xp, fl = np.zeros((nc, 7)), np.zeros((npt, 3)), ctypes.c_int32()
    dp = ctypes.POINTER(ctypes.c_double)
    p = lambda a: a.ctypes.data_as(dp)
    assert lib.sim3opt_ba_debug_linearization(b._b, None) == L.ERR_ARG
    assert lib.sim3opt_ba_debug_pattern(b._b, None, None, None) == L.ERR_ARG
    rp = np.zeros(nc + 1, dtype=np.int32)
    assert lib.sim3opt_ba_debug_pattern(b._b, ctypes.byref(n), rp.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), None) == L.ERR_ARG
    assert lib.sim3opt_ba_debug_reduced(b._b, 1.0, *([None] * 9)) == L.ERR_ARG
    assert lib.sim3opt_ba_debug_reduced(b._b, float("nan"), p(np.zeros(49 * n.value or 1)), *([None] * 8)) == L.ERR_ARG
    assert lib.sim3opt_ba_debug_step(b._b, 1.0, 0, 0, 1e-12, None, p(xp), None, None, ctypes.byref(fl)) == L.ERR_ARG
    assert lib.sim3opt_ba_debug_step(b._b, 1.0, 0, 0, 1e-12, p(xc), p(xp), None, None, None) == L.ERR_ARG
    assert lib.sim3opt_ba_debug_step(b._b, 1.0, 2, 0, 1e-12, p(xc), p(xp), None, None, ctypes.byref(fl)) == L.ERR_ARG
    assert lib.sim3opt_ba_debug_update(b._b, None, p(xp), 1.0, 0, p(xc), None, None, None) == L.ERR_ARG
    assert lib.sim3opt_ba_debug_update(b._b, p(xc), p(xp), 1.0, 0, None, None, None, None) == L.ERR_ARG
    assert lib.sim3opt_ba_last_error(b._b)
    assert b.debug_step(1.0, solver=0)["fail"] == 0  # and the handle still works
    b.close()
