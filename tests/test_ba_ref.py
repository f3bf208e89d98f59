"""CPU tests of tests/ba_ref.py and tests/ba_cases.py, the yardstick and the cases of tests/test_gpu_ba_operators.py:
the restatement against oracle/ba_oracle.py (system(), solve(schur=True), apply, chi2), the path condition of every
case on the restated pattern, the facts the `branches` case was designed for -- and the SENSITIVITY of the comparisons:
every defect of ba_ref.MUTATIONS moves the affected output by at least 1e4 x the tolerance the GPU test applies to it
(the derived bound gamma(k) x magnitude, or 32 x noise).

Nothing here needs a GPU: the float64 restatement stands in for the device."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import ba_oracle as BO
import amg_ref as R
import ba_cases as C
import ba_ref as BR

LD, U = R.LD, R.U
pytestmark = pytest.mark.skipif(not R.longdouble_ok(), reason="np.longdouble has no 64-bit mantissa here")


def pipeline(P, lam, dt, lin=None, mut=None):
    """The restated LM trial up to the reduced system, every stage from the stage before in dt."""
    nc, npt = P.cams.shape[0], P.points.shape[0]
    lin = BR.linearize(P, P.cams, P.points, dt) if lin is None else np.asarray(lin, dtype=dt)
    H, bp, bp_mag, m = BR.point_blocks(lin, P.op, npt, dt)
    Hinv = BR.point_inverse(H, lam, dt)
    Z, _ = BR.z_blocks(lin, Hinv, P.op, dt)
    lists = BR.pair_lists(P.oc, P.op, nc)
    red = BR.reduced_system(lin, Z, bp, P.oc, P.op, lists, P.fixed, lam, dt, mut=mut)
    return dict(lin=lin, H=H, bp=bp, Hinv=Hinv, Z=Z, lists=lists, red=red, m=m)


def lam_of(P, rel):
    H, _, _ = P.system()
    return rel * float(H.diagonal().max())


# ------------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("name", C.CASES)
def test_every_case_meets_its_path_condition_on_the_host(name):
    P = C.problem(name)
    dims = (P.cams.shape[0], P.points.shape[0], P.oc.shape[0])
    if name.startswith("big_chi_"):
        f = C.facts(P, None, None, dims)
    else:
        lists = BR.pair_lists(P.oc, P.op, dims[0])
        f = C.facts(P, lists["rptr"], lists["bcol"], dims)
    print(C.describe(name, f))
    C.check_path(name, f)


def test_pair_lists_against_a_plain_double_loop():
    P = C.problem("lists")
    nc = P.cams.shape[0]
    want = {(c, c): [] for c in range(nc)}
    for p in range(P.points.shape[0]):
        obs = np.flatnonzero(P.op == p)
        for a in obs:
            for b in obs:
                want.setdefault((int(P.oc[a]), int(P.oc[b])), []).append((int(a), int(b)))
    L = BR.pair_lists(P.oc, P.op, nc)
    keys = sorted(want, key=lambda ij: (ij[0], ij[0] != ij[1], ij[1]))
    assert keys == list(zip(L["brow"].tolist(), L["bcol"].tolist()))
    for k, ij in enumerate(keys):
        got = list(zip(L["pa"][L["sptr"][k]:L["sptr"][k + 1]].tolist(), L["pb"][L["sptr"][k]:L["sptr"][k + 1]].tolist()))
        assert got == want[ij], ij  # (the double loop runs in (point, o1, o2) order too)


def test_branches_case_is_what_it_was_designed_for():
    P = C.problem("branches")
    br = BR.quat_branch(P.cams)
    want = np.repeat([C.BRANCH_OF_BASE[n] for n, _, _ in C.BRANCH_BASES], 3)
    assert np.array_equal(br, want) and set(br) == {0, 1, 2, 3}
    assert (P.cams[:, 3] > 0).any() and (P.cams[:, 3] < 0).any()
    H, b, chi = P.system()
    lam = 1e-5 * float(H.diagonal().max())
    full, red = P.solve(H, b, lam), P.solve(H, b, lam, schur=True)
    agree = np.abs(full - red).max() / np.abs(full).max()
    print(f"[ba-ref] branches: full and Schur solves agree to {agree:.1e}")
    assert agree <= 1e-12  # two float64 sparse LU solves; 1.6e-13 observed
    # after a step every camera is still on its branch
    cn, _ = P.apply(P.cams, P.points, full)
    assert np.array_equal(BR.quat_branch(cn), want)
    Q = BO.Problem(P.cams, P.points, P.oc, P.op, P.uv)
    Q.fixed = P.fixed.copy()
    tr = Q.optimize(6)
    print(f"[ba-ref] branches: chi2 {chi:.4g} -> {tr[-1]['chi2']:.4g} in {len(tr)} iterations")
    assert len(tr) == 6 and tr[-1]["chi2"] < 0.006 * chi  # (7.9e4 -> 3.7e2)
    assert np.array_equal(BR.quat_branch(Q.cams), want)


# ------------------------------------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize("name", ["lists", "pcg_16"])
def test_restatement_agrees_with_the_oracle(name):
    P = C.problem(name)
    nc, npt = P.cams.shape[0], P.points.shape[0]
    H, b, chi = P.system()
    lam = 1e-4 * float(H.diagonal().max())
    for dt in (np.float64, LD):
        s = pipeline(P, lam, dt)
        red, L = s["red"], s["lists"]
        rho, _ = BR.rho_terms(P, P.cams, P.points, dt)
        assert abs(float(rho.sum()) - chi) <= 1e-12 * chi
        # the reduced system is the Schur complement of the oracle's H + lam I
        n6 = 6 * nc
        Hl = (H + lam * sp.identity(H.shape[0])).toarray()
        A, Bm, D = Hl[:n6, :n6], Hl[:n6, n6:], Hl[n6:, n6:]
        Sd = A - Bm @ np.linalg.solve(D, Bm.T)
        gd = b[:n6] - Bm @ np.linalg.solve(D, b[n6:])
        fx = np.repeat(P.fixed, 6)  # (the oracle damps its identity rows too: 1 + lam there, 1 here)
        Sd[fx, fx] = 1.0
        S7 = R.dense_of(nc, R._row_of_block(L["rptr"]), L["bcol"], red["S"], dt).reshape(nc, 7, nc, 7)
        assert R.relerr(S7[:, :6, :, :6].reshape(n6, n6), Sd) < 1e-10
        assert (S7[:, 6, :, :6] == 0).all() and (S7[:, :6, :, 6] == 0).all()
        assert np.array_equal(S7[:, 6, :, 6], np.eye(nc))
        assert R.relerr(red["g"][:, :6].ravel(), gd) < 1e-9 and (red["g"][:, 6] == 0).all()
        assert R.relerr(red["b_c"][:, :6].ravel(), b[:n6]) < 1e-12
        free = ~P.fixed
        diagH = H.diagonal()[:n6].reshape(nc, 6)
        assert R.relerr(red["cdmax"][free, :6], diagH[free]) < 1e-12 and (red["cdmax"][~free] == 0).all()
        # the step
        want = P.solve(H, b, lam, schur=True)
        dxc = BR.dense_solve(L["rptr"], L["bcol"], red["S"], red["g"], dt).reshape(nc, 7)
        dxp, _, _ = BR.backsub(s["Hinv"], s["bp"], s["Z"], dxc, P.oc, P.op, dt)
        assert R.relerr(dxc[:, :6].ravel(), want[:n6]) < 1e-8 and R.relerr(dxp.ravel(), want[n6:]) < 1e-8
        assert (dxc[:, 6] == 0).all() and (dxc[P.fixed] == 0).all()
        # the update
        cn, pn = P.apply(P.cams, P.points, want)
        up = BR.update(P.cams, P.points, want[:n6].reshape(nc, 6), want[n6:], P.fixed, dt)
        assert R.relerr(up["cams"], cn) < 1e-13 and R.relerr(up["points"], pn) < 1e-14
        # block-Jacobi CG reaches the same step
        cg = BR.block_jacobi_cg(L["rptr"], L["bcol"], red["S"], red["g"], 20 * nc + 100, 1e-13, dt)
        assert not cg["fail"] and 0 < cg["iters"] < 20 * nc + 100 and cg["rel"] <= 1e-13
        assert R.relerr(cg["x"][-1], dxc.ravel()) < 1e-8


@pytest.mark.parametrize("case", [(65, 24), (257, 19), (65, 24, "z+")])
def test_two_view_trial_agrees_with_the_oracle(case):
    """What the two-view trial adds to this file, against oracle/ba_oracle.py's two-camera Problem with camera 0 fixed:
    chi2 and activeChi2, computeLambdaInit's maximum, the damped S as one 6 x 6 block (the Schur complement of the
    oracle's H + lambda I) with g, the step, the trial estimate with its chi2, and the scale term."""
    import two_view_cases as TC
    c = TC.make_case(*case)
    P = TC.oracle_problem(c, TC.DEFAULTS)
    B = TC.ref_batch(TC.arrays_of([c]))
    H, b, chi = P.system()
    lam = 50.0
    e = P.residuals()
    Hl = (H + lam * sp.identity(H.shape[0])).toarray()[6:, 6:]
    rhs = b[6:]
    A, Bm, D = Hl[:6, :6], Hl[:6, 6:], Hl[6:, 6:]
    dx = np.concatenate([np.zeros(6), np.linalg.solve(Hl, rhs)])
    cn, pn = P.apply(P.cams, P.points, dx)
    for dt in (np.float64, LD):
        t = BR.two_view_trial(B, np.array([lam]), dt)
        s = t["sums"][0]
        assert abs(float(t["chi2"][0]) - chi) <= 1e-12 * chi
        assert abs(float(t["active"][0]) - float(P.omega * (e * e).sum())) <= 1e-12 * float(t["active"][0])
        assert abs(float(t["maxdiag"][0]) - np.abs(H.diagonal()[6:]).max()) <= 1e-12 * float(t["maxdiag"][0])
        assert R.relerr(s["S"], A - Bm @ np.linalg.solve(D, Bm.T)) < 1e-10
        assert R.relerr(s["g"], rhs[:6] - Bm @ np.linalg.solve(D, rhs[6:])) < 1e-9
        assert R.relerr(s["b_c"], rhs[:6]) < 1e-12 and R.relerr(t["rows"]["b_p"].ravel(), rhs[6:]) < 1e-12
        assert R.relerr(s["AtA"], H.toarray()[6:12, 6:12]) < 1e-12
        assert R.relerr(t["dx_c"][0], dx[6:12]) < 1e-8
        assert R.relerr(t["cams"][0], cn[1]) < 1e-9 and R.relerr(t["rows"]["trial_points"], pn) < 1e-9
        assert abs(float(t["chi2_new"][0]) - P.chi2(cn, pn)) <= 1e-7 * chi
        assert abs(float(t["scale"][0]) - float(dx[6:] @ (lam * dx[6:] + rhs))) <= 1e-8 * abs(float(t["scale"][0]))
        assert t["branch"][0] == BR.quat_branch(c["cam1"][None])[0] == (TC.GAUGE_BRANCH[case[2]] if len(case) > 2 else 3)


def test_update_matches_the_oracle_on_every_branch():
    P = C.problem("branches")
    nc = P.cams.shape[0]
    seen, small = set(), set()
    for name, (xc, xp) in C.update_steps(P).items():
        dx = np.concatenate([xc[:, :6].ravel(), xp.ravel()])
        cn, pn = P.apply(P.cams, P.points, dx)
        up = BR.update(P.cams, P.points, xc, xp, P.fixed, np.float64)
        assert R.relerr(up["cams"], cn) < 1e-12 and R.relerr(up["points"], pn) < 1e-15, name
        assert np.array_equal(up["cams"][P.fixed], P.cams[P.fixed])
        seen |= set(up["branch"][~P.fixed].tolist())
        small |= set(up["small"][~P.fixed].tolist())
    assert seen == {0, 1, 2, 3} and small == {True, False}


# ------------------------------------------------------------------------------------------------ sensitivity
def test_sensitivity_of_the_derived_checks():
    """S, g and dx_p of each defective restatement (float64, standing in for the device) against the long-double
    evaluation of the SAME inputs, in units of the derived bound of the GPU test."""
    P = C.problem("lists")
    lam = lam_of(P, 1e-4)
    dev = pipeline(P, lam, np.float64)
    L = dev["lists"]
    nc = P.cams.shape[0]
    ref = BR.reduced_system(dev["lin"], dev["Z"], dev["bp"], P.oc, P.op, L, P.fixed, lam, LD)
    kS = BR.s_counts(ref, L, nc)
    kg = BR.k_g(ref["nd"])[:, None]
    assert BR.derived_ratio(dev["red"]["S"], ref["S"], ref["S_mag"], kS) <= 1
    assert BR.derived_ratio(dev["red"]["g"], ref["g"], ref["g_mag"], kg) <= 1
    moved = {}
    for mut in ("pair_drop", "pair_65_as_1", "damp_offdiag"):
        bad = BR.reduced_system(dev["lin"], dev["Z"], dev["bp"], P.oc, P.op, L, P.fixed, lam, np.float64, mut=mut)
        moved[mut] = BR.derived_ratio(bad["S"], ref["S"], ref["S_mag"], kS)
    bad = BR.reduced_system(dev["lin"], dev["Z"], dev["bp"], P.oc, P.op, L, P.fixed, lam, np.float64, mut="g_no_Zbp")
    moved["g_no_Zbp"] = BR.derived_ratio(bad["g"], ref["g"], ref["g_mag"], kg)
    dxc = BR.dense_solve(L["rptr"], L["bcol"], dev["red"]["S"], dev["red"]["g"], np.float64)
    want, mag, m = BR.backsub(dev["Hinv"], dev["bp"], dev["Z"], dxc, P.oc, P.op, LD)
    good, _, _ = BR.backsub(dev["Hinv"], dev["bp"], dev["Z"], dxc, P.oc, P.op, np.float64)
    kx = BR.k_dxp(m)[:, None]
    assert BR.derived_ratio(good, want, mag, kx) <= 1
    bad, _, _ = BR.backsub(dev["Hinv"], dev["bp"], dev["Z"], dxc, P.oc, P.op, np.float64, mut="backsub_ZT")
    moved["backsub_ZT"] = BR.derived_ratio(bad, want, mag, kx)
    for k, v in moved.items():
        print(f"[ba-ref] lists: {k:14s} moves its output by {v:.2e} x the derived bound")
    assert min(moved.values()) >= 1e4, moved


def test_sensitivity_of_the_update_check():
    """Cameras of the defective update against the long-double update, in units of the GPU test's tolerance (32 x
    |float64 restatement - long double|, floored at 4u; quaternions up to sign, translations, per step)."""
    P = C.problem("branches")
    steps = C.update_steps(P)
    moved = {}
    for mut, names in (("V_half", ["below"]), ("quat_jl_swap", ["carry_0", "carry_1", "carry_2", "near_pi"])):
        for name in names:
            xc, xp = steps[name]
            ld = BR.update(P.cams, P.points, xc, xp, P.fixed, LD)
            f64 = BR.update(P.cams, P.points, xc, xp, P.fixed, np.float64)
            bad = BR.update(P.cams, P.points, xc, xp, P.fixed, np.float64, mut=mut)
            sl = slice(4, 7) if mut == "V_half" else slice(0, 4)
            _, tol = R.noise_and_tol(f64["cams"][:, sl], ld["cams"][:, sl])
            f = R.relerr(bad["cams"][:, sl], ld["cams"][:, sl]) / tol
            if mut == "quat_jl_swap" and not (ld["branch"] < 3).any():
                continue
            moved[mut] = min(moved.get(mut, np.inf), f)
            print(f"[ba-ref] branches {name}: {mut} moves the cameras by {f:.2e} x tolerance")
    assert set(moved) == {"V_half", "quat_jl_swap"} and min(moved.values()) >= 1e4, moved


@pytest.mark.parametrize("name", ["pcg_17", "pcg_147"])
def test_sensitivity_of_the_iterate_check(name):
    """x_k of each defective recurrence against the long-double x_k in units of the GPU test's tolerance.  beta_old_rz
    needs three steps to show (the first beta it changes is the second)."""
    P = C.problem(name)
    lam = lam_of(P, C.ITERATE_LAMBDA_REL)
    s = pipeline(P, lam, np.float64)
    a = (s["lists"]["rptr"], s["lists"]["bcol"], s["red"]["S"], s["red"]["g"])
    kmax = max(C.ITERATE_CAPS)
    ld = BR.block_jacobi_cg(*a, kmax, C.PCG_REL_TOL, LD)
    f64 = BR.block_jacobi_cg(*a, kmax, C.PCG_REL_TOL, np.float64)
    assert ld["iters"] == f64["iters"] == kmax and not ld["fail"]
    assert float(ld["rel"]) > C.ITERATE_FLOOR  # the largest cap still compares an iterate that moves
    print(f"[ba-ref] {name}: rel after {kmax} iterations {float(ld['rel']):.2e}")
    worst = {}
    for mut in ("beta_old_rz", "iter_plus_one"):
        for k in C.ITERATE_CAPS:
            if mut == "beta_old_rz" and k < 3:
                continue
            xm = BR.block_jacobi_cg(*a, k, C.PCG_REL_TOL, np.float64, mut=mut)["x"][-1]
            noise, tol = R.noise_and_tol(f64["x"][k - 1], ld["x"][k - 1])
            f = R.relerr(xm, ld["x"][k - 1]) / tol
            worst[mut] = min(worst.get(mut, np.inf), f)
            print(f"[ba-ref] {name} k {k:2d}: noise {noise:.2e}  {mut:14s} moves x_k by {f:.2e} x tolerance")
    assert min(worst.values()) >= 1e4, worst
