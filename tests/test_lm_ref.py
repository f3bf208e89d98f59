"""CPU tests of tests/lm_ref.py and tests/lm_cases.py, the yardstick and the cases of tests/test_gpu_lm_operators.py:
the float64 restatement against oracle/oracle.py (e, the dense H and b at delta = 1e-6, chi2 with Huber) and against the
library's host code (lib.edge_jacobian_host, lib.robustify), what the cases promise from their inputs alone -- and the
SENSITIVITY of the comparisons: every defect of lm_ref.MUTATIONS moves the checked quantity by at least FLOOR x the
tolerance the GPU test applies to it (the derived bound gamma(k) x magnitude, or 32 x noise).

Nothing here needs a GPU: the float64 restatement stands in for the device."""
import numpy as np
import pytest

from oracle import oracle as O
from sim3opt_amd import lib as L
import amg_ref as R
import lm_cases as C
import lm_ref as LR

LD, U = R.LD, R.U
FLOOR = 1e3
pytestmark = pytest.mark.skipif(not R.longdouble_ok(), reason="np.longdouble has no 64-bit mantissa here")


def ends(g):
    return g["meas"], g["states"][g["v0"]], g["states"][g["v1"]]


def hidx_of(g):
    h = np.full(g["fixed"].shape[0], -1)
    h[g["fixed"] == 0] = np.arange(int((g["fixed"] == 0).sum()))
    return h


def oracle_of(g, kernel=0, kdelta=0.0):
    inf = None if g["info"] is None else np.asarray(g["info"]).transpose(0, 2, 1).reshape(-1, 49)
    return O.Graph(g["states"], g["fixed"], g["v0"], g["v1"], g["meas"], info=inf, kernel=kernel, kdelta=kdelta)


# ------------------------------------------------------------------------------------------------ the cases
def test_thresholds_are_the_librarys():
    o = LR.mopts()
    d = L.default_options()
    assert o == dict(eps=d.exp_eps, half=d.small_rot_half, fixb=d.fix_small_angle_b) and o["eps"] == 1e-5
    assert LR.mopts(fix_small_angle_b=1)["fixb"] == 1


@pytest.mark.parametrize("name", C.CASES + ("partials",))
def test_ill_conditioned_share_of_every_case(name):
    """At most 10 % of a case's residuals amplify rounding beyond lm_ref.ILL (from the restatement alone)."""
    g = C.graph(name)
    o = LR.mopts(**g["options"])
    e64, eld = LR.edge_error(*ends(g), o, np.float64), LR.edge_error(*ends(g), o, LD)
    ill = LR.ill_edges(e64, eld)
    print(f"[lm-ref] {name}: {g['v0'].shape[0]} edges, {int(ill.sum())} ill-conditioned residuals")
    assert ill.mean() <= 0.10


@pytest.mark.parametrize("name", ["branches_b0", "branches_b1", "big_e", "info_kernels"])
def test_ill_conditioned_share_of_the_jacobians(name):
    """The edges whose Jacobian the GPU test gauges apart (an ill-conditioned residual, or restatement noise above
    lm_ref.ill_level: a perturbed residual across a branch threshold) stay below 10 % in every mode the case runs in."""
    g = C.graph(name)
    o = LR.mopts(**g["options"])
    for mode, delta in (("numeric", 1e-9), ("numeric", 1e-6), ("analytic", 0.0)):
        if mode == "analytic" and name == "branches_b0":
            continue  # (the closed form refuses the as-written B)
        oo = dict(o, fixb=1) if mode == "analytic" else o
        f = (lambda dt: LR.analytic_jacobian(*ends(g), oo, 127, dt)) if mode == "analytic" else (
            lambda dt: LR.numeric_jacobian(*ends(g), oo, delta, 127, dt))
        J64, Jl = f(np.float64), f(LD)
        r = LR.measured_ratio(J64[:, :14], J64[:, :14], Jl[:, :14], LR.ill_edges(J64[:, 14], Jl[:, 14]),
                              ill_above=LR.ill_level(mode, delta))
        print(f"[lm-ref] {name} {mode} {delta:g}: J noise {r['noise']:.2e}; {r['n_ill']} of {J64.shape[0]} edges apart, "
              f"noise {r['noise_ill']:.2e}")
        assert r["n_ill"] <= 0.10 * J64.shape[0]


@pytest.mark.parametrize("name", ["kernels", "info_kernels", "dof_0x78"])
def test_kernel_cases_have_every_kind_on_both_sides(name):
    g = C.graph(name)
    o = LR.mopts(**g["options"])
    chi, rho, w = LR.chi_rho_w(LR.edge_error(*ends(g), o, LD), g["info"], g["kinds"], g["deltas"], LD)
    for kind in range(1, 10):
        sel = g["kinds"] == kind
        assert (sel & g["above"]).any() and (sel & ~g["above"]).any(), kind
    thr = np.where(np.isin(g["kinds"], (4, 9)), g["deltas"], g["deltas"] ** 2)
    k = g["kinds"] > 0
    assert (chi[k & g["above"]] > 2 * thr[k & g["above"]]).all() and (chi[k & ~g["above"]] < thr[k & ~g["above"]] / 2).all()
    tukey = (g["kinds"] == LR.KINDS["TUKEY"]) & g["above"]
    assert tukey.any() and (w[tukey] == 0).all() and (w[~tukey & (g["kinds"] != LR.KINDS["SATURATED"])] > 0).all()
    assert (g["kinds"] == 0).any()


@pytest.mark.parametrize("fixb", [0, 1])
def test_branches_case_reaches_every_branch(fixb):
    g = C.graph(f"branches_b{fixb}")
    o = LR.mopts(**g["options"])
    assert o["fixb"] == fixb
    e = LR.edge_error(*ends(g), o, LD)
    small_th, small_sg = LR.log_branch(e, o)
    seen = set(zip(small_th.tolist(), small_sg.tolist()))
    assert seen == {(False, False), (False, True), (True, False), (True, True)}
    assert (g["states"][:, 3] < 0).any() and (g["states"][:, 3] > 0).any()
    assert (g["states"][g["v0"], 3] < 0).any() and (g["states"][g["v1"], 3] < 0).any()


def test_big_e_case_is_what_it_was_designed_for():
    g = C.graph("big_e")
    n = np.linalg.norm(LR.edge_error(*ends(g), LR.mopts(), LD).astype(np.float64), axis=1)
    print(f"[lm-ref] big_e: |e| from {n.min():.1e} to {n.max():.1e}")
    assert n.max() > 100 and (n < 1e-12).sum() > 100


# ------------------------------------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize("name", ["fixed_ends", "parallel", "info", "branches_b0", "branches_b1"])
def test_residuals_agree_with_the_oracle(name):
    g = C.graph(name)
    o = LR.mopts(**g["options"])
    e = LR.edge_error(*ends(g), o, np.float64)
    eo = oracle_of(g).errors(O.default_options(fix_small_angle_b=o["fixb"]))
    ill = LR.ill_edges(e, LR.edge_error(*ends(g), o, LD))
    assert np.abs(e - eo)[~ill].max() < 1e-12 * (1 + np.abs(eo).max())
    assert np.abs(e - eo).max() < 1e-5 * (1 + np.abs(eo).max())  # (the bound of test_residuals_all_branches)


@pytest.mark.parametrize("name,kernel", [("fixed_ends", 0), ("parallel", 0), ("info", 0), ("info", 1), ("dof_0x78", 0)])
def test_dense_system_agrees_with_the_oracle(name, kernel):
    g = C.graph(name)
    o = LR.mopts(**g["options"])
    mask = g["options"].get("dof_mask", 127)
    J = LR.numeric_jacobian(*ends(g), o, 1e-6, mask, np.float64)
    kd = 0.5
    kinds = None if not kernel else np.full(g["v0"].shape[0], kernel)
    chi, rho, w = LR.chi_rho_w(J[:, 14], g["info"], kinds, None if not kernel else np.full(kinds.shape, kd), np.float64)
    G, _ = LR.gram(J, w, g["info"], np.float64)
    nb = int((g["fixed"] == 0).sum())
    H, b = LR.dense_system(G, g["v0"], g["v1"], hidx_of(g), nb, np.float64)
    OG = oracle_of(g, kernel, kd)
    oo = O.default_options(fd_delta=1e-6, dof_mask=mask)
    Ho, bo = OG.build_dense(oo)
    assert abs(rho.sum() - OG.chi2(oo)) <= 1e-12 * rho.sum()
    assert np.abs(H - Ho).max() < 1e-7 * np.abs(Ho).max()  # (the oracle differentiates numerically itself)
    assert np.abs(b - bo).max() < 1e-7 * max(1.0, np.abs(bo).max())
    if kernel:
        assert (w < 1).any() and (w == 1).any()


def test_closed_form_jacobian_agrees_with_the_host_code():
    g = C.graph("branches_b1")
    o = LR.mopts(**g["options"])
    for mask in (127, 0x78):
        J = LR.analytic_jacobian(*ends(g), o, mask, np.float64)
        worst = 0.0
        for k in range(0, g["v0"].shape[0], 5):
            e, Jh = L.edge_jacobian_host(g["meas"][k], g["states"][g["v0"][k]], g["states"][g["v1"][k]], dof_mask=mask)
            worst = max(worst, np.abs(Jh.T - J[k, :14]).max() / np.abs(Jh).max())
            assert np.array_equal(Jh.T == 0, J[k, :14] == 0) or mask == 127
        print(f"[lm-ref] closed form against the host code, dof_mask {mask:#x}: {worst:.1e}")
        assert worst < 1e-12


def test_robustify_agrees_with_the_host_code():
    worst = 0.0
    for kind in range(10):
        for delta in (0.3, 2.0):
            for e2 in (0.0, 0.01, delta * delta * 0.999, delta * 0.999, delta, delta * delta, delta * delta * 1.001, 50.0):
                rho, w = LR.robustify(np.array([kind]), np.array([delta]), np.array([e2]), np.float64)
                rh, wh = L.robustify(kind, delta, e2)
                worst = max(worst, abs(rho[0] - rh) / max(1.0, abs(rh)), abs(w[0] - wh))
    assert worst < 1e-15


# ------------------------------------------------------------------------------------------------ sensitivity
def _moved_derived():
    """Defects of the Gram phase, the stores and the reductions, in units of the derived bound."""
    g = C.graph("info_kernels")
    o = LR.mopts(**g["options"])
    J = LR.numeric_jacobian(*ends(g), o, 1e-6, 127, np.float64)
    _, _, w = LR.chi_rho_w(J[:, 14], g["info"], g["kinds"], g["deltas"], np.float64)
    Gl, Gm = LR.gram(J, w, g["info"], LD)
    G64, _ = LR.gram(J, w, g["info"], np.float64)
    ref, mag, good = LR.edge_stores(Gl), LR.edge_stores(Gm), LR.edge_stores(G64)
    k = LR.K_GRAM_INFO
    names = ("H01", "H10", "s0", "s1")
    for i in range(4):
        assert LR.derived_ratio(good[i], ref[i], mag[i], k) <= 1, names[i]
    moved = {}
    live = w > 0  # (a rejected edge stores zeros whatever the map)

    def worst(bad):
        return min(LR.derived_ratio(np.asarray(bad[i])[live], ref[i][live], mag[i][live], k)
                   for i in range(4) if not np.array_equal(np.asarray(bad[i])[live], good[i][live]))

    for mut in ("h10_untransposed", "inc_swapped", "tri_off_by_one"):
        moved[mut] = worst(LR.edge_stores(G64, mut))
    for mut in ("b_sign", "w_twice"):
        sel = live & (w != 1) if mut == "w_twice" else live
        bad = LR.edge_stores(LR.gram(J, w, g["info"], np.float64, mut)[0])
        moved[mut] = min(LR.derived_ratio(bad[i][sel], ref[i][sel], mag[i][sel], k) for i in (2, 3))
    # the reductions, on a row with many incidences
    p = C.graph("parallel")
    Jp = LR.numeric_jacobian(*ends(p), LR.mopts(), 1e-6, 127, np.float64)
    Gp, _ = LR.gram(Jp, np.ones(Jp.shape[0]), None, np.float64)
    _, _, s0, s1 = LR.edge_stores(Gp)
    h = hidx_of(p)
    rows = np.concatenate([h[p["v0"]], h[p["v1"]]])
    sc = np.concatenate([s0, s1])[rows >= 0]
    order = np.argsort(rows[rows >= 0], kind="stable")
    sc = sc[order]
    incptr = np.concatenate([[0], np.cumsum(np.bincount(rows[rows >= 0], minlength=h.max() + 1))])
    want, wmag, cnt = LR.row_sums(sc, incptr, LD)
    got, _, _ = LR.row_sums(sc, incptr, np.float64)
    kr = LR.k_row(cnt)[:, None]
    assert LR.derived_ratio(got, want, wmag, kr) <= 1
    bad, _, _ = LR.row_sums(sc, incptr, np.float64, "inc_dropped")
    many = cnt > 1
    moved["inc_dropped"] = LR.derived_ratio(bad[many][:, :28], want[many][:, :28], wmag[many][:, :28], kr[many])
    # lambda_0's input: an exact check; the defect in units of one rounding of the value
    D, b = LR.diag_block(got)
    tr, trm, mx = LR.trace_and_max(D, np.float64)
    assert mx == np.abs(np.diagonal(D, axis1=1, axis2=2)).max()
    _, _, mx_bad = LR.trace_and_max(D, np.float64, "max_over_H")
    moved["max_over_H"] = abs(mx_bad - mx) / (U * mx)
    # the scale
    rng = np.random.default_rng(5)
    x = rng.standard_normal(b.size) * 0.01
    lam = 1e-3 * mx
    want, wm = LR.scale_terms(x, b.ravel(), lam, LD)
    got, _ = LR.scale_terms(x, b.ravel(), lam, np.float64)
    ks = LR.k_sum(b.size, LR.K_SCALE_TERM)
    assert LR.derived_ratio(got, want, wm, ks) <= 1
    moved["scale_no_lambda"] = LR.derived_ratio(LR.scale_terms(x, b.ravel(), lam, np.float64, "scale_no_lambda")[0], want, wm, ks)
    return moved


def _moved_measured():
    """Defects of the Jacobians, the weight and the update, in units of 32 x noise (lm_ref.measured_ratio)."""
    moved = {}
    g = C.graph("dof_0x78")
    o = LR.mopts(**g["options"])
    eld = LR.edge_error(*ends(g), o, LD)
    ill = LR.ill_edges(LR.edge_error(*ends(g), o, np.float64), eld)
    for delta in (1e-9, 1e-6):
        for mask, muts in ((0x78, ("frozen_nonzero",)), (127, ("right_perturbation", "delta_swapped", "half_factor"))):
            Jl = LR.numeric_jacobian(*ends(g), o, delta, mask, LD)[:, :14]
            J64 = LR.numeric_jacobian(*ends(g), o, delta, mask, np.float64)[:, :14]
            for mut in muts:
                bad = LR.numeric_jacobian(*ends(g), o, delta, mask, np.float64, mut)[:, :14]
                r = LR.measured_ratio(bad, J64, Jl, ill)
                print(f"[lm-ref] dof_0x78 delta {delta:g}: noise {r['noise']:.2e}  {mut:18s} moves J by {r['ratio']:.2e} x tolerance")
                moved[mut] = min(moved.get(mut, np.inf), r["ratio"])
    chi_l, rho_l, w_l = LR.chi_rho_w(eld, g["info"], g["kinds"], g["deltas"], LD)
    e64 = LR.edge_error(*ends(g), o, np.float64)
    _, _, w64 = LR.chi_rho_w(e64, g["info"], g["kinds"], g["deltas"], np.float64)
    _, _, wbad = LR.chi_rho_w(e64, g["info"], g["kinds"], g["deltas"], np.float64, "w_from_ee")
    moved["w_from_ee"] = LR.measured_ratio(wbad[:, None], w64[:, None], w_l[:, None], ill, floor=1.0)["ratio"]
    h = hidx_of(g)
    x = np.random.default_rng(6).standard_normal(7 * (h.max() + 1)) * 0.2
    Sl, S64 = LR.oplus(g["states"], x, h, o, LD), LR.oplus(g["states"], x, h, o, np.float64)
    bad = LR.oplus(g["states"], x, h, o, np.float64, "oplus_right")
    none = np.zeros(g["states"].shape[0], dtype=bool)
    moved["oplus_right"] = LR.measured_ratio(bad, S64, Sl, none)["ratio"]
    return moved


def test_every_seeded_defect_is_far_above_the_tolerance():
    moved = dict(_moved_derived())
    moved.update(_moved_measured())
    for k in LR.MUTATIONS:
        print(f"[lm-ref] {k:20s} moves its output by {moved[k]:.2e} x the tolerance of the GPU test")
    assert set(moved) == set(LR.MUTATIONS)
    # max_over_H cannot reach the floor, and no test can see it: a diagonal block is a sum of Gram matrices w A^T Omega A,
    # positive semi-definite, so |H_ij| <= sqrt(H_ii H_jj) <= max H_dd -- the maximum over the block IS the maximum over
    # its diagonal.  It stays in the list as a record; the floor holds for the thirteen others.
    assert moved.pop("max_over_H") == 0.0
    print(f"[lm-ref] smallest multiple of the {len(moved)} visible defects: {min(moved.values()):.2e}")
    assert len(moved) >= 10 and min(moved.values()) >= FLOOR, moved
