"""CPU tests of the dogleg's step rule (csrc/dogleg_rule.hpp through sim3opt_dogleg_rule: the function optimize() calls
per trial) against the long-double restatement of DESIGN.md 5h in tests/algorithms_ref.py, by PROPERTIES with bounds
built from the magnitudes of the quadratic forms: c = alpha b.g - ||h_sd||^2 can cancel completely, so no tolerance
relative to a value would hold.

The bounds.  u = 2^-53; every scalar below is evaluated by a handful of float64 operations on non-negative magnitudes:
  alpha = bb / bHb ............................ 1 rounding
  hsd2 = alpha alpha bb ....................... 4 (two of alpha, two products)
  c = alpha bg - hsd2 ......................... <= 5 u (|alpha bg| + hsd2)
  bma2 = gg - 2 alpha bg + hsd2 ............... <= 6 u (gg + 2 |alpha bg| + hsd2)
  d2 = delta delta - hsd2 ..................... <= 5 u (delta^2 + hsd2)
  beta from these: the form taken adds numbers of one sign (-c and the root for c <= 0, c and the root for c > 0), so
    beta is the exact root of a quadratic whose coefficients are those computed values, times (1 + <= 6 u): the root's
    square, product, sum, square root, the sum with -c or c, the quotient
  ca = (1 - beta) alpha ....................... 3 (alpha, the difference, the product)
The residual ||h_dl||^2 - delta^2 = bma2 beta^2 + 2 c beta - d2 therefore is at most K_RULE u times the sum of the
magnitudes each of these multiplies (norm_bound below), K_RULE = 8 >= every count above; second-order terms are u^2.
linearGain and ||h_dl||^2 as the function returns them are <= 6 roundings on sums of products: K_RULE u x magnitude."""
import numpy as np
import pytest

from sim3opt_amd import lib as L
import algorithms_ref as A
import amg_ref as R
import dogleg_cases as DC

LD, U = R.LD, R.U
pytestmark = pytest.mark.skipif(not R.longdouble_ok(), reason="np.longdouble has no 64-bit mantissa here")
K_RULE = 8


def norm_bound(s, delta, r):
    """K_RULE u x the magnitudes of ||h_dl||^2 - delta^2 as a function of the computed coefficients (module docstring)."""
    bb, bHb, gg, bg = (LD(x) for x in s[:4])
    alpha = bb / bHb
    hsd2, abg = alpha * alpha * bb, abs(alpha * bg)
    beta, ca, cg = LD(r["cg"]), LD(r["ca"]), LD(r["cg"])
    mag = (gg + 2 * abg + hsd2) * beta * beta + 2 * (abg + hsd2) * beta + LD(delta) ** 2 + hsd2
    mag += 2 * ca * ca * bb + 2 * abs(ca * cg * bg)
    return K_RULE * LD(U) * mag


def check_trial(s, delta, r):
    """What holds for every trial: alpha and the norms to their roundings, the returned norm and gain against the
    restated quadratic forms of the RETURNED (ca, cg)."""
    ref = A.dogleg_rule(s, delta)
    # (1, 3 and 1 roundings, and one more u for the long-double reference's own)
    assert abs(LD(r["alpha"]) - ref["alpha"]) <= 2 * LD(U) * abs(ref["alpha"])
    assert abs(LD(r["norm_sd"]) - ref["norm_sd"]) <= 4 * LD(U) * ref["norm_sd"]
    assert abs(LD(r["norm_gn"]) - ref["norm_gn"]) <= 2 * LD(U) * ref["norm_gn"]
    dl2, dl2_mag, gain, gain_mag = A.dogleg_step_model(s, r["ca"], r["cg"])
    assert abs(LD(r["linear_gain"]) - gain) <= K_RULE * LD(U) * gain_mag
    # norm_dl = sqrt(dl2): d(sqrt) = d(dl2) / (2 sqrt), plus the root's own rounding
    nd = np.sqrt(max(dl2, LD(0)))
    assert abs(LD(r["norm_dl"]) ** 2 - dl2) <= K_RULE * LD(U) * dl2_mag + 4 * LD(U) * dl2
    return ref, nd


# ------------------------------------------------------------------------------------------------ the step type
def test_step_type_on_both_sides_of_both_thresholds():
    s = DC.scalars_of([1.0, 0.0], [4.0, 0.5], DC.H2)
    r0 = L.dogleg_rule(s, 1.5)
    nsd, ngn = r0["norm_sd"], r0["norm_gn"]
    assert nsd == 1.0 and ngn == np.sqrt(s[2]) and nsd < ngn
    # ||h_gn|| < delta is Gauss-Newton; ||h_gn|| = delta is not
    up = L.dogleg_rule(s, np.nextafter(ngn, np.inf))
    assert (up["step"], up["ca"], up["cg"]) == (A.STEP_GN, 0.0, 1.0) and up["norm_dl"] == ngn
    at = L.dogleg_rule(s, ngn)
    assert at["step"] == A.STEP_DL
    # ||h_sd|| > delta is steepest descent cut to delta; ||h_sd|| = delta is the dogleg step with beta = 0
    dn = L.dogleg_rule(s, np.nextafter(nsd, 0.0))
    assert dn["step"] == A.STEP_SD and dn["cg"] == 0.0
    assert abs(LD(dn["ca"]) * LD(nsd) - LD(np.nextafter(nsd, 0.0))) <= 3 * LD(U) * nsd  # ||ca b|| = delta
    on = L.dogleg_rule(s, nsd)
    assert on["step"] == A.STEP_DL and on["cg"] == 0.0 and on["ca"] == on["alpha"]
    for delta, r in ((np.nextafter(ngn, np.inf), up), (ngn, at), (np.nextafter(nsd, 0.0), dn), (nsd, on)):
        ref, _ = check_trial(s, delta, r)
        assert ref["step"] == r["step"]


# ------------------------------------------------------------------------------------------------ the dogleg step
@pytest.mark.parametrize("name", DC.RULE_CASES)
def test_dogleg_step_lies_on_the_trust_radius(name):
    s, delta = DC.rule_case(name)
    c = DC.check_rule_case(name, s, delta)
    r = L.dogleg_rule(s, delta)
    ref, nd = check_trial(s, delta, r)
    assert r["step"] == ref["step"] == A.STEP_DL
    beta = r["cg"]
    assert 0.0 <= beta <= 1.0
    dl2 = A.dogleg_step_model(s, r["ca"], r["cg"])[0]
    err, tol = abs(dl2 - LD(delta) ** 2), norm_bound(s, delta, r)
    print(f"[dl-rule] {name:13s} c {c:+.3g} beta {beta:.17g} | ||h_dl||^2 - delta^2 | {float(err):.2e}, bound {float(tol):.2e}")
    assert err <= tol
    # The two forms of the root on the SAME float64 coefficients (so that what is compared is the form, not the
    # cancellation in d2 that both inherit): the exact root of that quadratic in long double, the form taken within
    # its 6 roundings, the form not taken -- useless where it cancels
    bb, bHb, gg, bg = (np.float64(x) for x in s[:4])
    alpha = bb / bHb
    hsd2 = alpha * alpha * bb
    cc, bma2, d2 = alpha * bg - hsd2, gg - 2.0 * alpha * bg + hsd2, np.float64(delta) * np.float64(delta) - hsd2
    rl = np.sqrt(LD(cc) * LD(cc) + LD(bma2) * LD(d2))
    exact = (-LD(cc) + rl) / LD(bma2) if cc <= 0 else LD(d2) / (LD(cc) + rl)
    assert abs(LD(beta) - exact) <= K_RULE * LD(U) * exact
    root = np.sqrt(cc * cc + bma2 * d2)
    with np.errstate(divide="ignore", invalid="ignore"):
        other = d2 / (cc + root) if cc <= 0 else (-cc + root) / bma2
    rel_other = float(abs(LD(other) - exact) / exact) if np.isfinite(other) else np.inf
    print(f"[dl-rule] {name:13s} the other form of the root: relative error {rel_other:.2e}")
    if name.endswith("cancel"):
        assert rel_other > 2.0 ** -26  # more than half of the 53 bits gone


def test_random_dogleg_steps():
    """400 random models in 5 dimensions, delta between the two norms: the properties above, both forms of the root
    (the counts of the two forms are asserted: a property of the generator, not of the rule)."""
    rng = np.random.default_rng(17)
    forms = {True: 0, False: 0}
    worst = 0.0
    for k in range(400):
        M = rng.standard_normal((5, 5))
        H = M @ M.T + 0.1 * np.eye(5)
        b = rng.standard_normal(5) * 10.0 ** rng.uniform(-3, 3)
        if k % 2:  # a perturbed Gauss-Newton solution (c > 0 as a rule) ...
            g = np.linalg.solve(H, b) + rng.standard_normal(5) * 10.0 ** rng.uniform(-6, 0) * np.linalg.norm(b)
        else:      # ... or any vector three times as long as h_sd (an inexact or damped solve: c of either sign)
            g = rng.standard_normal(5)
            g *= 3.0 * (b @ b) / (b @ H @ b) * np.linalg.norm(b) / np.linalg.norm(g)
        s = DC.scalars_of(b, g, H)
        r0 = L.dogleg_rule(s, 1.0)
        lo, hi = sorted((r0["norm_sd"], r0["norm_gn"]))
        if r0["norm_sd"] >= r0["norm_gn"]:
            continue
        delta = lo + (hi - lo) * rng.uniform(0.0, 1.0) ** 3
        r = L.dogleg_rule(s, delta)
        ref, _ = check_trial(s, delta, r)
        if r["step"] != A.STEP_DL:
            continue
        forms[bool(ref["c"] <= 0)] += 1
        assert 0.0 <= r["cg"] <= 1.0
        err = abs(A.dogleg_step_model(s, r["ca"], r["cg"])[0] - LD(delta) ** 2)
        worst = max(worst, float(err / norm_bound(s, delta, r)))
    print(f"[dl-rule] random: {forms[True]} steps with c <= 0, {forms[False]} with c > 0, worst residual / bound {worst:.3f}")
    assert min(forms.values()) >= 20 and worst <= 1.0


# ------------------------------------------------------------------------------------------------ bma2 = 0
def test_gauss_newton_step_equal_to_the_steepest_descent_step_is_recorded_as_it_is():
    """h_gn = h_sd on the trust radius (bma2 = c = d2 = 0): the root is 0 / 0.  DESIGN.md 5h records what the rule
    yields; this pins it (changing it is a decision of its own; g2o's form is the same)."""
    s = np.array([4.0, 2.0, 16.0, 8.0, 4.0, 8.0])  # b.b = 4, alpha = 2, h_gn = 2 b: g.g = 16, b.g = 8; H = I / 2
    with np.errstate(invalid="ignore"):
        ref = A.dogleg_rule(s, 4.0)
    assert ref["norm_sd"] == ref["norm_gn"] == 4.0 and ref["c"] == 0 and ref["bma2"] == 0 and ref["d2"] == 0
    with np.errstate(invalid="ignore"):
        r = L.dogleg_rule(s, 4.0)
    assert r["step"] == A.STEP_DL and np.isnan(r["ca"]) and np.isnan(r["cg"]) and np.isnan(r["linear_gain"])
    assert r["norm_dl"] == 0.0  # sqrt(max(0, NaN)) with std::max's argument order
    # one ulp either side of the radius the rule is sound: the GN step, or the cut SD step
    assert L.dogleg_rule(s, np.nextafter(4.0, 5.0))["step"] == A.STEP_GN
    dn = L.dogleg_rule(s, np.nextafter(4.0, 0.0))
    assert dn["step"] == A.STEP_SD and np.isfinite(dn["ca"])


def test_null_arguments_are_refused():
    assert L.load().sim3opt_dogleg_rule(None, 1.0, None, None, None) == L.ERR_ARG
    assert L.load().sim3opt_version() == 130
