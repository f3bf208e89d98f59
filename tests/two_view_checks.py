"""What a read-out of one two-view LM trial (lib.TwoViewBatch.debug_trial, sim3opt_ba_batch_debug_trial) is held to:
ratios(...) returns error / tolerance per quantity, the worst over the batch.  tests/test_gpu_two_view_operators.py
applies it to the device's read-out; tests/test_two_view_batch.py applies it, without a GPU, to the float64
restatement (which must pass) and to the restatement with one seeded defect (tests/ba_ref.py, TWO_VIEW_MUTATIONS: the
affected quantity must miss its tolerance by a factor of 1e4 or more), so the two files cannot drift apart.

Derived (the inputs are the read-out's own arrays, the operation is sums of products; ba_ref.derived_ratio, gamma(k) x
the expression with absolute values, for any summation order and any FMA contraction; m = 2 observations per point,
n = points of the problem = nd = pairs):
  H_pp, b_p ...... k = 2 m on B_1, es_1 of the read-out; camera 0's share, which the kernel keeps in registers, comes
                   from the estimate in long double, and the tolerance grows by its measured term (32 x |float64 - long
                   double| of that share, floored at 4u of its magnitude)
  Hpp_inv ........ the cofactor inverse's residual bound (ba_ref.inverse_residual_ratio) against the read-out's H_pp
  Z .............. k = 5
  AtA, b_c ....... k = 2 n;  ZY, S: k = 3 n + 2 n + 3;  Zb: k = 3 n + 1;  g: k = 5 n + 1
  maxdiag ........ the maximum of the read-out's diagonals (every point's H_pp, the camera's sum A_1^T A_1), bit for
                   bit: the ratio is 0 or inf
  scale .......... k = (3 n + 6) + 3, the issue's n + 3 with n = 3 n + 6 terms, on delta_p = trial point - point of the
                   read-out (delta_p itself is not among the 56 rows); the one rounding of that sum, u |trial| per
                   coordinate, is carried with the weight |2 lambda delta_p + b_p|
Measured (another formula order, libm, a solve: amg_ref.noise_and_tol per problem, 32 x |float64 restatement - long
double| floored at 4u):
  A1, B1, es1 .... from the estimate;  dx_c: a long-double solve of the read-out's S, g
  cam_q, cam_t ... the exp-map update of camera 1 by the step used;  trial_points: the back-substitution of the
                   read-out's rows
  chi2, active_chi2, chi2_new: gamma(2 n) sum + 32 x the per-term noise (ba_ref.chi2_ratio's rule)
"""
import numpy as np

import amg_ref as R
import ba_ref as BR
import two_view_cases as TC

LD, U = R.LD, R.U
M_OBS = 2


def sym6(v):
    """(.., 6) xx xy xz yy yz zz -> (.., 3, 3)"""
    v = np.asarray(v)
    return v[..., [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(v.shape[:-1] + (3, 3))


def tri21(v):
    """(21,) upper triangle row by row -> (6, 6) symmetric"""
    out = np.zeros((6, 6), dtype=np.asarray(v).dtype)
    out[np.triu_indices(6)] = v
    return out + np.triu(out, 1).T


def upper21(M):
    return np.asarray(M)[np.triu_indices(6)]


def as_readout(trial):
    """A ba_ref.two_view_trial result in the layout of lib.TwoViewBatch.debug_trial (float64)."""
    r, s = trial["rows"], trial["sums"]
    f = lambda a: np.asarray(a, dtype=np.float64)
    pick = [0, 1, 2, 4, 5, 8]
    out = dict(H_pp=f(r["H"]).reshape(-1, 9)[:, pick], b_p=f(r["b_p"]), A1=f(r["A1"]), B1=f(r["B1"]), es1=f(r["es1"]),
               Hpp_inv=f(r["Hinv"]).reshape(-1, 9)[:, pick], Z=f(r["Z"]), trial_points=f(r["trial_points"]))
    for k in ("AtA", "ZY", "S"):
        out[k] = np.stack([upper21(f(x[k])) for x in s])
    for k in ("b_c", "Zb", "g"):
        out[k] = np.stack([f(x[k]) for x in s])
    out.update(chi2=f(trial["chi2"]), active_chi2=f(trial["active"]), maxdiag=f(trial["maxdiag"]),
               dx_c=f(trial["dx_c"]),
               fail=np.zeros(len(s), dtype=bool), cam=f(trial["cams"]), chi2_new=f(trial["chi2_new"]),
               scale=f(trial["scale"]))
    return out


def _measured(dev, f64, ld):
    _, tol = R.noise_and_tol(f64, ld)
    return R.relerr(dev, ld) / tol


def _exact(equal):
    """The ratio of a quantity that has to be exact: 0 when it is, inf -- over any limit -- when it is not."""
    return 0.0 if equal else np.inf


def _sum_ratio(dev, t_ld, t_64):
    """A sum of non-negative terms formed from the estimate: gamma(n) sum + 32 x the per-term noise, floored at 4u."""
    per = np.maximum(np.abs(t_64.astype(LD) - t_ld), 4 * LD(U) * t_ld)
    tol = BR.gamma_k(t_ld.size) * t_ld.sum() + 32 * per.sum()
    err = abs(LD(dev) - t_ld.sum())
    return float(err / tol) if tol > 0 else _exact(err == 0)


def ratios(d, arrays, cams1, points, lam, dx_c=None, opts=TC.DEFAULTS, problems=None):
    """error / tolerance of every quantity of the read-out d of the batch `arrays` at the estimate (cams1, points) --
    the handle's own, bit for bit -- with damping lam (n,) and the supplied camera steps dx_c (n, 6) or None.  dict
    name -> the worst ratio over `problems` (default: all); a failed trial's back-substitution is not looked at."""
    ptr = np.asarray(arrays["point_ptr"], dtype=np.int64)
    n = ptr.shape[0] - 1
    lam = np.broadcast_to(np.asarray(lam, dtype=np.float64), (n,))
    P = TC.ref_batch(arrays, cams1, points, opts)
    lam_pt = lam[P.problem_of]
    rows = {dt: BR.two_view_rows(P, lam_pt, dt) for dt in (LD, np.float64)}
    out = {}

    def worst(name, v):
        out[name] = max(out.get(name, 0.0), float(v))

    Hd, Hi = sym6(d["H_pp"]), sym6(d["Hpp_inv"])
    dev_rows = dict(A1=d["A1"], B1=d["B1"], es1=d["es1"], Z=d["Z"], b_p=d["b_p"], Hinv=Hi)
    B1, es1 = np.asarray(d["B1"], dtype=LD), np.asarray(d["es1"], dtype=LD)
    # H_pp and b_p: camera 0's share from the estimate, camera 1's from the read-out's B_1, es_1
    for name, dev, own, own_mag, c0 in (
            ("H_pp", Hd, np.einsum("nri,nrj->nij", B1, B1), np.einsum("nri,nrj->nij", np.abs(B1), np.abs(B1)), "H0"),
            ("b_p", d["b_p"], -np.einsum("nri,nr->ni", B1, es1), np.einsum("nri,nr->ni", np.abs(B1), np.abs(es1)),
             "bp0")):
        v, mag = rows[LD][c0]
        noise = np.maximum(np.abs(rows[np.float64][c0][0].astype(LD) - v), 4 * LD(U) * mag)
        tol = BR.gamma_k(2 * M_OBS) * (mag + own_mag) + 32 * noise
        err = np.abs(np.asarray(dev, dtype=LD) - (v + own))
        assert (err[tol == 0] == 0).all(), name
        worst(name, (err[tol > 0] / tol[tol > 0]).max())
    Y = np.einsum("nri,nrj->nij", np.asarray(d["A1"], dtype=LD), B1)
    Ya = np.abs(np.einsum("nri,nrj->nij", np.abs(np.asarray(d["A1"], dtype=LD)), np.abs(B1)))
    worst("Z", BR.derived_ratio(d["Z"], Y @ Hi.astype(LD), Ya @ np.abs(Hi).astype(LD), BR.K_Z))

    step = np.asarray(d["dx_c"] if dx_c is None else dx_c, dtype=np.float64).reshape(n, 6)
    back = {dt: BR.two_view_backsub(dev_rows, step[P.problem_of], dt) for dt in (LD, np.float64)}
    full = np.zeros((2 * n, 6))
    full[1::2] = step
    up = {dt: BR.update(P.cams, P.points, full, back[dt][0], P.fixed, dt) for dt in (LD, np.float64)}
    assert np.array_equal(up[LD]["branch"], up[np.float64]["branch"])
    out["branch"], out["small"] = up[LD]["branch"][1::2], up[LD]["small"][1::2]
    # the chi2 terms at the estimate and at the READ-OUT's trial estimate
    trial_cams = P.cams.copy()
    trial_cams[1::2] = d["cam"]
    term = {dt: dict(rho=rows[dt]["rho"], e2=rows[dt]["e2"],
                     new=BR.rho_terms(P, trial_cams, d["trial_points"], dt)[0].reshape(-1, 2))
            for dt in (LD, np.float64)}

    for k in (range(n) if problems is None else problems):
        sl = slice(int(ptr[k]), int(ptr[k + 1]))
        idx = np.arange(sl.start, sl.stop)
        nk = idx.shape[0]
        for name, key in (("A1", "A1"), ("B1", "B1"), ("es1", "es1")):
            worst(name, _measured(d[name][sl], rows[np.float64][key][sl], rows[LD][key][sl]))
        worst("Hpp_inv", BR.inverse_residual_ratio(Hi[sl], Hd[sl], lam[k], np.full(nk, M_OBS))[0])
        s = BR.two_view_sums(dev_rows, idx, lam[k], LD)
        for name, key, kk in (("AtA", "AtA", BR.k_bc(nk)), ("ZY", "ZY", BR.k_S(nk, nk)), ("S", "S", BR.k_S(nk, nk))):
            # (the upper triangles: entry (r, c), r <= c, is the sum of Z's row r times Y's row c, not the mirror's)
            worst(name, BR.derived_ratio(d[name][k], upper21(s[key]), upper21(s[key + "_mag"]), kk))
        for name, kk in (("b_c", BR.k_bc(nk)), ("Zb", 3 * nk + 1), ("g", BR.k_g(nk))):
            worst(name, BR.derived_ratio(d[name][k], s[name], s[name + "_mag"], kk))
        worst("maxdiag", _exact(d["maxdiag"][k] == max(d["H_pp"][sl][:, [0, 3, 5]].max(),
                                                       tri21(d["AtA"][k]).diagonal().max())))
        worst("chi2", _sum_ratio(d["chi2"][k], term[LD]["rho"][sl], term[np.float64]["rho"][sl]))
        worst("active_chi2", _sum_ratio(d["active_chi2"][k], term[LD]["e2"][sl], term[np.float64]["e2"][sl]))
        if d["fail"][k]:
            continue
        Sd, gd = tri21(d["S"][k]), d["g"][k]
        worst("dx_c", _measured(d["dx_c"][k], np.linalg.solve(Sd, gd), BR.refined6(Sd, gd)))
        for name, c in (("cam_q", slice(0, 4)), ("cam_t", slice(4, 7))):
            worst(name, _measured(d["cam"][k, c], up[np.float64]["cams"][2 * k + 1, c], up[LD]["cams"][2 * k + 1, c]))
        worst("trial_points", _measured(d["trial_points"][sl], up[np.float64]["points"][sl], up[LD]["points"][sl]))
        worst("chi2_new", _sum_ratio(d["chi2_new"][k], term[LD]["new"][sl], term[np.float64]["new"][sl]))
        # delta_p is not among the rows; the trial point is fl(p + delta_p), so trial - p (exact in long double) is the
        # device's delta_p up to that one rounding, u |trial| per coordinate, which x.(lambda x + b) carries with the
        # weight |2 lambda delta_p + b_p| (1.01 for the second order)
        trial, bp = np.asarray(d["trial_points"][sl], dtype=LD), np.asarray(d["b_p"][sl], dtype=LD)
        dxp = trial - np.asarray(P.points[sl], dtype=LD)
        sc, mag, terms = BR.two_view_scale(dxp, bp, step[k], d["b_c"][k], lam[k], LD)
        carried = (LD(U) * np.abs(trial) * np.abs(2 * LD(lam[k]) * dxp + bp)).sum()
        tol = BR.gamma_k(BR.k_sum(terms, 3)) * mag + LD(1.01) * carried
        worst("scale", abs(LD(d["scale"][k]) - sc) / tol)
    return out
