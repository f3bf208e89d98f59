"""An independent numpy restatement of the batched PnP RANSAC (sim3opt_pnp_batch, sim3opt_amd/csrc/pnp_batch.hip).

TEST INFRASTRUCTURE ONLY.  PARITY UNPINNED, like the feature: the reference's loopConstraints.txt holds what its
cv::solvePnPRansac runs (kittiDetector.h:1300-1301) returned but not what they were given, and OpenCV's sampling is
not reproducible.  What pins this file is tests/test_pnp_ref.py: planted truth and seeded one-line defects.

What is restated and what is independent of the kernel:
  sampler      the same counter-based rule, written again over Python integers
  P3P          ANOTHER formulation than the kernel's.  The kernel eliminates to a quartic in v = s3 / s1 by a linear
               substitution, solves it in closed form (Ferrari) and gets the rotation from two triangle frames.  Here
               the unknowns are x = s1 / s3, y = s2 / s3; the two conics
                   a^2 (x^2 + 1 - 2 x cos b) = b^2 (y^2 + 1 - 2 y cos a),  c^2 (x^2 + 1 - 2 x cos b) = b^2 (x^2 + y^2 - 2 x y cos g)
               are quadratics in y whose Sylvester resultant is a quartic in x; numpy.roots finds its roots; the pose
               is the absolute orientation of the three points by SVD (Kabsch).
  scoring      z > 0 and squared reprojection error <= reproj_error^2 (OpenCV's criterion); count and sum
  refit        Levenberg-Marquardt in oracle/ba_oracle.py's conventions (VertexSE3Expmap's update, EdgeProjectXYZ2UV's
               error and camera Jacobian, OptimizationAlgorithmLevenberg's damping), the points fixed, no robust kernel;
               ended as well when a step's predicted decrease x.(lambda x + b) is at most 1e-9 of chi2

`defect` switches one statement to a wrong one (tests/test_pnp_ref.py shows that each is noticed).
"""
import numpy as np

from oracle import ba_oracle as BO

M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15
DEFAULTS = dict(iterations=100, reproj_error=3.0, min_inliers=10, min_points=9, refine_iters=10, max_trials=5,
                tau=1e-5, seed=0)
GAIN_TOL = 1e-9  # the refit ends when a step's predicted decrease of chi2 is at most this share of chi2


def splitmix64(x):
    z = (x + GOLD) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def sample(seed, h, n, defect=None):
    """Four distinct indices below n: draw j picks among the n - j left, stepping over the earlier picks in order."""
    picks = []
    for j in range(4):
        i = splitmix64((seed + (4 * h + j + 1) * GOLD) & M64) % (n - j)
        for p in sorted(picks):
            if (p < i) if defect == "sampler_skip" else (p <= i):
                i += 1
        picks.append(i)
    return picks


def project_sqerr(R, t, X, uv, f, cx, cy):
    """(squared reprojection error, depth) of the rows of X under (R, t).  Written out element by element, every
    product and sum rounded on its own in the order the kernel's pnp_sqerr states (which runs without fused
    multiply-add): the same bits per point, so counts compare exactly."""
    X0, X1, X2 = X[:, 0], X[:, 1], X[:, 2]
    x = ((R[0, 0] * X0 + R[0, 1] * X1) + R[0, 2] * X2) + t[0]
    y = ((R[1, 0] * X0 + R[1, 1] * X1) + R[1, 2] * X2) + t[1]
    z = ((R[2, 0] * X0 + R[2, 1] * X1) + R[2, 2] * X2) + t[2]
    with np.errstate(all="ignore"):
        e0 = uv[:, 0] - ((f * x) / z + cx)
        e1 = uv[:, 1] - ((f * y) / z + cy)
    return e0 * e0 + e1 * e1, z


def inliers(R, t, X, uv, f, cx, cy, thr, defect=None):
    e2, z = project_sqerr(R, t, X, uv, f, cx, cy)
    with np.errstate(invalid="ignore"):
        m = (e2 < thr * thr) if defect == "strict_threshold" else (e2 <= thr * thr)
        if defect != "no_depth_test":
            m &= z > 0
    return m, e2


def p3p(X, uv, f, cx, cy):
    """All poses (R, t) that put the three points X (3, 3) on the pixels uv (3, 2) with positive depths."""
    J = np.concatenate([(uv - [cx, cy]) / f, np.ones((3, 1))], axis=1)
    J /= np.linalg.norm(J, axis=1, keepdims=True)
    a2 = ((X[1] - X[2]) ** 2).sum()
    b2 = ((X[0] - X[2]) ** 2).sum()
    c2 = ((X[0] - X[1]) ** 2).sum()
    w = np.cross(X[1] - X[0], X[2] - X[0])
    if min(a2, b2, c2) <= 0.0 or w @ w <= 1e-20 * b2 * c2:
        return []
    ca, cb, cg = J[1] @ J[2], J[0] @ J[2], J[0] @ J[1]
    P = np.poly1d
    base = P([1.0, -2.0 * cb, 1.0])  # x^2 - 2 x cos b + 1
    p2, p1, p0 = P([-b2]), P([2.0 * b2 * ca]), base * float(a2) - float(b2)
    q2, q1, q0 = P([-b2]), P([2.0 * b2 * cg, 0.0]), base * float(c2) - P([float(b2), 0.0, 0.0])
    A, B, Cc = p2 * q0 - p0 * q2, p2 * q1 - p1 * q2, p1 * q0 - p0 * q1
    res = A * A - B * Cc
    if res.order < 1 or not np.all(np.isfinite(res.coeffs)):
        return []
    out = []
    dres = res.deriv()
    for r in np.roots(res.coeffs):
        if abs(r.imag) > 1e-10 * (1.0 + abs(r.real)):
            continue
        x = float(r.real)
        for _ in range(2):  # the eigenvalue, polished on the polynomial
            d = dres(x)
            if d != 0.0:
                x -= res(x) / d
        if not x > 0.0 or B(x) == 0.0:
            continue
        y = -A(x) / B(x)
        if not y > 0.0:
            continue
        s3 = np.sqrt(b2 / base(x))
        Y = np.array([x * s3, y * s3, s3])[:, None] * J
        Xm, Ym = X.mean(0), Y.mean(0)
        U, _, Vt = np.linalg.svd((X - Xm).T @ (Y - Ym))
        D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
        R = Vt.T @ D @ U.T
        t = Ym - R @ Xm
        if np.all(np.isfinite(R)) and np.all(np.isfinite(t)):
            out.append((R, t))
    return out


def hypothesis(X4, uv4, f, cx, cy, defect=None):
    """(valid, R, t, n_solutions): of the P3P solutions of the first three sample points, the one with the smallest
    squared error on the fourth, which must lie in front of the camera."""
    sols = p3p(X4[:3], uv4[:3], f, cx, cy)
    best = None
    for R, t in sols:
        e2, z = project_sqerr(R, t, X4[3:], uv4[3:], f, cx, cy)
        if not (z[0] > 0 and np.isfinite(e2[0])):
            continue
        if best is None or (e2[0] < best[0] and defect != "first_solution"):
            best = (e2[0], R, t)
    if best is None:
        return False, np.eye(3), np.zeros(3), len(sols)
    return True, best[1], best[2], len(sols)


def pose_of(R, t):
    q = BO.R_to_quat(R)
    return np.concatenate([q / np.linalg.norm(q), t])


def hypotheses(X, uv, f, cx, cy, opts, defect=None):
    """Every hypothesis of a problem: dict of sample (H, 4), valid (H,), n_solutions (H,), R (H, 3, 3), t (H, 3),
    e2 (H, n: squared errors, nan where not valid), z (H, n), count (H,), cost (H,)."""
    H, n = opts["iterations"], X.shape[0]
    out = dict(sample=np.zeros((H, 4), dtype=np.int64), valid=np.zeros(H, dtype=bool),
               n_solutions=np.zeros(H, dtype=np.int64), R=np.tile(np.eye(3), (H, 1, 1)), t=np.zeros((H, 3)),
               e2=np.full((H, n), np.nan), z=np.full((H, n), np.nan), count=np.zeros(H, dtype=np.int64),
               cost=np.zeros(H))
    for h in range(H):
        s = sample(opts["seed"], h, n, defect)
        out["sample"][h] = s
        ok, R, t, ns = hypothesis(X[s], uv[s], f, cx, cy, defect)
        out["valid"][h], out["R"][h], out["t"][h], out["n_solutions"][h] = ok, R, t, ns
        if ok:
            m, e2 = inliers(R, t, X, uv, f, cx, cy, opts["reproj_error"], defect)
            out["e2"][h], out["z"][h] = e2, project_sqerr(R, t, X, uv, f, cx, cy)[1]
            out["count"][h], out["cost"][h] = int(m.sum()), float(e2[m].sum())
    return out


def best_hypothesis(hyp, defect=None):
    """largest count, then smallest cost, then smallest index; -1 without a valid one"""
    best = -1
    for h in np.where(hyp["valid"])[0]:
        if best < 0 or hyp["count"][h] > hyp["count"][best] or (
                defect != "tie_ignores_cost" and hyp["count"][h] == hyp["count"][best]
                and hyp["cost"][h] < hyp["cost"][best]):
            best = int(h)
    return best


def camera_jacobian(Xc, f):
    """EdgeProjectXYZ2UV::linearizeOplus, the camera's block over [omega, upsilon] (as ba_oracle.Problem.jacobians)"""
    x, y, z = Xc[:, 0], Xc[:, 1], Xc[:, 2]
    z2 = z * z
    Jc = np.zeros((len(x), 2, 6))
    Jc[:, 0, 0] = x * y / z2 * f; Jc[:, 0, 1] = -(1 + x * x / z2) * f; Jc[:, 0, 2] = y / z * f
    Jc[:, 0, 3] = -1.0 / z * f; Jc[:, 0, 5] = x / z2 * f
    Jc[:, 1, 0] = (1 + y * y / z2) * f; Jc[:, 1, 1] = -x * y / z2 * f; Jc[:, 1, 2] = -x / z * f
    Jc[:, 1, 4] = -1.0 / z * f; Jc[:, 1, 5] = y / z2 * f
    return Jc


def refit(pose, X, uv, mask, f, cx, cy, opts):
    """LM on the six degrees of freedom of pose (7,) over the masked points: dict of pose, trials (list, one entry per
    iteration run), chi2_before, chi2_after."""
    P, obs = X[mask], uv[mask]
    q, t = pose[:4].copy(), pose[4:].copy()

    def resid(q, t):
        Xc = P @ BO.quat_to_R(q).T + t
        return obs - np.stack([f * Xc[:, 0] / Xc[:, 2] + cx, f * Xc[:, 1] / Xc[:, 2] + cy], axis=1), Xc

    e, Xc = resid(q, t)
    chi_cur = chi0 = float((e * e).sum())
    trials, lam = [], None
    for _ in range(opts["refine_iters"]):
        Jc = camera_jacobian(Xc, f)
        Hm = np.einsum("nri,nrj->ij", Jc, Jc)
        b = -np.einsum("nri,nr->i", Jc, e)
        if lam is None:
            lam = opts["tau"] * float(np.abs(np.diag(Hm)).max()) if len(P) else 0.0
        ni, k, rho = 2.0, 0, 0.0
        converged = False
        while True:
            try:
                dx = np.linalg.solve(Hm + lam * np.eye(6), b)
                if float(dx @ (lam * dx + b)) <= GAIN_TOL * chi_cur:  # the step promises nothing: converged
                    converged = True
                    break
                R, tt = BO.se3_exp(dx[None])
                qn = BO.R_to_quat(R[0] @ BO.quat_to_R(q))
                qn /= np.linalg.norm(qn)
                tn = R[0] @ t + tt[0]
                en, Xn = resid(qn, tn)
                chi_new = float((en * en).sum())
                scale = float(dx @ (lam * dx + b)) + 1e-3
            except np.linalg.LinAlgError:
                chi_new, scale = np.inf, 1e-3
            rho = (chi_cur - chi_new) / scale
            if rho > 0 and np.isfinite(chi_new):
                lam *= max(1.0 / 3.0, min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3.0))
                ni = 2.0
                q, t, e, Xc, chi_cur = qn, tn, en, Xn, chi_new
            else:
                lam *= ni
                ni *= 2.0
            k += 1
            if not (rho < 0 and k < opts["max_trials"]):
                break
        if converged and k == 0:
            break
        trials.append(k)
        if converged or k == opts["max_trials"] or rho == 0 or not np.isfinite(lam):
            break
    return dict(pose=np.concatenate([q, t]), trials=trials, chi2_before=chi0, chi2_after=chi_cur)


def solve(X, uv, f, cx, cy, opts, defect=None):
    """One problem: dict of status, pose (7,), mask (n,), n_inliers, rms_px, best, hyp (hypotheses' dict, None for
    status 1), mask_hypothesis, refit (refit's dict or None)."""
    n = X.shape[0]
    ident = np.array([0.0, 0, 0, 1, 0, 0, 0])
    out = dict(status=0, pose=ident, mask=np.zeros(n, dtype=bool), n_inliers=0, rms_px=0.0, best=-1, hyp=None,
               mask_hypothesis=None, refit=None)
    if n < opts["min_points"]:
        out["status"] = 1
        return out
    hyp = out["hyp"] = hypotheses(X, uv, f, cx, cy, opts, defect)
    best = out["best"] = best_hypothesis(hyp, defect)
    if best < 0:
        out["status"] = 2
        return out
    pose = pose_of(hyp["R"][best], hyp["t"][best])
    m, e2 = inliers(BO.quat_to_R(pose[:4]), pose[4:], X, uv, f, cx, cy, opts["reproj_error"], defect)
    out["mask_hypothesis"] = m
    if opts["refine_iters"] > 0:
        use = np.ones(n, dtype=bool) if defect == "refit_all_points" else m
        out["refit"] = refit(pose, X, uv, use, f, cx, cy, opts)
        pose = out["refit"]["pose"]
        m, e2 = inliers(BO.quat_to_R(pose[:4]), pose[4:], X, uv, f, cx, cy, opts["reproj_error"], defect)
    out["pose"], out["mask"], out["n_inliers"] = pose, m, int(m.sum())
    out["rms_px"] = float(np.sqrt(e2[m].sum() / m.sum())) if m.any() else 0.0
    if out["n_inliers"] < opts["min_inliers"]:
        out["status"] = 3
    return out


def median_depth_ratio(point_ptr, depth0, depth1):
    """kittiDetector.h:1305-1311 through numpy.sort"""
    out = []
    for lo, hi in zip(point_ptr[:-1], point_ptr[1:]):
        k = int(0.5 * (hi - lo))
        out.append(np.sort(depth1[lo:hi])[k] / np.sort(depth0[lo:hi])[k])
    return np.array(out)
