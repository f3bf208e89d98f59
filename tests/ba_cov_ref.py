"""References of the bundle-adjustment covariances (include/sim3opt.h, sim3opt_ba_covariances), in long double.

  Definition ... Sigma = (H + lam I)^-1 of the dense normal matrix of oracle/ba_oracle.py's Problem.system(), the
                 fixed cameras' rows removed, inverted in long double (a float64 inverse refined by Newton steps whose
                 residuals are formed in long double), with the comparison rule of the tests: the diagonally
                 equilibrated blocks and their bound.
  restate ...... the Schur route the device takes, restated in long double from the per-observation Jacobians: H_pp^-1,
                 Z, the reduced camera system S in 7 x 7 blocks with a unit pad, its inverse kept as the lower triangle
                 of blocks, the sums over a point's ordered observation pairs.  It takes one named defect, each a
                 one-line mistake such an implementation can make; tests/test_ba_cov_ref.py shows that the comparison
                 rule notices every one of them.
"""
import numpy as np

LD = np.longdouble
EPS = np.finfo(float).eps
DEFECTS = ("fixed_not_masked", "upper_not_transposed", "diag_terms_dropped", "hpp_inv_dropped", "cross_sign",
           "lambda_not_on_points", "pad_leak", "unordered_pairs_only")


def inverse_ld(A):
    """A^-1 of a symmetric positive definite matrix (float64 or long double), in long double.  The matrix is scaled to
    a unit diagonal in long double, its float64 inverse X0 refined by X <- X + X0 (I - A X): the residual is formed in
    long double (row by row over A's non-zeros), the correction -- tiny -- goes through float64.  What is left is the
    rounding of the last residual, eps_ld cond(A) relative: ten decades inside the comparison rule's bound."""
    A = np.asarray(A, dtype=LD)
    n = A.shape[0]
    d = np.sqrt(np.diag(A))
    At = A / np.outer(d, d)
    X0 = np.linalg.inv(At.astype(np.float64))
    X = X0.astype(LD)
    nz = [np.flatnonzero(At[i]) for i in range(n)]

    def residual(X):
        R = np.zeros((n, n), dtype=LD)
        for i in range(n):
            R[i] = -(At[i, nz[i]] @ X[nz[i]])
            R[i, i] += 1
        return R

    first = None
    for _ in range(3):
        R = residual(X)
        first = float(np.abs(R).max()) if first is None else first
        X = X + (X0 @ R.astype(np.float64)).astype(LD)
    last = float(np.abs(residual(X)).max())
    assert last < 1e-12 and last <= first, (first, last)
    return (X + X.T) / 2 / np.outer(d, d)


class Definition:
    """Sigma of a problem at lam, the scaling d = sqrt(diag(H + lam I)) and the bound of the comparison rule."""

    def __init__(self, P, lam):
        H, _, _ = P.system()
        nc, npt = P.cams.shape[0], P.points.shape[0]
        self.nc, self.npt = nc, npt
        self.fixed = np.asarray(P.fixed, dtype=bool)
        keep = np.ones(6 * nc + 3 * npt, dtype=bool)
        keep[(6 * np.flatnonzero(self.fixed)[:, None] + np.arange(6)).ravel()] = False
        A = H.toarray()[np.ix_(keep, keep)] + lam * np.eye(int(keep.sum()))
        self.n = A.shape[0]
        row = np.full(keep.shape[0], -1)
        row[keep] = np.arange(self.n)
        self.cam_rows = [row[6 * c:6 * c + 6] for c in range(nc)]       # (-1: fixed)
        self.pt_rows = [row[6 * nc + 3 * p:6 * nc + 3 * p + 3] for p in range(npt)]
        self.d = np.sqrt(np.diag(A))
        Ht = A / np.outer(self.d, self.d)
        ev = np.linalg.eigvalsh(Ht)
        self.cond = float(ev[-1] / ev[0])
        self.bound = max(1e-10, 1e3 * self.n * EPS * self.cond)
        self.Sigma = inverse_ld(A)
        self.St = self.Sigma * np.outer(self.d, self.d).astype(LD)

    def rows(self, kind, i):
        return self.cam_rows[i] if kind == "c" else self.pt_rows[i]

    def block(self, ka, a, kb, b):
        """Sigma's block in long double, zeros where a fixed camera is involved"""
        ra, rb = self.rows(ka, a), self.rows(kb, b)
        if ra[0] < 0 or rb[0] < 0:
            return np.zeros((len(ra), len(rb)), dtype=LD)
        return self.Sigma[np.ix_(ra, rb)]

    def ratio(self, ka, a, kb, b, M):
        """max |S~_M - S~_ref| over the block / (bound sqrt(m_a m_b)); a block with a fixed camera must be exactly +0"""
        ra, rb = self.rows(ka, a), self.rows(kb, b)
        M = np.asarray(M)
        if ra[0] < 0 or rb[0] < 0:
            return 0.0 if (not M.any() and not np.signbit(M).any()) else np.inf
        if not np.isfinite(np.asarray(M, dtype=np.float64)).all():
            return np.inf
        ref = self.St[np.ix_(ra, rb)]
        dev = M.astype(LD) * np.outer(self.d[ra], self.d[rb]).astype(LD)
        ma, mb = self.St[ra, ra].max(), self.St[rb, rb].max()
        return float(np.abs(dev - ref).max() / (self.bound * np.sqrt(ma * mb)))

    def worst(self, cam_pairs, cc, points, pp, point_cams, pc):
        """the largest ratio over a whole answer (arrays as BundleAdjuster.covariances returns them)"""
        w = 0.0
        for (a, b), M in zip(cam_pairs, cc):
            w = max(w, self.ratio("c", a, "c", b, M))
        for p, M in zip(points, pp):
            w = max(w, self.ratio("p", p, "p", p, M))
        for (p, c), M in zip(point_cams, pc):
            w = max(w, self.ratio("p", p, "c", c, M))
        return w


def _inv3(M):
    """inverse of (n, 3, 3) symmetric matrices by cofactors, in long double"""
    a, b, c, d, e, f = M[:, 0, 0], M[:, 0, 1], M[:, 0, 2], M[:, 1, 1], M[:, 1, 2], M[:, 2, 2]
    c00, c01, c02 = d * f - e * e, c * e - b * f, b * e - c * d
    c11, c12, c22 = a * f - c * c, b * c - a * e, a * d - b * b
    det = a * c00 + b * c01 + c * c02
    out = np.empty_like(M)
    out[:, 0, 0], out[:, 0, 1], out[:, 0, 2] = c00, c01, c02
    out[:, 1, 0], out[:, 1, 1], out[:, 1, 2] = c01, c11, c12
    out[:, 2, 0], out[:, 2, 1], out[:, 2, 2] = c02, c12, c22
    return out / det[:, None, None]


def restate(P, lam, cam_pairs, points, point_cams, defect=None):
    """(cc, pp, pc) for the requests, by the Schur route, in long double; `defect`: one of DEFECTS, or None."""
    assert defect is None or defect in DEFECTS
    nc, npt = P.cams.shape[0], P.points.shape[0]
    fixed = np.asarray(P.fixed, dtype=bool)
    Jp, Jc = P.jacobians()
    _, w = P.robust(P.residuals())
    sw = np.sqrt(w * P.omega).astype(LD)
    A = Jc.astype(LD) * sw[:, None, None]   # (no, 2, 6)
    B = Jp.astype(LD) * sw[:, None, None]   # (no, 2, 3)
    lam = LD(lam)
    obs_of = [np.flatnonzero(P.op == p) for p in range(npt)]  # ascending: the device's list order
    Hpp = np.zeros((npt, 3, 3), dtype=LD)
    np.add.at(Hpp, P.op, np.einsum("nri,nrj->nij", B, B))
    Hpp += (LD(0) if defect == "lambda_not_on_points" else lam) * np.eye(3, dtype=LD)
    Hinv = _inv3(Hpp)
    Y = np.einsum("nri,nrj->nij", A, B)               # (no, 6, 3)
    Z = np.einsum("nij,njk->nik", Y, Hinv[P.op])      # (no, 6, 3)
    # the reduced camera system in 7 x 7 blocks, a fixed camera an identity row, the pad a one
    S = np.zeros((7 * nc, 7 * nc), dtype=LD)
    for c in range(nc):
        S[7 * c + 6, 7 * c + 6] = 1
        if fixed[c]:
            S[7 * c:7 * c + 6, 7 * c:7 * c + 6] = np.eye(6, dtype=LD)
    for o in range(len(P.oc)):
        c = P.oc[o]
        if not fixed[c]:
            S[7 * c:7 * c + 6, 7 * c:7 * c + 6] += A[o].T @ A[o]
    for c in np.flatnonzero(~fixed):
        S[7 * c:7 * c + 6, 7 * c:7 * c + 6] += lam * np.eye(6, dtype=LD)
    for p in range(npt):
        for a in obs_of[p]:
            for b in obs_of[p]:
                ca, cb = P.oc[a], P.oc[b]
                if not fixed[ca] and not fixed[cb]:
                    S[7 * ca:7 * ca + 6, 7 * cb:7 * cb + 6] -= Z[a] @ Y[b].T
    Zs = inverse_ld(S)
    # the inverse is kept as the lower triangle of blocks
    lower = {(i, j): Zs[7 * i:7 * i + 7, 7 * j:7 * j + 7] for i in range(nc) for j in range(i + 1)}
    lo, hi = (1, 7) if defect == "pad_leak" else (0, 6)

    def sigma_cc(a, b):
        if (fixed[a] or fixed[b]) and defect != "fixed_not_masked":
            return np.zeros((6, 6), dtype=LD)
        blk = lower[(a, b)] if a >= b else (lower[(b, a)] if defect == "upper_not_transposed" else lower[(b, a)].T)
        return blk[lo:hi, lo:hi]

    cc = np.stack([sigma_cc(a, b) for a, b in cam_pairs]) if len(cam_pairs) else np.zeros((0, 6, 6), dtype=LD)
    pp = np.zeros((len(points), 3, 3), dtype=LD)
    for q, p in enumerate(points):
        M = np.zeros((3, 3), dtype=LD)
        for ia, a in enumerate(obs_of[p]):
            for ib, b in enumerate(obs_of[p]):
                if defect == "diag_terms_dropped" and ia == ib:
                    continue
                if defect == "unordered_pairs_only" and ib < ia:
                    continue
                M += Z[a].T @ sigma_cc(P.oc[a], P.oc[b]) @ Z[b]
        if defect != "hpp_inv_dropped":
            M += Hinv[p]
        pp[q] = (M + M.T) / 2
    pc = np.zeros((len(point_cams), 3, 6), dtype=LD)
    for q, (p, c) in enumerate(point_cams):
        if fixed[c]:
            continue
        M = np.zeros((3, 6), dtype=LD)
        for a in obs_of[p]:
            M += Z[a].T @ sigma_cc(P.oc[a], c)
        pc[q] = M if defect == "cross_sign" else -M
    return cc, pp, pc


def point_pivot_fails(P, lam):
    """The points whose H_pp + lam I fails the header's pivot test: the 3 x 3 LDL^T in x, y, z order, a pivot <= 1e-13
    x the point's largest undamped diagonal entry, or <= 0 (float64, as the device)."""
    Jp, _ = P.jacobians()
    _, w = P.robust(P.residuals())
    B = Jp * np.sqrt(w * P.omega)[:, None, None]
    H = np.zeros((P.points.shape[0], 3, 3))
    np.add.at(H, P.op, np.einsum("nri,nrj->nij", B, B))
    bad = []
    for p, M in enumerate(H):
        thr = 1e-13 * max(M[0, 0], M[1, 1], M[2, 2])
        M = M + lam * np.eye(3)
        d0 = M[0, 0]
        with np.errstate(all="ignore"):
            l10, l20 = M[0, 1] / d0, M[0, 2] / d0
            d1 = M[1, 1] - l10 * M[0, 1]
            l21 = (M[1, 2] - l20 * M[0, 1]) / d1
            d2 = M[2, 2] - l20 * M[0, 2] - l21 * l21 * d1
        if not all(d > thr and d > 0 for d in (d0, d1, d2)):
            bad.append(p)
    return bad
