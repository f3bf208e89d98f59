"""Plain numpy restatement of the bundle-adjustment pipeline of sim3opt_amd/csrc/ba.hip -- linearisation, point blocks,
Z, the pair lists and the reduced camera system, back-substitution, the exp-map update with Eigen's matrix->quaternion
rule, the robustified chi2 and the one-workgroup block-Jacobi CG -- written from the comments of that file and the
published formulas (EdgeProjectXYZ2UV::linearizeOplus, SE3Quat::exp, RobustKernelHuber), with no product code.
dtype-generic like amg_ref.py / pcg_ref.py: np.longdouble is the reference the device is compared with, np.float64 the
noise gauge of the "measured" checks (tests/test_gpu_ba_operators.py).  oracle/ba_oracle.py stays the float64 oracle of
the parity tests; tests/test_ba_ref.py pins this file to it.

A problem `P` is any object with cams (nc, 7) [qx qy qz qw tx ty tz], points (np, 3), oc, op (no,), uv (no, 2), f, cx,
cy, omega (= 1 / pixel_noise^2), huber and fixed (nc,) bool: oracle.ba_oracle.Problem is one.

Layouts are the device's: lin (no, 20) = [A (2 x 6 row-major), B (2 x 3 row-major), es (2)], all times sqrt(w omega);
Z (no, 6, 3); camera vectors 7 per camera with a zero pad; blocks [k, r, c] 7 x 7 whose 7th row / column is the
identity's; block-CSR with the diagonal block first in every row, then ascending columns.

The sums come with their MAGNITUDES (the same expression with every term replaced by its absolute value): the derived
bounds of the GPU test are gamma(k) x magnitude.

`mut` names ONE deliberate defect (MUTATIONS); tests/test_ba_ref.py shows that the comparison the GPU test makes
separates each of them from rounding:
  pair_drop .......... k_ba_reduced's lane-stride loop over a block's pair list loses the list's last pair (a list
                       of 65: the one pair of the second pass)
  pair_65_as_1 ....... the same loop reads the 65th pair as the 1st (e - 64 instead of e)
  damp_offdiag ....... `if (r == c) mine += lambda` without the `dg` around it
  g_no_Zbp ........... g = b_c, the `vg` term (sum Z_o b_p) left out
  backsub_ZT ......... k_ba_backsub reads Z_o as 3 x 6 (z[6 c + r] for z[3 r + c])
  V_half ............. the small-angle branch of SE3Quat::exp with the series' V = I + Omega / 2 instead of the
                       as-written V = R = I + Omega + Omega^2
  quat_jl_swap ....... j and l exchanged in Eigen's largest-diagonal-entry branch
  beta_old_rz ........ k_ba_pcg's beta = rz_new / rz with the rz of the iteration before
  iter_plus_one ...... k_ba_pcg runs one iteration past its cap
"""
import numpy as np

import amg_ref as R

LD, U = R.LD, R.U

MUTATIONS = ("pair_drop", "pair_65_as_1", "damp_offdiag", "g_no_Zbp", "backsub_ZT", "V_half", "quat_jl_swap",
             "beta_old_rz", "iter_plus_one")


def gamma_k(k):
    """gamma(k) = k u / (1 - k u) in long double (Higham's constant of a sum of k rounded terms)."""
    ku = np.asarray(k, dtype=LD) * LD(U)
    return ku / (1 - ku)


# ---------------------------------------------------------------------------------------------- linearisation
def quat_to_R(q, dt):
    return R.rot_from_quat(q, dt)


def camera_frame(P, cams, points, dt):
    """(R (no, 3, 3), X (no, 3)): rotation of every observation's camera and the point in its frame."""
    cams, points = np.asarray(cams, dtype=dt), np.asarray(points, dtype=dt)
    Rm = quat_to_R(cams[:, :4], dt)[P.oc]
    X = np.einsum("nij,nj->ni", Rm, points[P.op]) + cams[P.oc, 4:7]
    return Rm, X


def residual(P, cams, points, dt):
    """(R, X, e): e = uv - K (R p + t)."""
    Rm, X = camera_frame(P, cams, points, dt)
    f, cx, cy = dt(P.f), dt(P.cx), dt(P.cy)
    uv = np.asarray(P.uv, dtype=dt)
    e = np.stack([uv[:, 0] - (f * X[:, 0] / X[:, 2] + cx), uv[:, 1] - (f * X[:, 1] / X[:, 2] + cy)], axis=1)
    return Rm, X, e


def huber(e2, delta, dt):
    """RobustKernelHuber on e2 = e^T Omega e: (rho, w = rho'), inliers e2 <= delta^2 (or delta <= 0)."""
    e2 = np.asarray(e2, dtype=dt)
    d = dt(delta)
    inl = (e2 <= d * d) if delta > 0 else np.ones(e2.shape, dtype=bool)
    sq = np.sqrt(np.where(inl, dt(1), e2))
    rho = np.where(inl, e2, 2 * sq * d - d * d)
    w = np.where(inl, dt(1), d / sq)
    return rho, w, inl


def rho_terms(P, cams, points, dt):
    """(rho (no,), inlier mask): the terms of the robustified chi2."""
    _, _, e = residual(P, cams, points, dt)
    rho, _, inl = huber(dt(P.omega) * (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]), P.huber, dt)
    return rho, inl


def jacobians(P, cams, points, dt):
    """(J_cam (no, 2, 6) over [omega, upsilon], J_point (no, 2, 3), e (no, 2)) of EdgeProjectXYZ2UV (analytic)."""
    Rm, X, e = residual(P, cams, points, dt)
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    f, z2 = dt(P.f), X[:, 2] * X[:, 2]
    n = x.shape[0]
    Jc = np.zeros((n, 2, 6), dtype=dt)
    Jc[:, 0, 0] = x * y / z2 * f; Jc[:, 0, 1] = -(1 + x * x / z2) * f; Jc[:, 0, 2] = y / z * f
    Jc[:, 0, 3] = -1 / z * f; Jc[:, 0, 5] = x / z2 * f
    Jc[:, 1, 0] = (1 + y * y / z2) * f; Jc[:, 1, 1] = -x * y / z2 * f; Jc[:, 1, 2] = -x / z * f
    Jc[:, 1, 4] = -1 / z * f; Jc[:, 1, 5] = y / z2 * f
    # J_point = -1/z [[f, 0, -f x/z], [0, f, -f y/z]] R
    T = np.zeros((n, 2, 3), dtype=dt)
    T[:, 0, 0] = f; T[:, 0, 2] = -x / z * f
    T[:, 1, 1] = f; T[:, 1, 2] = -y / z * f
    Jp = -(T @ Rm) / z[:, None, None]
    return Jc, Jp, e


def linearize(P, cams, points, dt):
    """lin (no, 20) of k_ba_obs: [sqrt(w omega) J_cam, sqrt(w omega) J_point, sqrt(w omega) e]."""
    Jc, Jp, e = jacobians(P, cams, points, dt)
    _, w, _ = huber(dt(P.omega) * (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]), P.huber, dt)
    sw = np.sqrt(w * dt(P.omega))[:, None]
    return np.concatenate([sw * Jc.reshape(-1, 12), sw * Jp.reshape(-1, 6), sw * e], axis=1)


def split_lin(lin, dt):
    """(A (no, 2, 6), B (no, 2, 3), es (no, 2)) of a lin array."""
    lin = np.asarray(lin, dtype=dt)
    return lin[:, :12].reshape(-1, 2, 6), lin[:, 12:18].reshape(-1, 2, 3), lin[:, 18:20]


# ---------------------------------------------------------------------------------------------- point blocks
def _seg_sum(v, idx, n):
    """out[i] = sum of the rows of v with idx == i (any dtype; empty segments are zero)."""
    out = np.zeros((n,) + v.shape[1:], dtype=v.dtype)
    if v.shape[0]:
        order = np.argsort(idx, kind="stable")
        cnt = np.bincount(idx, minlength=n)
        start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
        ne = cnt > 0
        out[ne] = np.add.reduceat(v[order], start[ne], axis=0)
    return out


def point_blocks(lin, op, n_points, dt):
    """Undamped H_pp = sum B^T B (np, 3, 3), b_p = -sum B^T es (np, 3), the magnitude of b_p and the observations per
    point m (np,).  (The magnitude of H_pp's diagonal is the diagonal itself.)"""
    _, B, es = split_lin(lin, dt)
    H = _seg_sum(np.einsum("nri,nrj->nij", B, B), op, n_points)
    bp = -_seg_sum(np.einsum("nri,nr->ni", B, es), op, n_points)
    bp_mag = _seg_sum(np.einsum("nri,nr->ni", np.abs(B), np.abs(es)), op, n_points)
    return H, bp, bp_mag, np.bincount(op, minlength=n_points)


def point_inverse(H, lam, dt):
    """(H_pp + lam I)^-1 to the precision of dt."""
    return R.accurate_inverse(np.asarray(H, dtype=dt) + dt(lam) * np.eye(3, dtype=dt), dt)


def z_blocks(lin, Hinv, op, dt):
    """(Z, magnitude): Z_o = (A^T B)_o Hinv_point(o), (no, 6, 3)."""
    A, B, _ = split_lin(lin, dt)
    Hi = np.asarray(Hinv, dtype=dt).reshape(-1, 3, 3)[op]
    Z = np.einsum("nri,nrj->nij", A, B) @ Hi
    mag = np.einsum("nri,nrj->nij", np.abs(A), np.abs(B)) @ np.abs(Hi)
    return Z, mag


# ---------------------------------------------------------------------------------------------- reduced system
def pair_lists(oc, op, n_cams):
    """The reduced camera system's pattern and the observation pairs behind every block, from the observations alone.
    Block (i, j) exists when i == j or cameras i and j see a common point; its list holds every ordered pair (o1, o2)
    of observations of ONE point with cam(o1) = i, cam(o2) = j -- for the diagonal block that includes (o, o) for
    every observation of the camera, and (o1, o2), (o2, o1) for a point the camera sees twice.
    Returns dict(rptr, bcol, brow, sptr, pa, pb): block-CSR with the diagonal first in every row, then ascending
    columns; block k's pairs are pa/pb[sptr[k]:sptr[k + 1]], ascending (point, o1, o2)."""
    oc, op = np.asarray(oc, dtype=np.int64), np.asarray(op, dtype=np.int64)
    order = np.lexsort((np.arange(op.shape[0]), op))
    cnt = np.bincount(op)
    cnt = cnt[cnt > 0]
    start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    # all ordered pairs within every point's run of `order`
    rep = np.repeat(cnt, cnt)                         # per observation: size of its point's run
    base = np.repeat(start, cnt)                      # per observation: start of its point's run
    a = np.repeat(np.arange(order.shape[0]), rep)     # position of o1
    off = np.arange(a.shape[0]) - np.repeat(np.concatenate([[0], np.cumsum(rep)[:-1]]), rep)
    b = base[a] + off                                 # position of o2
    o1, o2 = order[a], order[b]
    i, j = oc[o1], oc[o2]
    nc = int(n_cams)
    # key: row, then diagonal first, then column; the diagonal of every camera exists (maybe empty)
    key = i * (nc + 1) + np.where(i == j, 0, j + 1)
    dkey = np.arange(nc) * (nc + 1)
    ukey = np.unique(np.concatenate([key, dkey]))
    blk = np.searchsorted(ukey, key)
    srt = np.lexsort((o2, o1, op[o1], blk))
    pa, pb, blk = o1[srt], o2[srt], blk[srt]
    brow, rem = ukey // (nc + 1), ukey % (nc + 1)
    bcol = np.where(rem == 0, brow, rem - 1)
    sptr = np.concatenate([[0], np.cumsum(np.bincount(blk, minlength=ukey.shape[0]))])
    rptr = np.concatenate([[0], np.cumsum(np.bincount(brow, minlength=nc))])
    return dict(rptr=rptr.astype(np.int32), bcol=bcol.astype(np.int32), brow=brow.astype(np.int32),
                sptr=sptr.astype(np.int64), pa=pa, pb=pb)


def _block_sum(v, sptr):
    """out[k] = sum of v[sptr[k]:sptr[k + 1]] (empty lists give zero)."""
    out = np.zeros((sptr.shape[0] - 1,) + v.shape[1:], dtype=v.dtype)
    ne = np.diff(sptr) > 0
    if v.shape[0]:
        out[ne] = np.add.reduceat(v, sptr[:-1][ne], axis=0)
    return out


def reduced_system(lin, Z, bp, oc, op, lists, fixed, lam, dt, mut=None, chunk=400000, mag_dt=None):
    """The reduced camera system of k_ba_reduced from lin, Z and b_p:
         S_ij = [i = j] (lam I + sum_o A_o^T A_o) - sum over the block's pairs Z_o1 (A^T B)_o2^T
         b_c,i = -sum_o A_o^T es_o,   g_i = b_c,i - sum_o Z_o b_p(point(o)),   cdmax_i = diag sum_o A_o^T A_o
       (o: the observations of camera i); a block with a fixed camera on either side is the identity
       (diagonal) or zero, and the camera's g, b_c, cdmax are zero.
    Returns dict(S (nblk, 7, 7), g, b_c, cdmax (nc, 7), their magnitudes S_mag, g_mag, bc_mag, the term counts
    pairs (nblk,) and nd (nc,) = observations per camera).  mag_dt = np.float64 forms S_mag's pair sums in float64 and
    enlarges them by 1e-9 (a sum of non-negative terms: relative error <= gamma(3 pairs + 2) << 1e-9): the long-double
    products over a million pairs are most of this function's time."""
    A, B, es = split_lin(lin, dt)
    Z = np.asarray(Z, dtype=dt).reshape(-1, 6, 3)
    bp = np.asarray(bp, dtype=dt).reshape(-1, 3)
    fixed = np.asarray(fixed, dtype=bool)
    rptr, bcol, brow, sptr = lists["rptr"], lists["bcol"], lists["brow"], lists["sptr"]
    pa, pb = lists["pa"], lists["pb"]
    nblk, nc = bcol.shape[0], rptr.shape[0] - 1
    if mut in ("pair_drop", "pair_65_as_1"):  # the slip shows in lists whose second pass holds exactly one pair
        pa, pb = pa.copy(), pb.copy()
        keep = np.ones(pa.shape[0], dtype=bool)
        for k in np.flatnonzero(np.diff(sptr) == 65):
            if mut == "pair_drop":
                keep[sptr[k + 1] - 1] = False
            else:
                pa[sptr[k] + 64], pb[sptr[k] + 64] = pa[sptr[k]], pb[sptr[k]]
        blk_of = np.repeat(np.arange(nblk), np.diff(sptr))[keep]
        pa, pb = pa[keep], pb[keep]
        sptr = np.concatenate([[0], np.cumsum(np.bincount(blk_of, minlength=nblk))])
    Y = np.einsum("nri,nrj->nij", A, B)            # (A^T B)_o, 6 x 3
    Ya = np.einsum("nri,nrj->nij", np.abs(A), np.abs(B))
    Za = np.abs(Z)
    Zm, Ym = (Za, Ya) if mag_dt is None else (Za.astype(mag_dt), Ya.astype(mag_dt))
    S6 = np.zeros((nblk, 6, 6), dtype=dt)
    M6 = np.zeros((nblk, 6, 6), dtype=dt)
    blk_of = np.repeat(np.arange(nblk), np.diff(sptr))
    for s0 in range(0, pa.shape[0], chunk):  # (chunks: the temporaries stay small; a block's list may span two)
        sl = slice(s0, min(s0 + chunk, pa.shape[0]))
        a, b, k = pa[sl], pb[sl], blk_of[sl]
        kk, first = np.unique(k, return_index=True)
        S6[kk] -= np.add.reduceat(np.einsum("nik,njk->nij", Z[a], Y[b]), first, axis=0)
        mg = np.add.reduceat(np.einsum("nik,njk->nij", Zm[a], Ym[b]), first, axis=0)
        M6[kk] += mg if mag_dt is None else mg.astype(dt) * dt(1 + 1e-9)
    oc_of = np.asarray(oc, dtype=np.int64)
    dg = brow == bcol
    AtA = _seg_sum(np.einsum("nri,nrj->nij", A, A), oc_of, nc)
    AtA_mag = _seg_sum(np.einsum("nri,nrj->nij", np.abs(A), np.abs(A)), oc_of, nc)
    dk = rptr[:-1]
    S6[dk] += AtA + dt(lam) * np.eye(6, dtype=dt)
    M6[dk] += AtA_mag + abs(dt(lam)) * np.eye(6, dtype=dt)
    if mut == "damp_offdiag":
        S6[~dg] += dt(lam) * np.eye(6, dtype=dt)
    bc = -_seg_sum(np.einsum("nri,nr->ni", A, es), oc_of, nc)
    bc_mag = _seg_sum(np.einsum("nri,nr->ni", np.abs(A), np.abs(es)), oc_of, nc)
    zb = -_seg_sum(np.einsum("nik,nk->ni", Z, bp[op]), oc_of, nc)
    zb_mag = _seg_sum(np.einsum("nik,nk->ni", Za, np.abs(bp[op])), oc_of, nc)
    g = bc.copy() if mut == "g_no_Zbp" else bc + zb
    g_mag = bc_mag + zb_mag
    cdmax = AtA.diagonal(0, 1, 2).copy()
    # fixed cameras leave the system
    fb = fixed[brow] | fixed[bcol]
    S6[fb] = 0
    M6[fb] = 0
    S6[fb & dg] = np.eye(6, dtype=dt)
    for v in (g, g_mag, bc, bc_mag, cdmax):
        v[fixed] = 0
    S = np.zeros((nblk, 7, 7), dtype=dt)
    Sm = np.zeros((nblk, 7, 7), dtype=dt)
    S[:, :6, :6], Sm[:, :6, :6] = S6, M6
    S[dg, 6, 6] = 1
    pad7 = lambda v: np.concatenate([v, np.zeros((nc, 1), dtype=dt)], axis=1)
    return dict(S=S, S_mag=Sm, g=pad7(g), g_mag=pad7(g_mag), b_c=pad7(bc), bc_mag=pad7(bc_mag), cdmax=pad7(cdmax),
                pairs=np.diff(sptr), nd=np.bincount(oc_of, minlength=nc), fixed_block=fb)


def backsub(Hinv, bp, Z, dxc, oc, op, dt, mut=None):
    """(dx_p, magnitude, m): dx_p = Hinv b_p - sum_o Z_o^T dx_c(cam(o)) per point."""
    Hi = np.asarray(Hinv, dtype=dt).reshape(-1, 3, 3)
    bp = np.asarray(bp, dtype=dt).reshape(-1, 3)
    Z = np.asarray(Z, dtype=dt).reshape(-1, 6, 3)
    if mut == "backsub_ZT":
        Z = Z.reshape(-1, 3, 6).transpose(0, 2, 1)
    x6 = np.asarray(dxc, dtype=dt).reshape(-1, 7)[oc, :6]
    n = Hi.shape[0]
    d = np.einsum("pij,pj->pi", Hi, bp) - _seg_sum(np.einsum("nrc,nr->nc", Z, x6), op, n)
    mag = np.einsum("pij,pj->pi", np.abs(Hi), np.abs(bp)) + _seg_sum(np.einsum("nrc,nr->nc", np.abs(Z), np.abs(x6)), op, n)
    return d, mag, np.bincount(op, minlength=n)


# ---------------------------------------------------------------------------------------------- the update
def _skew(w):
    return R._skew(w)


def se3_exp(u, dt, mut=None):
    """SE3Quat::exp of u = [omega, upsilon] (n, 6): (R, t, small), with the as-written small-angle branch
    th < 1e-5: R = I + Omega + Omega^2, V = R."""
    u = np.asarray(u, dtype=dt)
    om, up = u[:, :3], u[:, 3:6]
    th = np.sqrt(om[:, 0] * om[:, 0] + om[:, 1] * om[:, 1] + om[:, 2] * om[:, 2])
    Om = _skew(om)
    Om2 = Om @ Om
    small = th < dt(1e-5)
    t1 = np.where(small, dt(1), th)
    a = (np.sin(t1) / t1)[:, None, None]
    b = ((1 - np.cos(t1)) / (t1 * t1))[:, None, None]
    c = ((t1 - np.sin(t1)) / (t1 * t1 * t1))[:, None, None]
    I = np.eye(3, dtype=dt)
    Rs = I + Om + Om2
    Vs = I + Om / 2 if mut == "V_half" else Rs
    s3 = small[:, None, None]
    Rm = np.where(s3, Rs, I + a * Om + b * Om2)
    V = np.where(s3, Vs, I + b * Om + c * Om2)
    return Rm, np.einsum("nij,nj->ni", V, up), small


def R_to_quat(Rm, dt, mut=None):
    """Eigen's Quaternion(Matrix3) on (n, 3, 3): (q (n, 4) x y z w, branch (n,)): branch 3 = trace > 0, else the index
    i of the largest diagonal entry (ties: the first, then `>`)."""
    Rm = np.asarray(Rm, dtype=dt)
    n = Rm.shape[0]
    q = np.zeros((n, 4), dtype=dt)
    branch = np.zeros(n, dtype=np.int64)
    for m in range(n):
        M = Rm[m]
        tr = M[0, 0] + M[1, 1] + M[2, 2]
        if tr > 0:
            k = np.sqrt(tr + 1)
            q[m, 3] = k / 2
            k = 1 / (2 * k)
            q[m, :3] = [(M[2, 1] - M[1, 2]) * k, (M[0, 2] - M[2, 0]) * k, (M[1, 0] - M[0, 1]) * k]
            branch[m] = 3
        else:
            i = 0
            if M[1, 1] > M[0, 0]:
                i = 1
            if M[2, 2] > M[i, i]:
                i = 2
            j, l = (i + 1) % 3, (i + 2) % 3
            if mut == "quat_jl_swap":
                j, l = l, j
            k = np.sqrt(M[i, i] - M[j, j] - M[l, l] + 1)
            q[m, i] = k / 2
            k = 1 / (2 * k)
            q[m, 3] = (M[l, j] - M[j, l]) * k
            q[m, j] = (M[j, i] + M[i, j]) * k
            q[m, l] = (M[l, i] + M[i, l]) * k
            branch[m] = i
    return q, branch


def update(cams, points, dxc, dxp, fixed, dt, mut=None):
    """k_ba_update: T <- exp([omega, upsilon]) T for the free cameras (quaternion by Eigen's rule, normalised), p += dx.
    dxc (nc, 7) or (nc, 6).  Returns dict(cams, points, branch (nc,; -1 for a fixed camera), small (nc,))."""
    cams = np.asarray(cams, dtype=dt).reshape(-1, 7)
    nc = cams.shape[0]
    u = np.asarray(dxc, dtype=dt).reshape(nc, -1)[:, :6]
    fixed = np.asarray(fixed, dtype=bool)
    Re, te, small = se3_exp(u, dt, mut)
    Rn = Re @ quat_to_R(cams[:, :4], dt)
    tn = np.einsum("nij,nj->ni", Re, cams[:, 4:7]) + te
    q, branch = R_to_quat(Rn, dt, mut)
    q = q / np.sqrt((q * q).sum(1))[:, None]
    new = np.concatenate([q, tn], axis=1)
    new[fixed] = cams[fixed]
    branch[fixed] = -1
    pts = np.asarray(points, dtype=dt).reshape(-1, 3) + np.asarray(dxp, dtype=dt).reshape(-1, 3)
    return dict(cams=new, points=pts, branch=branch, small=small & ~fixed)


def quat_branch(cams, dt=LD):
    """Branch of Eigen's rule every camera's OWN rotation falls on (where an identity step leaves it)."""
    return R_to_quat(quat_to_R(np.asarray(cams, dtype=dt)[:, :4], dt), dt)[1]


def scale_terms(x, b, lam, dt):
    """(terms, magnitudes) of scale = sum x (lam x + b)."""
    x, b = np.asarray(x, dtype=dt).ravel(), np.asarray(b, dtype=dt).ravel()
    return x * (dt(lam) * x + b), np.abs(x) * (abs(dt(lam)) * np.abs(x) + np.abs(b))


# ---------------------------------------------------------------------------------------------- the two-view trial
# One LM trial of sim3opt_amd/csrc/ba_batch.hip (k_ba_two_view: a workgroup per problem, camera 0 fixed) for a whole
# ragged batch at once.  The per-point arrays are the kernel's scratch rows; a problem's sums run over an index list
# into them, so that the slips of an index (TWO_VIEW_MUTATIONS) can be stated on the list.
#   wave3_drop ......... wg_sum without the fourth wavefront's partial: the points i with i % 256 >= 192 leave every sum
#   p256_as_0 .......... the 256-thread stride reads point i - 256 for point i = 256
#   prev_offset ........ problem k's point i read at problem k - 1's offset (scr[r total + ptr[k - 1] + i])
#   damp_none .......... H_pp inverted without lambda;  damp_offdiag: lambda on every entry of H_pp
#   no_cam0 ............ camera 0's observation missing from H_pp and b_p;  cam0_in_AtA: present in sum A_1^T A_1
#   huber_swapped ...... sqrt(w omega) of one view's observation used for the other view's
#   g_no_Zbp ........... g = b_c;  backsub_ZT: Z read as 3 x 6;  scale_no_cam: x.(lambda x + b) over the points only
#   hinv_other_lambda .. the H_pp^-1 rows of the trial before, at lambda / 2, left in the scratch: Z and the sums are
#                        this trial's, the back-substitution reads the stale inverse
#   maxdiag_no_cam ..... computeLambdaInit's maximum over the points only, the camera's diagonal left out
#   maxdiag_wave3 ...... wg_max without the fourth wavefront's maximum
#   V_half, quat_jl_swap as above
TWO_VIEW_MUTATIONS = ("wave3_drop", "p256_as_0", "prev_offset", "damp_none", "damp_offdiag", "no_cam0", "cam0_in_AtA",
                      "huber_swapped", "g_no_Zbp", "backsub_ZT", "scale_no_cam", "hinv_other_lambda", "maxdiag_no_cam",
                      "maxdiag_wave3", "V_half", "quat_jl_swap")


class TwoViewBatch:
    """The batch as one problem `P` of this file: cameras 2 k (fixed) and 2 k + 1 of problem k, observations 2 g (camera
    0's) and 2 g + 1 (camera 1's) of point g; ptr as sim3opt_ba_batch_set_problems takes it."""

    def __init__(self, ptr, cam0, cam1, points, uv0, uv1, f, cx, cy, huber=3.0, pixel_noise=1.0):
        self.ptr = np.asarray(ptr, dtype=np.int64)
        n, cnt = self.ptr.shape[0] - 1, np.diff(self.ptr)
        self.cams = np.stack([np.asarray(cam0).reshape(n, 7), np.asarray(cam1).reshape(n, 7)], axis=1).reshape(2 * n, 7)
        self.points = np.asarray(points).reshape(-1, 3)
        self.uv = np.stack([np.asarray(uv0).reshape(-1, 2), np.asarray(uv1).reshape(-1, 2)], axis=1).reshape(-1, 2)
        self.problem_of = np.repeat(np.arange(n), cnt)
        self.oc = np.stack([2 * self.problem_of, 2 * self.problem_of + 1], axis=1).ravel()
        self.op = np.repeat(np.arange(self.points.shape[0]), 2)
        self.fixed = np.tile([True, False], n)
        self.f, self.cx, self.cy, self.huber, self.omega = f, cx, cy, huber, 1.0 / (pixel_noise * pixel_noise)

    def index_lists(self, mut=None):
        """Per problem: the points its sums read."""
        out = []
        for k in range(self.ptr.shape[0] - 1):
            i = np.arange(self.ptr[k + 1] - self.ptr[k])
            idx = self.ptr[k] + i
            if mut == "wave3_drop":
                idx = idx[i % 256 < 192]
            elif mut == "p256_as_0" and idx.shape[0] > 256:
                idx[256] = idx[0]
            elif mut == "prev_offset" and k > 0:
                idx = np.minimum(self.ptr[k - 1] + i, self.ptr[-1] - 1)
            out.append(idx)
        return out


def active_terms(P, cams, points, dt):
    """e^T Omega e of every observation: the terms of g2o's activeChi2 (no robust kernel)."""
    _, _, e = residual(P, cams, points, dt)
    return dt(P.omega) * (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1])


def lambda_init_maxdiag(hpp_diag, cam_diag):
    """computeLambdaInit's maximum over the free vertices: the diagonals of the (undamped) H_pp of the points and of
    sum A^T A of the free cameras."""
    return max(np.max(hpp_diag), np.max(cam_diag))


def two_view_rows(P, lam_point, dt, mut=None):
    """The per-point rows of pass L and pass S at the estimate P.cams, P.points: dict of H (T, 3, 3, undamped), b_p,
    bp_mag, A1 (T, 2, 6), B1 (T, 2, 3), es1 (T, 2), A0 (camera 0's A, which the kernel never forms), H0 and bp0
    (camera 0's share of H and b_p), Hinv (T, 3, 3), Y, Z, Z_mag (T, 6, 3), rho, e2 (T, 2).  lam_point (T,): the
    damping of every point's problem."""
    Jc, Jp, e = jacobians(P, P.cams, P.points, dt)
    e2 = dt(P.omega) * (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1])
    rho, w, _ = huber(e2, P.huber, dt)
    if mut == "huber_swapped":
        w = w.reshape(-1, 2)[:, ::-1].reshape(-1)
    sw = np.sqrt(w * dt(P.omega))[:, None]
    lin = np.concatenate([sw * Jc.reshape(-1, 12), sw * Jp.reshape(-1, 6), sw * e], axis=1)
    T = P.points.shape[0]
    lin_h = lin.copy()
    if mut == "no_cam0":
        lin_h[0::2] = 0
    H, bp, bp_mag, _ = point_blocks(lin_h, P.op, T, dt)
    A, B, es = split_lin(lin, dt)
    A0, B0, es0, A1, B1 = A[0::2], B[0::2], es[0::2], A[1::2], B[1::2]
    # camera 0's share of H_pp and b_p, which the kernel keeps in registers only: (value, magnitude) each
    H0 = (np.einsum("nri,nrj->nij", B0, B0), np.einsum("nri,nrj->nij", np.abs(B0), np.abs(B0)))
    bp0 = (-np.einsum("nri,nr->ni", B0, es0), np.einsum("nri,nr->ni", np.abs(B0), np.abs(es0)))
    lam = np.asarray(lam_point, dtype=dt)[:, None, None]
    damp = np.ones((3, 3), dtype=dt) if mut == "damp_offdiag" else np.eye(3, dtype=dt)

    def inverse(l):  # (the kernel stores six entries: its inverse is symmetric)
        X = R.accurate_inverse(H + (0 if mut == "damp_none" else l * damp), dt)
        return (X + X.transpose(0, 2, 1)) / 2

    Hinv = inverse(lam)
    Y = np.einsum("nri,nrj->nij", A1, B1)
    Z = Y @ Hinv
    Z_mag = np.einsum("nri,nrj->nij", np.abs(A1), np.abs(B1)) @ np.abs(Hinv)
    if mut == "hinv_other_lambda":
        Hinv = inverse(lam / 2)
    return dict(H=H, b_p=bp, bp_mag=bp_mag, H0=H0, bp0=bp0, A1=A1, B1=B1, es1=es[1::2], A0=A0, Hinv=Hinv, Y=Y, Z=Z,
                Z_mag=Z_mag, rho=rho.reshape(-1, 2), e2=e2.reshape(-1, 2))


def two_view_sums(rows, idx, lam, dt, mut=None):
    """One problem's sums over the points idx of per-point rows (the reference's, or the device's own A1, B1, es1, Z,
    b_p in dt): AtA = sum A_1^T A_1, b_c = -sum A_1^T es_1, ZY = -sum Z Y^T, Zb = -sum Z b_p, the damped S = lam I +
    AtA + ZY as one 6 x 6 block, g = b_c + Zb, each with its magnitude `<name>_mag`; n = len(idx)."""
    g = lambda k: np.asarray(rows[k], dtype=dt)[idx]
    A, B, es, Z, bp = g("A1"), g("B1"), g("es1"), g("Z"), g("b_p")
    Y = np.einsum("nri,nrj->nij", A, B)
    out = dict(AtA=np.einsum("nri,nrj->ij", A, A), AtA_mag=np.einsum("nri,nrj->ij", np.abs(A), np.abs(A)),
               b_c=-np.einsum("nri,nr->i", A, es), b_c_mag=np.einsum("nri,nr->i", np.abs(A), np.abs(es)),
               ZY=-np.einsum("nik,njk->ij", Z, Y), ZY_mag=np.einsum("nik,njk->ij", np.abs(Z), np.abs(Y)),
               Zb=-np.einsum("nik,nk->i", Z, bp), Zb_mag=np.einsum("nik,nk->i", np.abs(Z), np.abs(bp)), n=len(idx))
    if mut == "cam0_in_AtA":
        A0 = g("A0")
        out["AtA"] = out["AtA"] + np.einsum("nri,nrj->ij", A0, A0)
    I6 = np.eye(6, dtype=dt)
    out["S"] = out["AtA"] + out["ZY"] + dt(lam) * I6
    out["S_mag"] = out["AtA_mag"] + out["ZY_mag"] + abs(dt(lam)) * I6
    out["g"] = out["b_c"].copy() if mut == "g_no_Zbp" else out["b_c"] + out["Zb"]
    out["g_mag"] = out["b_c_mag"] + out["Zb_mag"]
    return out


def two_view_backsub(rows, step_point, dt, mut=None):
    """(dx_p, magnitude) of every point: H_pp^-1 b_p - Z^T dx_c, dx_c (T, 6) the step of the point's camera 1."""
    g = lambda k: np.asarray(rows[k], dtype=dt)
    Hi, bp, Z, x = g("Hinv"), g("b_p"), g("Z"), np.asarray(step_point, dtype=dt)
    if mut == "backsub_ZT":
        Z = Z.reshape(-1, 3, 6).transpose(0, 2, 1)
    return (np.einsum("pij,pj->pi", Hi, bp) - np.einsum("nrc,nr->nc", Z, x),
            np.einsum("pij,pj->pi", np.abs(Hi), np.abs(bp)) + np.einsum("nrc,nr->nc", np.abs(Z), np.abs(x)))


def two_view_scale(dxp, bp, step, bc, lam, dt, mut=None):
    """(x.(lam x + b), its magnitude, the number of terms) of one problem: its points, then camera 1's six."""
    x, b = [np.asarray(dxp, dtype=dt).ravel()], [np.asarray(bp, dtype=dt).ravel()]
    if mut != "scale_no_cam":
        x.append(np.asarray(step, dtype=dt).ravel())
        b.append(np.asarray(bc, dtype=dt).ravel())
    t, mag = scale_terms(np.concatenate(x), np.concatenate(b), lam, dt)
    return t.sum(), mag.sum(), t.shape[0]


def two_view_trial(P, lam, dt, dx_c=None, mut=None):
    """The whole read-out of sim3opt_ba_batch_debug_trial from the estimate, in dt: dict of the rows (two_view_rows, and
    trial_points), and per problem (lists / arrays over k) the sums (two_view_sums), chi2, active, maxdiag, dx_c (the
    solve of S, g), cams (the trial camera 1 after the step dx_c[k] if given, else the solve's), branch, small, chi2_new
    and scale.  lam (n,).  No trial fails here: S must be positive definite."""
    n = P.ptr.shape[0] - 1
    lam = np.asarray(lam, dtype=dt)
    rows = two_view_rows(P, lam[P.problem_of], dt, mut)
    lists = P.index_lists(mut)
    sums = [two_view_sums(rows, lists[k], lam[k], dt, mut) for k in range(n)]
    out = dict(rows=rows, sums=sums)
    out["chi2"] = np.array([rows["rho"][i].sum() for i in lists], dtype=dt)
    out["active"] = np.array([rows["e2"][i].sum() for i in lists], dtype=dt)
    def maxdiag(i, s):
        hpp, cam = rows["H"][i].diagonal(0, 1, 2), s["AtA"].diagonal()
        if mut == "maxdiag_wave3":
            hpp = np.concatenate([hpp[np.arange(hpp.shape[0]) % 256 < 192], np.zeros((1, 3), dtype=dt)])
        return lambda_init_maxdiag(hpp, np.zeros(6, dtype=dt) if mut == "maxdiag_no_cam" else cam)

    out["maxdiag"] = np.array([maxdiag(i, s) for i, s in zip(lists, sums)], dtype=dt)
    out["dx_c"] = np.stack([np.linalg.solve(s["S"].astype(np.float64), s["g"].astype(np.float64)).astype(dt)
                            if dt is np.float64 else refined6(s["S"], s["g"]) for s in sums])
    step = out["dx_c"] if dx_c is None else np.asarray(dx_c, dtype=dt).reshape(n, 6)
    dxp, _ = two_view_backsub(rows, step[P.problem_of], dt, mut)
    full = np.zeros((2 * n, 6), dtype=dt)
    full[1::2] = step
    up = update(P.cams, P.points, full, dxp, P.fixed, dt, mut)
    rows["trial_points"] = up["points"]
    out["cams"], out["branch"], out["small"] = up["cams"][1::2], up["branch"][1::2], up["small"][1::2]
    rho_new = rho_terms(P, up["cams"], up["points"], dt)[0].reshape(-1, 2)
    out["chi2_new"] = np.array([rho_new[i].sum() for i in lists], dtype=dt)
    out["scale"] = np.array([two_view_scale(dxp[i], rows["b_p"][i], step[k], sums[k]["b_c"], lam[k], dt, mut)[0]
                             for k, i in enumerate(lists)], dtype=dt)
    return out


def refined6(S, g):
    """x = S^-1 g of one small dense system in long double: a float64 inverse, refined."""
    S, g = np.asarray(S, dtype=LD), np.asarray(g, dtype=LD)
    return R.refined_solve(S, np.linalg.inv(S.astype(np.float64)), g, steps=5)


# ---------------------------------------------------------------------------------------------- the PCG
def bcsr_matvec(rptr, bcol, S, p):
    """q = S p on the padded block-CSR (blocks [k, r, c])."""
    rows = R._row_of_block(np.asarray(rptr))
    q = np.zeros((rptr.shape[0] - 1, 7), dtype=S.dtype)
    t = np.einsum("krc,kc->kr", S, p.reshape(-1, 7)[bcol])
    if t.shape[0]:
        ne = np.diff(rptr) > 0
        q[ne] = np.add.reduceat(t, np.asarray(rptr)[:-1][ne], axis=0)
    return q.ravel()


def block_jacobi_cg(rptr, bcol, S, g, max_iter, rel_tol, dt, mut=None):
    """k_ba_pcg: block-Jacobi CG on S x = g, x_0 = 0:
         r = g, z = D^-1 r, p = z, rz = r.z;  while it < max_iter and rz > tol^2 rz_0 and rz > 0:
           q = S p, pq = p.q (not > 0 or not finite: fail, stop), alpha = rz / pq, x += alpha p, r -= alpha q,
           z = D^-1 r, beta = rz_new / rz, p = z + beta p
       fail also when a diagonal block has a non-positive Gauss-Jordan pivot or rz ends negative / NaN.
    Returns dict(x = [x_1 ...], x_last, iters, rel = sqrt(|rz| / rz_0) (0 when rz_0 = 0), fail, pivots_ok, left = "pq"
    when the p.q test ended the loop, else "test": the loop condition did)."""
    rptr, bcol = np.asarray(rptr), np.asarray(bcol)
    S = np.asarray(S, dtype=dt)
    g = np.asarray(g, dtype=dt).ravel()
    D = S[rptr[:-1]]
    with np.errstate(all="ignore"):
        piv_ok = bool((gj_pivots(D) > 0).all())
        Dinv = R.small_inverse(D, dt)
        x, r = np.zeros_like(g), g.copy()
        z = R._bmv(Dinv, r)
        p = z.copy()
        rz = r @ z
        rz0 = rz_prev = rz
        tol2 = dt(rel_tol) * dt(rel_tol)
        xs, it, fail, left = [], 0, not piv_ok, "test"
        cap = max_iter + 1 if mut == "iter_plus_one" else max_iter
        while it < cap and rz > tol2 * rz0 and rz > 0:
            q = bcsr_matvec(rptr, bcol, S, p)
            pq = p @ q
            if not (pq > 0) or not np.isfinite(pq):
                fail, left = True, "pq"
                break
            alpha = rz / pq
            x = x + alpha * p
            r = r - alpha * q
            z = R._bmv(Dinv, r)
            rzn = r @ z
            beta = rzn / (rz_prev if (mut == "beta_old_rz" and it > 0) else rz)
            p = z + beta * p
            rz_prev, rz = rz, rzn
            it += 1
            xs.append(x.copy())
        if not (rz >= 0):
            fail = True
        rel = np.sqrt(abs(rz) / rz0) if rz0 > 0 else dt(0)
    return dict(x=xs, iters=it, rel=rel, fail=fail, pivots_ok=piv_ok, left=left, x_last=x)


def gj_pivots(D):
    """Pivots of the unpivoted elimination of [n, 7, 7] blocks, in the blocks' dtype: what k_ba_pcg's D^-1 loop tests
    (`!(a[k][k] > 0)` sets fail; the iteration goes on)."""
    a = np.array(D, copy=True)
    piv = np.empty(a.shape[:2], dtype=a.dtype)
    for k in range(a.shape[1]):
        piv[:, k] = a[:, k, k]
        a = a - a[:, :, k, None] * (a[:, k, None, :] / a[:, k, k, None, None])
    return piv


def dense_solve(rptr, bcol, S, g, dt):
    """x = S^-1 g by a dense float64 LU, refined in dt (the long-double yardstick of the exact solver)."""
    rptr, bcol = np.asarray(rptr), np.asarray(bcol)
    nb = rptr.shape[0] - 1
    A = R.dense_of(nb, R._row_of_block(rptr), bcol, S, dt)
    g = np.asarray(g, dtype=dt).ravel()
    if dt is np.float64:
        return np.linalg.solve(A, g)
    X0 = np.linalg.inv(A.astype(np.float64))
    return R.refined_solve(A, X0, g, steps=5)


# ---------------------------------------------------------------------------------------------- the comparisons
# Roundings on the longest path to an entry, for ANY summation order and any FMA contraction (a product is one
# rounding, a sum of T terms at most T - 1 more; an FMA only removes roundings).  m = observations of the point,
# nd = observations of the camera, pairs = length of the block's pair list:
K_Z = 5                                   # y = a b + a' b' (2), times Hinv (1), sum of three (2)
k_bp = lambda m: 2 * m                    # 2 m products (1) summed (2 m - 1); the same for the diagonal of H_pp
k_bc = lambda nd: 2 * nd                  # likewise; the same for cdmax
k_g = lambda nd: 5 * nd + 1               # 2 nd + 3 nd products summed (5 nd), g = b_c + (Z b_p part) one more
k_S = lambda pairs, nd: 3 * pairs + 2 * nd + 3   # y (2), z y (1), 3 pairs + 2 nd terms summed, + lambda (1)
k_dxp = lambda m: 6 * m + 3               # 3 + 6 m products (1) summed (6 m + 2)
k_sum = lambda n, per_term: n + per_term  # n terms of per_term roundings each, summed (n - 1)


def derived_ratio(dev, ref, mag, k):
    """max over the entries of |dev - ref| / (gamma(k) mag); an entry whose bound is zero must be exact."""
    err = np.abs(np.asarray(dev, dtype=LD) - np.asarray(ref, dtype=LD))
    tol = np.broadcast_to(gamma_k(k), err.shape) * np.asarray(mag, dtype=LD)
    assert (err[tol == 0] == 0).all(), "an entry with a zero bound is not exact"
    return float((err[tol > 0] / tol[tol > 0]).max()) if (tol > 0).any() else 0.0


def s_counts(red, lists, n_cams):
    """k of every entry of S (nblk, 1, 1): the block's pairs, and the camera's observations on the diagonal."""
    dg = lists["brow"] == lists["bcol"]
    nd = np.where(dg, red["nd"][lists["brow"]], 0)
    return k_S(red["pairs"].astype(np.int64), nd)[:, None, None]


def inverse_residual_ratio(Hinv_dev, H_ld, lam, m):
    """max over the points of || Hinv_dev (H + lam I) - I ||_1 / bound, H = sum B^T B in long double from the device's
    lin.  The bound, with A = H + lam I, rho = ||A||_1^3 / det A (<= 3 sqrt(3) kappa_1(A)^2: the cofactor inverse's
    error is u ||A||^2 per cofactor against det / ||A||) and kappa_1 = ||A||_1 ||A^-1||_1:
        (22 rho + 2) u ............ cofactors (gamma(2) of <= 2 ||A||^2), determinant (gamma(3) more), 1 / det and the
                                    product (2 u), multiplied out in X A - I
      + 3 gamma(2 m + 1) kappa_1 .. the device inverts ITS sum of 2 m products plus lambda, |dH| <= gamma(2 m + 1)
                                    |B|^T |B|, ||.||_1 of which is <= 3 max diag <= 3 ||A||_1
    times 1.01 for the second-order terms."""
    A = np.asarray(H_ld, dtype=LD) + LD(lam) * np.eye(3, dtype=LD)
    X = np.asarray(Hinv_dev, dtype=LD).reshape(-1, 3, 3)
    res = np.abs(X @ A - np.eye(3, dtype=LD)).sum(1).max(1)
    n1 = np.abs(A).sum(1).max(1)
    det = np.linalg.det(A.astype(np.float64)).astype(LD)
    kap = n1 * np.abs(R.accurate_inverse(A, LD)).sum(1).max(1)
    bound = LD(1.01) * ((22 * n1 ** 3 / det + 2) * LD(U) + 3 * gamma_k(2 * np.asarray(m) + 1) * kap)
    return float((res / bound).max()), float(kap.max())


def chi2_ratio(chi_dev, P, cams, points):
    """(|chi_dev - sum rho_ld| / tolerance, inlier mask) of the robustified chi2 of an estimate.  The tolerance has
    two parts: the sum of n terms in any order, gamma(n) sum rho (derived); and the terms themselves, which the device
    forms from the estimate through a division and a cancelling difference: 32 x |float64 restatement - long double|
    per term, floored at 4u rho, added up as if all terms erred the same way (the measured convention, per term)."""
    rho_ld, inl = rho_terms(P, cams, points, LD)
    rho_64, _ = rho_terms(P, cams, points, np.float64)
    per_term = np.maximum(np.abs(rho_64.astype(LD) - rho_ld), 4 * LD(U) * rho_ld)
    tol = gamma_k(rho_ld.shape[0]) * rho_ld.sum() + 32 * per_term.sum()
    return float(abs(LD(chi_dev) - rho_ld.sum()) / tol), inl
