"""Plain numpy restatement of the Sim(3) LM set-up and update kernels of sim3opt_amd/csrc/lm_kernels.hpp -- residuals,
numeric and closed-form Jacobians, the robust kernels, the Gram phase with its slot and incidence stores, the per-row
reduction, trace and max, oplus, the scale and chi2 sums -- written from the comments of sim3_math.hpp, sim3_jac.hpp,
robust.hpp and lm_kernels.hpp and the published formulas (g2o's Sim3 exp / log, EdgeSim3, RobustKernel*), with no product
code.  dtype-generic like amg_ref.py / ba_ref.py / pcg_ref.py: np.longdouble is the reference the device is compared with,
np.float64 the noise gauge of the "measured" checks (tests/test_gpu_lm_operators.py).  oracle/oracle.py stays the float64
oracle of the parity tests; tests/test_lm_ref.py pins this file to it.

Layouts are the device's: states [qx qy qz qw tx ty tz s], tangents [omega upsilon sigma]; J (edges, 15, 7) = 14
Jacobian COLUMNS (7 of endpoint 0, 7 of endpoint 1) of 7 residual rows each, then e; Omega (edges, 7, 7), symmetric;
blocks [k, r, c]; the per-incidence scratch = upper triangle in column-major order (entry (m, M), m <= M, at
M (M + 1) / 2 + m), then the 7 entries of b.

The sums come with their MAGNITUDES (the same expression with every term replaced by its absolute value): the derived
bounds of the GPU test are gamma(k) x magnitude, k below.

`mut` names ONE deliberate defect (MUTATIONS); tests/test_lm_ref.py shows that the comparison the GPU test makes
separates each of them from rounding:
  h10_untransposed ... H10 stored as H01 (G[r][7 + c] for G[c][7 + r])
  inc_swapped ........ the endpoints' incidence slots exchanged (A^T W A into endpoint 1's slot)
  inc_dropped ........ k_diag_reduce's loop over a row's incidences stops one short
  tri_off_by_one ..... the upper-triangle map tr / tc shifted by one entry
  b_sign ............. b = +J^T W e
  w_twice ............ the robust weight applied to the Gram entries twice
  w_from_ee .......... the weight taken at e^T e instead of e^T Omega e
  frozen_nonzero ..... a frozen DoF's Jacobian column left as differentiated
  right_perturbation . S exp(d) for exp(d) S in the central differences
  delta_swapped ...... +delta and -delta exchanged (the quotient's sign)
  half_factor ........ 1 / delta for 1 / (2 delta)
  oplus_right ........ S exp(dx) for exp(dx) S in the update
  scale_no_lambda .... scale = x . b
  max_over_H ......... max |H| over the whole diagonal blocks instead of their scalar diagonals (invisible: the blocks
                       are positive semi-definite, their largest entry is on the diagonal)
"""
import numpy as np

import amg_ref as R

LD, U = R.LD, R.U

MUTATIONS = ("h10_untransposed", "inc_swapped", "inc_dropped", "tri_off_by_one", "b_sign", "w_twice", "w_from_ee",
             "frozen_nonzero", "right_perturbation", "delta_swapped", "half_factor", "oplus_right", "scale_no_lambda",
             "max_over_H")

KINDS = dict(NONE=0, HUBER=1, PSEUDO_HUBER=2, CAUCHY=3, GEMAN_MCCLURE=4, WELSCH=5, FAIR=6, TUKEY=7, SATURATED=8, DCS=9)


def gamma_k(k):
    """gamma(k) = k u / (1 - k u) in long double (Higham's constant of a sum of k rounded terms)."""
    ku = np.asarray(k, dtype=LD) * LD(U)
    return ku / (1 - ku)


def mopts(**options):
    """The branch thresholds and switches of sim3_math.hpp as Engine::mopts() hands them to the kernels: exp_eps,
    small_rot_half and fix_small_angle_b of the library's own option defaults, overridden by `options`."""
    from sim3opt_amd import lib as L
    o = L.default_options(**options)
    return dict(eps=float(o.exp_eps), half=int(o.small_rot_half), fixb=int(o.fix_small_angle_b))


# ---------------------------------------------------------------------------------------------- quaternions, Sim(3)
def _c(x, dt):
    return np.asarray(x, dtype=dt)


def quat_mul(a, b):
    ax, ay, az, aw = (a[..., i] for i in range(4))
    bx, by, bz, bw = (b[..., i] for i in range(4))
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz], axis=-1)


def quat_rot(q, v):
    qv = q[..., :3]
    u = 2 * np.cross(qv, v)
    return v + q[..., 3:4] * u + np.cross(qv, u)


def R_from_quat(q):
    x, y, z, w = (q[..., i] for i in range(4))
    Rm = np.empty(q.shape[:-1] + (3, 3), dtype=q.dtype)
    Rm[..., 0, 0] = 1 - 2 * (y * y + z * z); Rm[..., 0, 1] = 2 * (x * y - z * w); Rm[..., 0, 2] = 2 * (x * z + y * w)
    Rm[..., 1, 0] = 2 * (x * y + z * w); Rm[..., 1, 1] = 1 - 2 * (x * x + z * z); Rm[..., 1, 2] = 2 * (y * z - x * w)
    Rm[..., 2, 0] = 2 * (x * z - y * w); Rm[..., 2, 1] = 2 * (y * z + x * w); Rm[..., 2, 2] = 1 - 2 * (x * x + y * y)
    return Rm


def quat_from_R(Rm):
    """Eigen's rule as sim3_math.hpp states it: the trace branch, else the largest diagonal entry's (ties: x, then y)."""
    d0, d1, d2 = Rm[..., 0, 0], Rm[..., 1, 1], Rm[..., 2, 2]
    tr = d0 + d1 + d2
    br = np.where(tr > 0, 3, np.where((d0 >= d1) & (d0 >= d2), 0, np.where((d1 > d0) & (d1 >= d2), 1, 2)))
    q = np.empty(Rm.shape[:-2] + (4,), dtype=Rm.dtype)
    one = Rm.dtype.type(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.sqrt(tr + one)
        cand = [np.stack([(Rm[..., 2, 1] - Rm[..., 1, 2]) * (0.5 / t), (Rm[..., 0, 2] - Rm[..., 2, 0]) * (0.5 / t),
                          (Rm[..., 1, 0] - Rm[..., 0, 1]) * (0.5 / t), 0.5 * t], axis=-1)]
        for i in range(3):
            j, k = (i + 1) % 3, (i + 2) % 3
            t = np.sqrt(Rm[..., i, i] - Rm[..., j, j] - Rm[..., k, k] + one)
            c = np.empty_like(q)
            c[..., i] = 0.5 * t
            c[..., 3] = (Rm[..., k, j] - Rm[..., j, k]) * (0.5 / t)
            c[..., j] = (Rm[..., j, i] + Rm[..., i, j]) * (0.5 / t)
            c[..., k] = (Rm[..., k, i] + Rm[..., i, k]) * (0.5 / t)
            cand.append(c)
    q[...] = cand[0]
    for i in range(3):
        q[br == i] = cand[i + 1][br == i]
    return q


def mul(a, b):
    """a * b : x -> a(b(x))"""
    q = quat_mul(a[..., :4], b[..., :4])
    t = a[..., 7:8] * quat_rot(a[..., :4], b[..., 4:7]) + a[..., 4:7]
    return np.concatenate([q, t, a[..., 7:8] * b[..., 7:8]], axis=-1)


def inv(a):
    qc = a[..., :4] * np.array([-1, -1, -1, 1], dtype=a.dtype)
    t = quat_rot(qc, (-1 / a[..., 7:8]) * a[..., 4:7])
    return np.concatenate([qc, t, 1 / a[..., 7:8]], axis=-1)


def _skew(w):
    W = np.zeros(w.shape[:-1] + (3, 3), dtype=w.dtype)
    W[..., 0, 1] = -w[..., 2]; W[..., 0, 2] = w[..., 1]
    W[..., 1, 0] = w[..., 2]; W[..., 1, 2] = -w[..., 0]
    W[..., 2, 0] = -w[..., 1]; W[..., 2, 1] = w[..., 0]
    return W


def w_coeffs(sigma, s, theta, small_theta, o):
    """A, B, C of W = A Omega + B Omega^2 + C I, the four branches of sim3_math.hpp (|sigma| < eps or not, small theta
    or not; fixb: the exact small-theta limit of B instead of the as-written one)."""
    one = sigma.dtype.type(1)
    small_sigma = np.abs(sigma) < o["eps"]
    th = np.where(small_theta, one, theta)
    sg = np.where(small_sigma, one, sigma)
    th2 = th * th
    A0 = np.where(small_theta, one / 2, (1 - np.cos(th)) / th2)
    B0 = np.where(small_theta, one / 6, (th - np.sin(th)) / (th2 * th))
    C1 = (s - 1) / sg
    sg2 = sg * sg
    A1s = ((sg - 1) * s + 1) / sg2
    B1s = ((sg2 / 2 - sg + 1) * s - (1 if o["fixb"] else 0)) / (sg2 * sg)
    a, b, c = s * np.sin(th), s * np.cos(th), th2 + sg2
    A1 = (a * sg + (1 - b) * th) / (th * c)
    B1 = (C1 - ((b - 1) * sg + a * th) / c) / th2
    return (np.where(small_sigma, A0, np.where(small_theta, A1s, A1)),
            np.where(small_sigma, B0, np.where(small_theta, B1s, B1)), np.where(small_sigma, one, C1))


def exp(xi, o, dt):
    xi = _c(xi, dt)
    om, up, sigma = xi[..., :3], xi[..., 3:6], xi[..., 6]
    theta = np.sqrt((om * om).sum(-1))
    small = theta < o["eps"]
    Om = _skew(om)
    Om2 = Om @ Om
    s = np.exp(sigma)
    A, B, Cc = w_coeffs(sigma, s, theta, small, o)
    th = np.where(small, dt(1), theta)
    k1 = np.where(small, dt(1), np.sin(th) / th)
    k2 = np.where(small, dt(0.5 if o["half"] else 1), (1 - np.cos(th)) / (th * th))
    I = np.eye(3, dtype=dt)
    Rm = I + k1[..., None, None] * Om + k2[..., None, None] * Om2
    W = A[..., None, None] * Om + B[..., None, None] * Om2 + Cc[..., None, None] * I
    t = (W * up[..., None, :]).sum(-1)
    return np.concatenate([quat_from_R(Rm), t, s[..., None]], axis=-1)


def solve3(W, t):
    """W x = t by Gaussian elimination with partial pivoting (first row of maximal magnitude), batched."""
    M = np.concatenate([W, t[..., None]], axis=-1).reshape(-1, 3, 4).copy()
    n = M.shape[0]
    ar = np.arange(n)
    for c in range(2):
        p = np.argmax(np.abs(M[:, c:, c]), axis=1) + c
        rc, rp = M[ar, c].copy(), M[ar, p].copy()
        M[ar, c], M[ar, p] = rp, rc
        for r in range(c + 1, 3):
            f = M[:, r, c] / M[:, c, c]
            M[:, r, c:] -= f[:, None] * M[:, c, c:]
    x = np.empty((n, 3), dtype=M.dtype)
    for i in (2, 1, 0):
        acc = M[:, i, 3].copy()
        for j in range(i + 1, 3):
            acc -= M[:, i, j] * x[:, j]
        x[:, i] = acc / M[:, i, i]
    return x.reshape(t.shape)


def log(S, o, dt):
    S = _c(S, dt)
    s = S[..., 7]
    sigma = np.log(s)
    Rm = R_from_quat(S[..., :4])
    d = (Rm[..., 0, 0] + Rm[..., 1, 1] + Rm[..., 2, 2] - 1) / 2
    dR = np.stack([Rm[..., 2, 1] - Rm[..., 1, 2], Rm[..., 0, 2] - Rm[..., 2, 0], Rm[..., 1, 0] - Rm[..., 0, 1]], axis=-1)
    small = d > 1 - dt(o["eps"])
    with np.errstate(invalid="ignore", divide="ignore"):
        dc = np.where(small, dt(0), d)
        theta = np.where(small, dt(0), np.arccos(dc))
        k = np.where(small, dt(0.5), theta / (2 * np.sqrt(1 - dc * dc)))
    om = k[..., None] * dR
    A, B, Cc = w_coeffs(sigma, s, theta, small, o)
    Om = _skew(om)
    W = A[..., None, None] * Om + B[..., None, None] * (Om @ Om) + Cc[..., None, None] * np.eye(3, dtype=dt)
    up = solve3(W, S[..., 4:7])
    return np.concatenate([om, up, sigma[..., None]], axis=-1)


def edge_error(C, S0, S1, o, dt):
    """EdgeSim3::computeError: e = log(C S0 S1^-1)"""
    return log(mul(mul(_c(C, dt), _c(S0, dt)), inv(_c(S1, dt))), o, dt)


def log_branch(e, o):
    """(small theta, small sigma) of a residual: which of w_coeffs' four branches log took."""
    e = np.asarray(e, dtype=LD)
    th = np.sqrt((e[..., :3] ** 2).sum(-1))
    # log's own test is d > 1 - eps on d = cos(theta): theta < sqrt(2 eps)
    return np.cos(th) > 1 - LD(o["eps"]), np.abs(e[..., 6]) < o["eps"]


# ---------------------------------------------------------------------------------------------- Jacobians
def _with_e(Jc, e):
    return np.concatenate([Jc, e[:, None, :]], axis=1)


def numeric_jacobian(C, S0, S1, o, delta, dof_mask, dt, mut=None):
    """(edges, 15, 7): central differences with left perturbations exp(+-delta e_d) S, the quotient formed as
    (1 / (2 delta)) (e+ - e-); cleared bit d of dof_mask: column d of both endpoints is zero; column 14 = e."""
    C, S0, S1 = _c(C, dt), _c(S0, dt), _c(S1, dt)
    m = C.shape[0]
    J = np.zeros((m, 14, 7), dtype=dt)
    scalar = dt(1) / (2 * dt(delta))
    if mut == "half_factor":
        scalar = dt(1) / dt(delta)
    for d in range(7):
        if not (dof_mask >> d) & 1 and mut != "frozen_nonzero":
            continue
        xi = np.zeros(7, dtype=dt)
        xi[d] = dt(delta)
        Pp, Pm = exp(xi, o, dt), exp(-xi, o, dt)
        if mut == "delta_swapped":
            Pp, Pm = Pm, Pp
        for end in range(2):
            S = S0 if end == 0 else S1
            Sp, Sm = (mul(S, Pp), mul(S, Pm)) if mut == "right_perturbation" else (mul(Pp, S), mul(Pm, S))
            ep = edge_error(C, Sp, S1, o, dt) if end == 0 else edge_error(C, S0, Sp, o, dt)
            em = edge_error(C, Sm, S1, o, dt) if end == 0 else edge_error(C, S0, Sm, o, dt)
            J[:, 7 * end + d] = scalar * (ep - em)
    return _with_e(J, edge_error(C, S0, S1, o, dt))


GL_U = (0.009219682876640375, 0.04794137181476257, 0.11504866290284765, 0.2063410228566913, 0.3160842505009099,
        0.43738329574426554, 0.5626167042557345, 0.6839157494990901, 0.7936589771433087, 0.8849513370971523,
        0.9520586281852375, 0.9907803171233597)  # the 12-node Gauss-Legendre rule on [0, 1] (Abramowitz & Stegun 25.4.30)
GL_W = (0.023587668193255914, 0.05346966299765921, 0.08003916427167311, 0.10158371336153296, 0.1167462682691774,
        0.12457352290670139)


def exp_exact(xi, u, dt):
    """exp(u xi) as (R, t, s): the exact map, no branch thresholds (sim3_jac.hpp): A, B, C through the power series of
    phi(z) = (e^z - 1) / z for |z| < 1, the rearranged closed forms beyond."""
    om, up, sigma = u * xi[..., :3], u * xi[..., 3:6], u * xi[..., 6]
    theta = np.sqrt((om * om).sum(-1))
    Om = _skew(om)
    Om2 = Om @ Om
    z = theta == 0
    ths = np.where(z, dt(1), theta)
    sinc = np.where(z, dt(1), np.sin(ths) / ths)
    h = np.where(z, dt(0.5), 2 * (np.sin(ths / 2) / ths) ** 2)
    s = np.exp(sigma)
    th2 = theta * theta
    rho2 = th2 + sigma * sigma
    p, q, r, sg, f = np.ones_like(theta), np.zeros_like(theta), np.zeros_like(theta), np.ones_like(theta), dt(1)
    As, Bs, Cs = np.zeros_like(theta), np.zeros_like(theta), np.zeros_like(theta)
    for n in range(20 if dt is np.float64 else 26):  # (long double: terms below 1e-21)
        Cs = Cs + sg * f
        As = As + q * f
        Bs = Bs + r * f
        p, q, r = sigma * p - th2 * q, p + sigma * q, sigma * r + q
        sg = sg * sigma
        f = f / dt(n + 2)
    big = rho2 >= 1
    rs = np.where(big, rho2, dt(1))
    sgs = np.where(sigma == 0, dt(1), sigma)
    Cc = np.where(sigma == 0, dt(1), np.expm1(sgs) / sgs)
    Ac = (s * sinc * sigma + ((1 - s) + s * th2 * h)) / rs
    Bc = (Cc + s * sigma * h - s * sinc) / rs
    A, B, Cf = np.where(big, Ac, As), np.where(big, Bc, Bs), np.where(big, Cc, Cs)
    I = np.eye(3, dtype=dt)
    Rm = I + sinc[..., None, None] * Om + h[..., None, None] * Om2
    W = A[..., None, None] * Om + B[..., None, None] * Om2 + Cf[..., None, None] * I
    return Rm, (W * up[..., None, :]).sum(-1), s


def adjoint(Rm, t, s):
    """Ad_S = [[R, 0, 0], [[t]x R, s R, -t], [0, 0, 1]]"""
    Ad = np.zeros(Rm.shape[:-2] + (7, 7), dtype=Rm.dtype)
    Ad[..., :3, :3] = Rm
    Ad[..., 3:6, :3] = _skew(t) @ Rm
    Ad[..., 3:6, 3:6] = s[..., None, None] * Rm
    Ad[..., 3:6, 6] = -t
    Ad[..., 6, 6] = 1
    return Ad


def left_jacobian(xi, dt):
    """J_l(xi) = int_0^1 Ad_exp(u xi) du by the 12-node rule, summed in node order."""
    Jl = np.zeros(xi.shape[:-1] + (7, 7), dtype=dt)
    for k in range(12):
        w = dt(GL_W[min(k, 11 - k)])
        Jl = Jl + w * adjoint(*exp_exact(xi, dt(GL_U[k]), dt))
    return Jl


def analytic_jacobian(C, S0, S1, o, dof_mask, dt):
    """(edges, 15, 7): J0 = J_l(e)^-1 Ad_C, J1 = -J_l(e)^-1 Ad_exp(e) by block substitution (3 x 3 pivoted solves with
    J_SO3 and V); frozen columns zero; column 14 = e."""
    C, S0, S1 = _c(C, dt), _c(S0, dt), _c(S1, dt)
    e = edge_error(C, S0, S1, o, dt)
    Jl = left_jacobian(e, dt)
    AdC = adjoint(R_from_quat(C[:, :4]), C[:, 4:7], C[:, 7])
    AdE = adjoint(*exp_exact(e, dt(1), dt))
    Y = np.concatenate([AdC, -AdE], axis=-1)  # (m, 7, 14)
    J = np.zeros((C.shape[0], 14, 7), dtype=dt)
    for c in range(14):
        if not (dof_mask >> (c % 7)) & 1:
            continue
        y = Y[:, :, c]
        x0 = solve3(Jl[:, :3, :3], y[:, :3])
        r = y[:, 3:6] - (Jl[:, 3:6, :3] * x0[:, None, :]).sum(-1) - Jl[:, 3:6, 6] * y[:, 6:7]
        J[:, c, :3] = x0
        J[:, c, 3:6] = solve3(Jl[:, 3:6, 3:6], r)
        J[:, c, 6] = y[:, 6]
    return _with_e(J, e)


# ---------------------------------------------------------------------------------------------- robust kernels
def robustify(kind, delta, e2, dt):
    """(rho, w = rho') of robust.hpp's table, per edge; kind and delta arrays."""
    kind = np.asarray(kind)
    d = _c(delta, dt)
    e2 = _c(e2, dt)
    one = dt(1)
    ds = np.where(kind == 0, one, d)  # (NONE carries delta 0)
    d2 = ds * ds
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        sq = np.sqrt(e2)
        sqs = np.where(sq == 0, one, sq)
        inl = e2 <= d2
        r2 = np.sqrt(1 + e2 / d2)
        a3 = 1 + e2 / d2
        a4 = ds + e2
        x5 = np.exp(-e2 / d2)
        a6 = sq / ds
        a7 = 1 - e2 / d2
        s9 = 2 * ds / (ds + e2)
        table = {
            0: (e2, np.ones_like(e2)),
            1: (np.where(inl, e2, 2 * sq * ds - d2), np.where(inl, one, ds / sqs)),
            2: (2 * d2 * (r2 - 1), 1 / r2),
            3: (d2 * np.log(a3), 1 / a3),
            4: (ds * e2 / a4, d2 / (a4 * a4)),
            5: (d2 * (1 - x5), x5),
            6: (2 * d2 * (a6 - np.log(1 + a6)), 1 / (1 + a6)),
            7: (np.where(inl, d2 / 3 * (1 - a7 * a7 * a7), d2 / 3), np.where(inl, a7 * a7, dt(0))),
            8: (np.where(inl, e2, d2), np.where(inl, one, dt(0))),
            9: (np.where(s9 >= 1, e2, s9 * s9 * e2), np.where(s9 >= 1, one, s9 * s9)),
        }
    rho, w = np.empty_like(e2), np.empty_like(e2)
    for k, (r_, w_) in table.items():
        rho[kind == k] = r_[kind == k]
        w[kind == k] = w_[kind == k]
    return rho, w


def chi_rho_w(e, Om, kind, delta, dt, mut=None):
    """(e^T Omega e, rho, w) per edge; Om None: the identity; kind None: no kernels."""
    e = _c(e, dt)
    chi = (e * e).sum(-1) if Om is None or mut == "w_from_ee" else np.einsum("kr,krc,kc->k", e, _c(Om, dt), e)
    if kind is None:
        return chi, chi.copy(), np.ones_like(chi)
    rho, w = robustify(kind, delta, chi, dt)
    return chi, rho, w


# ---------------------------------------------------------------------------------------------- the Gram phase
TRI = [(m, M) for M in range(7) for m in range(M + 1)]  # the scratch order of the upper triangle


def gram(J, w, Om, dt, mut=None):
    """G = w [J | e]^T Omega [J | -e] per edge, (edges, 14, 15) with column 14 = -w J^T Omega e, and its magnitude
    (every term in absolute value).  J, w, Omega are inputs: the device's own, bit for bit, in the derived checks."""
    J, w = _c(J, dt), _c(w, dt)
    if Om is None:
        OJ, OJm = J, np.abs(J)
    else:
        Om = _c(Om, dt)
        OJ = np.einsum("krc,kac->kar", Om, J)
        OJm = np.einsum("krc,kac->kar", np.abs(Om), np.abs(J))
    G = np.einsum("kar,kbr->kab", J[:, :14], OJ)
    Gm = np.einsum("kar,kbr->kab", np.abs(J[:, :14]), OJm)
    ww = w * w if mut == "w_twice" else w
    G, Gm = ww[:, None, None] * G, np.abs(ww)[:, None, None] * Gm
    if mut != "b_sign":
        G[:, :, 14] = -G[:, :, 14]
    return G, Gm


def edge_stores(G, mut=None):
    """What an edge's Gram matrix becomes: H01 and H10 as blocks [r, c], the two incidences' 35 scratch values."""
    H01 = G[:, :7, 7:14]
    H10 = H01 if mut == "h10_untransposed" else H01.transpose(0, 2, 1)
    tri = TRI[1:] + TRI[:1] if mut == "tri_off_by_one" else TRI
    tr = np.array([t[0] for t in tri])
    tc = np.array([t[1] for t in tri])
    s0 = np.concatenate([G[:, tr, tc], G[:, :7, 14]], axis=1)
    s1 = np.concatenate([G[:, 7 + tr, 7 + tc], G[:, 7:14, 14]], axis=1)
    if mut == "inc_swapped":
        s0, s1 = s1, s0
    return H01, H10, s0, s1


def dense_system(G, v0, v1, hidx, nb, dt):
    """Dense (H, b) of the edges' Gram matrices (tests/test_lm_ref.py: against the oracle's)."""
    H, b = np.zeros((nb, 7, nb, 7), dtype=dt), np.zeros((nb, 7), dtype=dt)
    for k in range(G.shape[0]):
        h = (hidx[v0[k]], hidx[v1[k]])
        for i in range(2):
            if h[i] < 0:
                continue
            b[h[i]] += G[k, 7 * i:7 * i + 7, 14]
            for j in range(2):
                if h[j] >= 0:
                    H[h[i], :, h[j], :] += G[k, 7 * i:7 * i + 7, 7 * j:7 * j + 7]
    return H.reshape(7 * nb, 7 * nb), b.reshape(-1)


def row_sums(scratch, incptr, dt, mut=None):
    """(sums, magnitudes, counts) per block row of the 35 scratch values of its incidences."""
    sc = _c(scratch, dt)
    nb = incptr.shape[0] - 1
    out, mag = np.zeros((nb, 35), dtype=dt), np.zeros((nb, 35), dtype=dt)
    cnt = np.diff(incptr)
    row = np.repeat(np.arange(nb), cnt)
    keep = np.ones(sc.shape[0], dtype=bool)
    if mut == "inc_dropped":
        keep[incptr[1:][cnt > 1] - 1] = False
    np.add.at(out, row[keep], sc[keep])
    np.add.at(mag, row[keep], np.abs(sc[keep]))
    return out, mag, cnt


def diag_block(row35):
    """(rows, 7, 7) symmetric blocks and (rows, 7) b of the row sums."""
    n = row35.shape[0]
    D = np.empty((n, 7, 7), dtype=row35.dtype)
    for t, (m, M) in enumerate(TRI):
        D[:, m, M] = row35[:, t]
        D[:, M, m] = row35[:, t]
    return D, row35[:, 28:]


def trace_and_max(D, dt, mut=None):
    """(trace, its magnitude, max |H_dd|) of the diagonal blocks (rows, 7, 7)."""
    dg = _c(np.diagonal(D, axis1=1, axis2=2), dt)
    mx = np.abs(_c(D, dt)).max() if mut == "max_over_H" else np.abs(dg).max()
    return dg.sum(), np.abs(dg).sum(), mx


# ---------------------------------------------------------------------------------------------- the update
def oplus(states, x, hidx, o, dt, mut=None):
    """S <- exp(dx) S for the free vertices (hidx >= 0: the block row whose 7 entries of x are the step)."""
    S = _c(states, dt).copy()
    free = hidx >= 0
    P = exp(_c(x, dt).reshape(-1, 7)[hidx[free]], o, dt)
    S[free] = mul(S[free], P) if mut == "oplus_right" else mul(P, S[free])
    return S


def scale_terms(x, b, lam, dt, mut=None):
    """(sum, magnitude) of x_j (lambda x_j + b_j)."""
    x, b = _c(x, dt), _c(b, dt)
    lam = dt(0) if mut == "scale_no_lambda" else dt(lam)
    return (x * (lam * x + b)).sum(), (np.abs(x) * (np.abs(lam * x) + np.abs(b))).sum()


# ---------------------------------------------------------------------------------------------- the comparisons
# Roundings on the longest path to an entry, for ANY summation order and any FMA contraction (a product is one rounding,
# a sum of T terms at most T - 1 more; an FMA only removes roundings):
K_GRAM = 8        # no Omega: 7 products (1) summed (6), times w (1)
K_GRAM_INFO = 15  # Omega J: 7 products summed (7); times J (1), 7 of those summed (6); times w (1)
k_row = lambda n: np.maximum(np.asarray(n) - 1, 0)  # n stored values added; one incidence: a copy, exact
k_trace = lambda nb: 7 * nb - 1                     # 7 nb diagonal entries added
k_sum = lambda n, per_term: n + per_term            # n terms of per_term roundings each, summed (n - 1)
K_SCALE_TERM = 3                                    # lambda x (1), + b (1), times x (1)


def derived_ratio(dev, ref, mag, k):
    """max over the entries of |dev - ref| / (gamma(k) mag); an entry whose bound is zero must be exact."""
    err = np.abs(np.asarray(dev, dtype=LD) - np.asarray(ref, dtype=LD))
    tol = np.broadcast_to(gamma_k(k), err.shape) * np.asarray(mag, dtype=LD)
    assert (err[tol == 0] == 0).all(), "an entry with a zero bound is not exact"
    return float((err[tol > 0] / tol[tol > 0]).max()) if (tol > 0).any() else 0.0


def edge_scaled_err(a, ref, floor=None):
    """Per edge: max |a - ref| over the edge's entries, relative to the edge's own largest |ref| (not below `floor`)."""
    ref = np.asarray(ref, dtype=LD).reshape(ref.shape[0], -1)
    a = np.asarray(a, dtype=LD).reshape(ref.shape)
    sc = np.abs(ref).max(1)
    if floor is not None:
        sc = np.maximum(sc, LD(floor))
    sc = np.where(sc == 0, LD(1), sc)
    return (np.abs(a - ref).max(1) / sc).astype(np.float64)


ILL = 1024 * U  # an edge whose float64 RESIDUAL is further than this from long double amplifies rounding: set apart


def ill_edges(e64, eld):
    """Edges whose residual the formulas themselves cannot deliver to rounding level (the cancellation near the exp /
    log branch thresholds that test_residuals_all_branches documents; the as-written B), from the restatement alone."""
    return edge_scaled_err(e64, eld, 1.0) > ILL


def ill_level(mode, delta=0.0):
    """Restatement noise of a Jacobian above which an edge is set apart like an ill-conditioned residual.  Closed form:
    ILL, as for e.  Central differences divide the residuals' rounding (~u) by 2 delta: 1024 u / (2 delta); an edge
    beyond that has a perturbed residual on the other side of a branch threshold of exp / log, or cancels."""
    return ILL if mode == "analytic" else ILL / (2 * delta)


def measured_ratio(dev, z64, zld, ill, floor=None, ill_above=None):
    """The measured convention, edge by edge: every edge's error relative to ITS OWN largest entry, so that a weak or
    small edge is held as tightly as the largest.  noise = the float64 restatement's largest such error, floored at 4u,
    tolerance 32 x noise.  The edges of `ill` (ill_edges), and those whose own restatement noise is above `ill_above`
    (ill_level), are gauged among themselves.  Returns dict(noise, ratio, n_ill, noise_ill, ratio_ill); a ratio <= 1
    passes."""
    n64 = edge_scaled_err(z64, zld, floor)
    dv = edge_scaled_err(dev, zld, floor)
    if ill_above is not None:
        ill = ill | (n64 > ill_above)
    out = dict(n_ill=int(ill.sum()), noise_ill=0.0, ratio_ill=0.0, noise=4 * U, ratio=0.0)
    if (~ill).any():
        out["noise"] = max(float(n64[~ill].max()), 4 * U)
        out["ratio"] = float(dv[~ill].max()) / (32 * out["noise"])
    if ill.any():
        out["noise_ill"] = max(float(n64[ill].max()), 4 * U)
        out["ratio_ill"] = float(dv[ill].max()) / (32 * out["noise_ill"])
    return out
