"""Plain numpy restatement of the PCG's preconditioners -- the aggregation multigrid (amg_kernels.hpp, amg.hpp,
engine_amg.hip), the chain segments and block-Jacobi (pcg_kernels.hpp) -- written from the comments of those files,
with no product code.  dtype-generic: np.longdouble is the reference the device is compared with, np.float64 the
noise gauge (the same arithmetic in another summation order; tests/test_gpu_preconditioners.py).

Conventions: blocks are [k, r, c] (what Graph.get_system returns), states [qx qy qz qw tx ty tz s], tangent order
[omega upsilon sigma].  Level 0 = the LM system (rows may hold parallel blocks: the same column twice); level l + 1 =
P_l^T A_l P_l with P_0 = block rows Ad(S_v), P_l = identity blocks below; coarse pattern = diagonal first, then unique
ascending columns; W_{l+1} = sum P_l^T W_l P_l (W_0 = I); damping lambda W_l on the diagonal blocks;
Minv_l = omega (D_l + lambda W_l)^-1.

`mut` names ONE deliberate defect (MUTATIONS): the sensitivity table of tests/test_amg_ref.py shows that the
comparison the GPU tests make separates each of them from rounding.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53

MUTATIONS = ("galerkin_drop", "ad_sign", "omega1_l1", "damp_I", "over0_1.7", "over1_1.5", "visits_l1_once",
             "visits_l2_twice", "stale_fp32_diag", "restrict_no_P", "prolong_PT", "dense_tail",
             "chain_boundary", "chain_link_T")


def longdouble_ok():
    return np.finfo(LD).eps < 2e-19


# ---------------------------------------------------------------------------------------------- Ad(S)
def rot_from_quat(q, dt):
    """R of an UNNORMALISED quaternion exactly as sim3::R_from_quat writes it (no normalisation there)."""
    q = np.asarray(q, dtype=dt)
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    R = np.empty(q.shape[:-1] + (3, 3), dtype=dt)
    R[..., 0, 0] = 1 - 2 * (y * y + z * z); R[..., 0, 1] = 2 * (x * y - z * w); R[..., 0, 2] = 2 * (x * z + y * w)
    R[..., 1, 0] = 2 * (x * y + z * w); R[..., 1, 1] = 1 - 2 * (x * x + z * z); R[..., 1, 2] = 2 * (y * z - x * w)
    R[..., 2, 0] = 2 * (x * z - y * w); R[..., 2, 1] = 2 * (y * z + x * w); R[..., 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def _rot_abs(q, dt):
    """The same expressions with every term replaced by its absolute value."""
    q = np.abs(np.asarray(q, dtype=dt))
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    R = np.empty(q.shape[:-1] + (3, 3), dtype=dt)
    R[..., 0, 0] = 1 + 2 * (y * y + z * z); R[..., 0, 1] = 2 * (x * y + z * w); R[..., 0, 2] = 2 * (x * z + y * w)
    R[..., 1, 0] = 2 * (x * y + z * w); R[..., 1, 1] = 1 + 2 * (x * x + z * z); R[..., 1, 2] = 2 * (y * z + x * w)
    R[..., 2, 0] = 2 * (x * z + y * w); R[..., 2, 1] = 2 * (y * z + x * w); R[..., 2, 2] = 1 + 2 * (x * x + y * y)
    return R


def _skew(t):
    K = np.zeros(t.shape[:-1] + (3, 3), dtype=t.dtype)
    K[..., 0, 1] = -t[..., 2]; K[..., 0, 2] = t[..., 1]
    K[..., 1, 0] = t[..., 2]; K[..., 1, 2] = -t[..., 0]
    K[..., 2, 0] = -t[..., 1]; K[..., 2, 1] = t[..., 0]
    return K


def adjoint(states, dt, mut=None):
    """Ad(S) [n, 7, 7]:  [[R 0 0], [[t]x R, s R, -t], [0 0 1]]  (S exp(x) S^-1 = exp(Ad_S x))."""
    S = np.asarray(states, dtype=dt).reshape(-1, 8)
    R = rot_from_quat(S[:, :4], dt)
    t, s = S[:, 4:7], S[:, 7]
    A = np.zeros((S.shape[0], 7, 7), dtype=dt)
    A[:, :3, :3] = R
    A[:, 3:6, :3] = _skew(t) @ R
    A[:, 3:6, 3:6] = s[:, None, None] * R
    A[:, 3:6, 6] = t if mut == "ad_sign" else -t
    A[:, 6, 6] = 1
    return A


def adjoint_abs(states):
    """Every entry of Ad(S) with each term of its expression replaced by its absolute value, down to the quaternion
    products of R: the B of the bound |Ad_dev - Ad| <= 16 u B (zeros stay zero: those entries must be exact)."""
    S = np.asarray(states, dtype=LD).reshape(-1, 8)
    Ra = _rot_abs(S[:, :4], LD)
    t, s = np.abs(S[:, 4:7]), S[:, 7]
    B = np.zeros((S.shape[0], 7, 7), dtype=LD)
    B[:, :3, :3] = Ra
    B[:, 3:6, :3] = np.abs(_skew(t)) @ Ra  # |t1||R2c| + |t2||R1c|
    B[:, 3:6, 3:6] = s[:, None, None] * Ra
    B[:, 3:6, 6] = t
    B[:, 6, 6] = 1
    return B


# ---------------------------------------------------------------------------------------------- small inverses
def gj_inverse(a):
    """Unpivoted Gauss-Jordan inverse of [..., n, n] the way k_jacobi / k_chain_factor / gj_invert_rows eliminate."""
    a = np.array(a, copy=True)
    n = a.shape[-1]
    for k in range(n):
        d = 1 / a[..., k, k]
        rowk = a[..., k, :] * d[..., None]
        f = a[..., :, k].copy()
        a = a - f[..., :, None] * rowk[..., None, :]
        a[..., :, k] = -f * d[..., None]
        a[..., k, :] = rowk
        a[..., k, k] = d
    return a


def accurate_inverse(a, dt, steps=4):
    """Inverse to the precision of dt: LAPACK in float64, then corrections X <- X + X0 (I - A X) with the residual
    in dt and the (small) correction in float64; every step gains a factor ~ cond(A) u."""
    a = np.asarray(a, dtype=dt)
    x0 = np.linalg.inv(a.astype(np.float64))
    x = x0.astype(dt)
    if dt is not np.float64:
        eye = np.eye(a.shape[-1], dtype=dt)
        for _ in range(steps):
            x = x + (x0 @ (eye - a @ x).astype(np.float64)).astype(dt)
    return x


def refined_solve(A, X0, r, steps=4):
    """x = A^-1 r to the precision of A's dtype from a float64 inverse X0: x <- x + X0 (r - A x), matrix-vector
    products only (the long-double cycle needs the coarsest SOLVE, not the inverse)."""
    dt = A.dtype.type
    x = (X0 @ r.astype(np.float64)).astype(dt)
    for _ in range(steps):
        x = x + (X0 @ (r - A @ x).astype(np.float64)).astype(dt)
    return x


def small_inverse(a, dt):
    return gj_inverse(a) if dt is np.float64 else accurate_inverse(a, dt)


def pivot_schedule(nd, pivot):
    """Rows of the pivot blocks of the dense inverse: `pivot` (14 or 28) while they fit, then 14, then 7."""
    out, k0 = [], 0
    while k0 < nd:
        pb = pivot if nd - k0 >= pivot else (14 if nd - k0 >= 14 else 7)
        out.append(pb)
        k0 += pb
    return out


def block_gj_inverse(A, pivot, skip_last=False):
    """Block Gauss-Jordan without pivot search, out of place per step, as k_amg_dense_gj_step:
    P = A_kk^-1;  B_kk = P;  B_kj = P A_kj;  B_ik = -A_ik P;  B_ij = A_ij - A_ik (P A_kj)."""
    A = np.array(A, copy=True)
    nd = A.shape[0]
    sched = pivot_schedule(nd, pivot)
    if skip_last:
        sched = sched[:-1]
    k0 = 0
    for pb in sched:
        k = slice(k0, k0 + pb)
        P = gj_inverse(A[k, k])
        Rk = P @ A[k, :]
        Rk[:, k] = P
        Ck = A[:, k].copy()
        B = A.copy()
        B[:, k] = 0
        B = B - Ck @ Rk
        B[k, :] = Rk
        A = B
        k0 += pb
    return A


# ---------------------------------------------------------------------------------------------- hierarchy
def _row_of_block(rowptr):
    return np.repeat(np.arange(rowptr.shape[0] - 1), np.diff(rowptr))


def coarse_pattern(rows, cols, agg):
    """Pattern of P^T A P: per coarse row the diagonal first, then unique ascending columns.  Returns
    (rowptr, colidx, slot of every fine block in the coarse block list, fine blocks summed per coarse block)."""
    nc = int(agg.max()) + 1
    I, J = agg[rows].astype(np.int64), agg[cols].astype(np.int64)
    key = I * (nc + 1) + np.where(I == J, 0, J + 1)
    uk, slot, cnt = np.unique(key, return_inverse=True, return_counts=True)
    ci, cj = uk // (nc + 1), uk % (nc + 1)
    colidx = np.where(cj == 0, ci, cj - 1).astype(np.int32)
    rowptr = np.zeros(nc + 1, dtype=np.int32)
    np.add.at(rowptr, ci + 1, 1)
    return np.cumsum(rowptr).astype(np.int32), colidx, slot, cnt


def galerkin(blocks, rows, cols, agg, P, dt, drop=None):
    """Coarse blocks sum_k P_i^T A_k P_j in ascending fine-block order (P None: plain sums); returns
    (rowptr, colidx, coarse blocks, contributions per coarse block)."""
    rowptr, colidx, slot, cnt = coarse_pattern(rows, cols, agg)
    b = np.asarray(blocks, dtype=dt)
    contrib = b if P is None else np.einsum("kqr,kqc->krc", P[rows], np.einsum("krq,kqc->krc", b, P[cols]))
    if drop is not None:
        contrib = contrib.copy()
        contrib[drop] = 0
    C = np.zeros((colidx.shape[0], 7, 7), dtype=dt)
    np.add.at(C, slot, contrib)
    return rowptr, colidx, C, cnt


def wsum(src, agg, first, dt):
    """W_c[a] = sum over the members i of a, ascending, of P_i^T P_i (first) or W_f[i]."""
    src = np.asarray(src, dtype=dt)
    t = np.einsum("imr,imc->irc", src, src) if first else src
    W = np.zeros((int(agg.max()) + 1, 7, 7), dtype=dt)
    np.add.at(W, agg, t)
    return W


class Level:
    pass


def _f32(a, dt):
    return np.asarray(a).astype(np.float32).astype(dt)


def build(dt, rowptr, colidx, blocks, states_free, aggs, lam, omega=0.9, fp32=True, additive=False, pivot=14,
          mut=None, exact_inverse=False):
    """Levels of the hierarchy with their numbers for the damping `lam`.  aggs: aggregate of every row, per level
    but the coarsest.  Each level: nb, rowptr, colidx, rows, und (undamped blocks), vals (diagonal damped on coarse
    levels), cyc (what a matrix pass of the cycle reads), lamI (level 0: the scalar added by the pass), W, diagH,
    Minv ([i, r, c]), agg, P; the last level also A (dense) and Ainv -- in float64 by the kernels' block
    Gauss-Jordan; in long double the coarsest level is SOLVED by refinement (X0, refined_solve) and Ainv is formed
    only on request (exact_inverse: three n^3 products in long double)."""
    lam = dt(lam)
    levels = []
    rp, ci, und = np.asarray(rowptr), np.asarray(colidx), np.asarray(blocks, dtype=dt)
    P = adjoint(states_free, dt, mut)
    W = None
    for l in range(len(aggs) + 1):
        L = Level()
        L.nb, L.rowptr, L.colidx, L.rows, L.und = rp.shape[0] - 1, rp, ci, _row_of_block(rp), und
        L.agg = None if l == len(aggs) else np.asarray(aggs[l])
        L.P = P if l == 0 else None
        L.W, L.diagH = W, und[rp[:-1]]
        eye = np.broadcast_to(np.eye(7, dtype=dt), (L.nb, 7, 7))
        Wd = eye if (l == 0 or mut == "damp_I") else W
        D = L.diagH + lam * Wd
        L.vals = und.copy()
        if l > 0:
            L.vals[rp[:-1]] = D
        L.lamI = lam if l == 0 else dt(0)
        src = L.und if (l == 0 or mut == "stale_fp32_diag") else L.vals
        L.cyc = _f32(src, dt) if fp32 else (L.und if l == 0 else L.vals)
        om = 1.0 if (l == 0 and additive) or (l == 1 and mut == "omega1_l1") else omega
        L.Minv = dt(om) * small_inverse(D, dt)
        levels.append(L)
        if L.agg is None:
            break
        drop = (und.shape[0] // 2) if (mut == "galerkin_drop" and l == 0) else None
        rp2, ci2, C, _ = galerkin(und, L.rows, ci, L.agg, L.P, dt, drop)
        W = wsum(P if l == 0 else W, L.agg, l == 0, dt)
        rp, ci, und = rp2, ci2, C
    Lc = levels[-1]
    Lc.A = dense_of(Lc.nb, Lc.rows, Lc.colidx, Lc.vals, dt)
    if mut == "dense_tail":
        assert Lc.nb % 2 == 1, "the 7-row tail exists only for an odd number of coarsest rows"
        Lc.Ainv = block_gj_inverse(Lc.A, pivot, skip_last=True)
    elif dt is np.float64:
        Lc.Ainv = block_gj_inverse(Lc.A, pivot)
    else:
        Lc.X0 = np.linalg.inv(Lc.A.astype(np.float64))
        Lc.Ainv = accurate_inverse(Lc.A, dt, steps=3) if exact_inverse else None
    return levels


def dense_of(nb, rows, cols, blocks, dt):
    A = np.zeros((nb, 7, nb, 7), dtype=dt)
    np.add.at(A, (rows, slice(None), cols, slice(None)), np.asarray(blocks, dtype=dt))
    return A.reshape(7 * nb, 7 * nb)


# ---------------------------------------------------------------------------------------------- the cycle
def _bmv(M, x):  # block-diagonal times vector
    return np.einsum("irc,ic->ir", M, x.reshape(-1, 7)).ravel()


def matvec(L, x):
    """One matrix pass of the cycle on level L: (cyc + lamI) x."""
    y = np.zeros((L.nb, 7), dtype=x.dtype)
    np.add.at(y, L.rows, np.einsum("krc,kc->kr", L.cyc, x.reshape(-1, 7)[L.colidx]))
    return y.ravel() + L.lamI * x


class Cycle:
    def __init__(self, levels, visits=(2, 3, 3, 3), over=(1.8, 1.6), over_on=True, additive=False, mut=None):
        self.lv, self.additive, self.mut = levels, additive, mut
        v = list(visits)
        if mut == "visits_l1_once":
            v[0] = 1
        if mut == "visits_l2_twice":
            v[1] = 2
        self.visits = [1] + [v[min(l - 1, 3)] for l in range(1, len(levels) + 1)]
        o0, o1 = (over if over_on else (1.0, 1.0))
        if mut == "over0_1.7":
            o0 = 1.7
        if mut == "over1_1.5":
            o1 = 1.5
        self.over = (o0, o1)

    def restrict(self, l, t):
        L = self.lv[l]
        t = t.reshape(-1, 7)
        if L.P is not None and self.mut != "restrict_no_P":
            t = np.einsum("imc,im->ic", L.P, t)
        out = np.zeros((self.lv[l + 1].nb, 7), dtype=t.dtype)
        np.add.at(out, L.agg, t)
        return out.ravel()

    def prolong(self, l, xc):
        L = self.lv[l]
        x = xc.reshape(-1, 7)[L.agg]
        if L.P is not None:
            x = np.einsum("icr,ic->ir" if self.mut == "prolong_PT" else "irc,ic->ir", L.P, x)
        return x.ravel()

    def coarse(self, l, rc):
        """Level l + 1 from the right-hand side rc: exact on the coarsest level, else visits[l + 1] cycles from the
        first iterate Minv rc with a smoothing pass between them."""
        Lc = self.lv[l + 1]
        if l + 2 == len(self.lv):
            return Lc.Ainv @ rc if Lc.Ainv is not None else refined_solve(Lc.A, Lc.X0, rc)
        res = self.cycle(l + 1, _bmv(Lc.Minv, rc), rc)
        for _ in range(1, self.visits[l + 1]):
            oth = res + _bmv(Lc.Minv, rc - matvec(Lc, res))
            res = self.cycle(l + 1, oth, rc)
        return res

    def cycle(self, l, cur, r):
        L = self.lv[l]
        t = r - matvec(L, cur)
        xc = self.coarse(l, self.restrict(l, t))
        cur = cur + r.dtype.type(self.over[0 if l == 0 else 1]) * self.prolong(l, xc)
        return cur + _bmv(L.Minv, r - matvec(L, cur))

    def apply(self, r):
        """z = M^-1 r.  Multiplicative: one cycle from Minv_0 r; additive: Minv_0 r + over_0 P_0 C P_0^T r."""
        z0 = _bmv(self.lv[0].Minv, r)
        if self.additive:
            xc = self.coarse(0, self.restrict(0, r))
            return z0 + r.dtype.type(self.over[0]) * self.prolong(0, xc)
        return self.cycle(0, z0, r)

    def dense(self):
        n = 7 * self.lv[0].nb
        dt = self.lv[0].und.dtype.type
        return np.stack([self.apply(e) for e in np.eye(n, dtype=dt)], axis=1)


# ---------------------------------------------------------------------------------------------- chain, Jacobi
def jacobi_apply(rowptr, blocks, lam, r, dt):
    D = np.asarray(blocks, dtype=dt)[np.asarray(rowptr)[:-1]] + dt(lam) * np.eye(7, dtype=dt)
    return _bmv(small_inverse(D, dt), np.asarray(r, dtype=dt))


def chain_links(rowptr, colidx, blocks, dt):
    """L_i = sum of ALL blocks between rows i and i - 1 (parallel edges keep separate blocks), zero if none."""
    rows = _row_of_block(np.asarray(rowptr))
    Lk = np.zeros((rowptr.shape[0] - 1, 7, 7), dtype=dt)
    sel = np.asarray(colidx) == rows - 1
    np.add.at(Lk, rows[sel], np.asarray(blocks, dtype=dt)[sel])
    return Lk


def chain_apply(rowptr, colidx, blocks, lam, seg, r, dt, mut=None):
    """z = M^-1 r, M = the block-tridiagonal part of H + lam I inside segments of `seg` rows, solved exactly by the
    block LDL^T recurrence:  S_i = D_i + lam I - G_i L_i^T,  G_i = L_i S_{i-1}^-1;  y_i = r_i - G_i y_{i-1};
    z_i = S_i^-1 y_i - G_{i+1}^T z_{i+1}."""
    nb = rowptr.shape[0] - 1
    D = np.asarray(blocks, dtype=dt)[np.asarray(rowptr)[:-1]] + dt(lam) * np.eye(7, dtype=dt)
    Lk = chain_links(rowptr, colidx, blocks, dt)
    if mut == "chain_link_T":
        Lk = Lk.transpose(0, 2, 1)
    starts = np.arange(0, nb, seg)
    if mut == "chain_boundary":
        starts = np.concatenate([[0], starts[1:] + 1])
        starts = starts[starts < nb]
    first = np.zeros(nb, dtype=bool)
    first[starts] = True
    r = np.asarray(r, dtype=dt).reshape(nb, 7)
    Sinv = np.zeros((nb, 7, 7), dtype=dt)
    G = np.zeros((nb, 7, 7), dtype=dt)
    y = np.zeros((nb, 7), dtype=dt)
    for i in range(nb):
        a = D[i]
        if not first[i]:
            G[i] = Lk[i] @ Sinv[i - 1]
            a = a - G[i] @ Lk[i].T
            y[i] = r[i] - G[i] @ y[i - 1]
        else:
            y[i] = r[i]
        Sinv[i] = small_inverse(a, dt)
    z = np.zeros((nb, 7), dtype=dt)
    for i in range(nb - 1, -1, -1):
        z[i] = Sinv[i] @ y[i]
        if i + 1 < nb and not first[i + 1]:
            z[i] = z[i] - G[i + 1].T @ z[i + 1]
    return z.ravel()


def chain_dense(rowptr, colidx, blocks, lam, seg):
    """The chain preconditioner's M assembled densely in long double (to check chain_apply itself)."""
    nb = rowptr.shape[0] - 1
    D = np.asarray(blocks, dtype=LD)[np.asarray(rowptr)[:-1]] + LD(lam) * np.eye(7, dtype=LD)
    Lk = chain_links(rowptr, colidx, blocks, LD)
    M = np.zeros((nb, 7, nb, 7), dtype=LD)
    for i in range(nb):
        M[i, :, i, :] = D[i]
        if i % seg:
            M[i, :, i - 1, :] = Lk[i]
            M[i - 1, :, i, :] = Lk[i].T
    return M.reshape(7 * nb, 7 * nb)


# ---------------------------------------------------------------------------------------------- helpers of the tests
def relerr(a, ref):
    """max-norm difference relative to the max norm of the reference."""
    ref = np.asarray(ref, dtype=LD)
    return float(np.abs(np.asarray(a, dtype=LD) - ref).max() / np.abs(ref).max())


def noise_and_tol(z64, zld):
    """(noise, tolerance): the float64 restatement's distance from long double, floored at 4u; the device must be
    within 32 x that of the long-double result."""
    noise = max(relerr(z64, zld), 4 * U)
    return noise, 32 * noise


def blocks_from_dense(H, rowptr, colidx):
    """Block-CSR values of a dense H on the given pattern: a column that occurs more than once in a row (parallel
    edges) gets the whole block in its first slot and zeros after it."""
    rows = _row_of_block(np.asarray(rowptr))
    H4 = np.asarray(H).reshape(rowptr.shape[0] - 1, 7, -1, 7)
    blk = H4[rows, :, colidx, :].copy()
    dup = np.zeros(rows.shape[0], dtype=bool)
    dup[1:] = (rows[1:] == rows[:-1]) & (np.asarray(colidx)[1:] == np.asarray(colidx)[:-1])
    blk[dup] = 0
    return blk
