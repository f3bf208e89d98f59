"""Plain numpy restatement of the PCG's own operator and recurrence -- the block-CSR product q = (H + lambda I) p of
k_spmv_span MODE 0 (spmv_kernel.hpp) and the single-reduction iteration of k_pcg_init / k_pcg_step (pcg_kernels.hpp;
templates on the number K of systems) -- written from the comments of those files, with no product code.
dtype-generic like amg_ref.py: np.longdouble is the reference the device is compared with, np.float64 the noise gauge
of the iterates (tests/test_gpu_pcg_operator.py).

Three parts:
  bcsr_apply ...... the product on the device's own pattern and values, with the entrywise magnitude
                    |A||p| + |lambda||p| the derived bound of the GPU test needs.
  pcg ............. the recurrence; returns every iterate.
  span_model ...... a walk over spans, chunks of CH blocks and 64-wide windows that reproduces the kernel's INDEX
                    logic (what is read from where, and when) and otherwise computes the same product; `defect` names
                    ONE deliberate slip of that logic (SPAN_DEFECTS), `mut` of pcg one slip of the recurrence
                    (PCG_DEFECTS).  tests/test_pcg_ref.py shows that the comparisons the GPU tests make separate each
                    of them from rounding.

What each defect stands for (lines of k_spmv_span unless stated):
  skip_64, dup_64 ........ the consumption loop `for u < CH: kk = k + u ... acc += vc[u] * x` at the first block of the
                           second window (kk - k0 == 64): the hand-over `vc[u] = vn[u]`, `xgc = xgn` across a window
                           change loses or repeats a block.
  window_stale ........... `if (kn - cbase >= 64) { cbase += 64; cv = cvn; cvn = ... }`: cbase advances, cv does not,
                           so `__shfl(cv, kk - cbase)` returns columns of the previous window.
  rowend_no_refill ....... `if (row - rbase >= 64) { rbase += 64; rpv = ... rowptr[rbase + 1 + lane] ... }` in
                           next_row: rbase advances, the row-end table is not reloaded.
  last_block_clamp ....... `kk = ks + u < kend ? ks + u : kend - 1` in load_chunk and gather, applied one short: the
                           span's last block is replaced by the one before it.
  lam_skip_last_row ...... `y += lam[s] * pi` in the row_end that follows the loop (the span's last row).
  lam_prev_p ............. `pi_n[s] = xget(...)` in row_begin: the row's own entries of p are not refreshed, so the
                           damping term uses the previous row's.
  first_row_chunk_pos .... `row_begin(row, kbeg - k0, xgc)`: the position of the span's first block inside its chunk,
                           taken as if chunks were aligned to multiples of CH (kbeg % CH).
  batch_lambda0 .......... `lam[s] = sc[s].lambda`: system s of a batch reads system 0's damping.
  empty_span_shift ....... `rA = wrow[w], rB = wrow[w + 1]` with `if (rA < rB)`: an empty span is counted as one row,
                           and every span after it starts and ends one row late (the row after the hole is never
                           written).
  beta_parity ............ k_pcg_step `beta = gamma / sc->rz[par]` reading sc->rz[par ^ 1].
  s_stale ................ k_pcg_step `sv[j] = sn` left out.
  z_prev ................. k_pcg_step `zout[j] = zv` one iteration late (the SpMV multiplies the previous z).
  alpha_old_stale ........ k_pcg_step `sc->alpha[par ^ 1] = alpha` left out.
  cap_plus_one ........... k_pcg_step `if (itn >= sc->max_iter) sc->stop = 1` (or the replay's count) one late.
"""
import numpy as np

import amg_ref as R

LD, U = R.LD, R.U

SPAN_DEFECTS = ("skip_64", "dup_64", "window_stale", "rowend_no_refill", "last_block_clamp", "lam_skip_last_row",
                "lam_prev_p", "first_row_chunk_pos", "batch_lambda0", "empty_span_shift")
PCG_DEFECTS = ("beta_parity", "s_stale", "z_prev", "alpha_old_stale", "cap_plus_one")


def gamma_k(k):
    """gamma(k) = k u / (1 - k u) in long double (Higham's constant of a sum of k rounded terms)."""
    ku = LD(k) * LD(U)
    return ku / (1 - ku)


# ---------------------------------------------------------------------------------------------- the product
def bcsr_apply(rowptr, colidx, blocks, lam, p, dt=LD):
    """(q, mag): q = A p + lam p and mag = |A||p| + |lam||p| on the given block-CSR pattern (blocks [k, r, c]; a column
    that occurs twice in a row is two blocks).  p: (n,) with a scalar lam or (m, n) with a scalar or m dampings."""
    rowptr, colidx = np.asarray(rowptr), np.asarray(colidx)
    nb = rowptr.shape[0] - 1
    B = np.asarray(blocks, dtype=dt)
    x = np.asarray(p, dtype=dt)
    one = x.ndim == 1
    x = np.atleast_2d(x).reshape(-1, nb, 7)
    lam = np.broadcast_to(np.asarray(lam, dtype=dt), (x.shape[0],)).reshape(-1, 1, 1)
    rows = R._row_of_block(rowptr)
    q = np.zeros_like(x)
    mag = np.zeros_like(x)
    Ba = np.abs(B)
    for s in range(x.shape[0]):  # (per vector: the temporaries stay small)
        xs = x[s][colidx]
        np.add.at(q[s], rows, np.einsum("krc,kc->kr", B, xs))
        np.add.at(mag[s], rows, np.einsum("krc,kc->kr", Ba, np.abs(xs)))
    q = q + lam * x
    mag = mag + np.abs(lam) * np.abs(x)
    q, mag = q.reshape(x.shape[0], -1), mag.reshape(x.shape[0], -1)
    return (q[0], mag[0]) if one else (q, mag)


def blocks_per_row(rowptr):
    """Stored blocks of the block row every scalar row belongs to, (7 nb,)."""
    return np.repeat(np.diff(np.asarray(rowptr)), 7)


# ---------------------------------------------------------------------------------------------- the recurrence
def pcg(rowptr, colidx, blocks, b, lam, max_iter, rel_tol, dt=LD, mut=None):
    """Single-reduction PCG on (A + lam I) x = b with Minv = (D + lam I)^-1 per block row, as k_pcg_init / k_pcg_step:
         x = 0, r = b, z = Minv r, p = s = 0
         per iteration: w = (A + lam I) z, delta = w.z, gamma = r.z;  stop if gamma <= tol^2 gamma_0;
                        beta = gamma / gamma_old (0 first), alpha = gamma / (delta - beta gamma / alpha_old) (delta first)
                        p = z + beta p, s = w + beta s, x += alpha p, r -= alpha s, z = Minv r
    Returns dict(x = [x_1 ... x_iters], gamma = [gamma_0 ...] (the gamma every executed test saw), iters, rel_res =
    sqrt(gamma seen by the last executed test or step / gamma_0), fail).  The iteration stops after max_iter steps."""
    rowptr = np.asarray(rowptr)
    A = np.asarray(blocks, dtype=dt)
    lam = dt(lam)
    D = A[rowptr[:-1]] + lam * np.eye(7, dtype=dt)
    Minv = R.small_inverse(D, dt)
    mv = lambda v: bcsr_apply(rowptr, colidx, A, lam, v, dt)[0]
    b = np.asarray(b, dtype=dt)
    x, r = np.zeros_like(b), b.copy()
    z = R._bmv(Minv, r)
    p, s = np.zeros_like(b), np.zeros_like(b)
    tol2 = dt(rel_tol) * dt(rel_tol)
    rz = [dt(0), dt(0)]      # sc->rz, sc->alpha: ping-pong by parity
    al = [dt(0), dt(0)]
    xs, gammas = [], []
    gamma0 = gam_last = dt(0)
    iters, fail, par = 0, False, 0
    z_in = z
    cap = max_iter + 1 if mut == "cap_plus_one" else max_iter
    with np.errstate(all="ignore"):
        for it in range(cap):
            w = mv(z_in)
            delta, gamma = w @ z_in, r @ z_in
            first = it == 0
            if first:
                gamma0 = gamma
            gammas.append(gamma)
            if not (gamma == gamma) or gamma < 0 or gamma <= tol2 * gamma0 or (first and gamma == 0):
                fail = bool(not (gamma == gamma) or gamma < 0)
                gam_last = gamma
                break
            beta = dt(0) if first else gamma / rz[par ^ 1 if mut == "beta_parity" else par]
            denom = delta if first else delta - beta * gamma / al[par]
            if not (denom > 0) or not np.isfinite(denom):
                fail = True
                break
            alpha = gamma / denom
            p = z_in + beta * p
            if mut != "s_stale":
                s = w + beta * s
            x = x + alpha * p
            r = r - alpha * s
            z_new = R._bmv(Minv, r)
            z_in = z if mut == "z_prev" else z_new  # (z_prev: the step's z reaches the SpMV one iteration late)
            z = z_new
            rz[par ^ 1] = gamma
            if mut != "alpha_old_stale":
                al[par ^ 1] = alpha
            gam_last = gamma
            iters = it + 1
            xs.append(x.copy())
            par ^= 1
    rel = np.sqrt(abs(gam_last) / gamma0) if gamma0 > 0 else dt(0)
    return dict(x=xs, gamma=gammas, iters=iters, rel_res=rel, fail=fail)


# ---------------------------------------------------------------------------------------------- the kernel's index logic
def span_model(rowptr, colidx, blocks, wrow, lam, p, CH=8, dt=LD, defect=None):
    """q (m, 7 nb) of m systems (p (m, 7 nb), lam (m,)) by the walk k_spmv_span makes: wavefront w owns the rows
    wrow[w] .. wrow[w + 1] - 1 and streams their blocks in chunks of CH, the chunk after the current one already
    loaded; column indices come from a 64-block window (cv, the next one in cvn), row ends from a 64-row table (rpv);
    a row ends when the stream reaches the next row's first block.  Rows no span covers stay zero."""
    rowptr, colidx, wrow = np.asarray(rowptr), np.asarray(colidx), np.asarray(wrow)
    nb = rowptr.shape[0] - 1
    B = np.asarray(blocks, dtype=dt)
    x = np.asarray(p, dtype=dt).reshape(-1, nb, 7)
    m = x.shape[0]
    lam = np.broadcast_to(np.asarray(lam, dtype=dt), (m,)).copy()
    if defect == "batch_lambda0":
        lam[:] = lam[0]
    q = np.zeros_like(x)
    lanes = np.arange(64)
    spans = [(int(wrow[w]), int(wrow[w + 1])) for w in range(wrow.shape[0] - 1)]
    if defect == "empty_span_shift":
        nonempty = [w for w, (a, c) in enumerate(spans) if a < c]
        holes = [w for w, (a, c) in enumerate(spans) if a == c and nonempty and nonempty[0] < w < nonempty[-1]]
        if holes:  # every span after the first interior hole starts and ends one row late
            h = holes[0]
            spans = spans[:h] + [(min(a + 1, nb), min(c + 1, nb)) if a < c else (a, c) for a, c in spans[h:]]
    for rA, rB in spans:
        if not rA < rB:
            continue
        kbeg, kend = int(rowptr[rA]), int(rowptr[rB])
        k0 = kbeg
        clamp = kend - 2 if (defect == "last_block_clamp" and kend - kbeg >= 2) else kend - 1

        def row_ends(rbase):
            idx = rbase + 1 + lanes
            return np.where(idx <= rB, rowptr[np.minimum(idx, rB)], kend)

        def window(cb):
            idx = cb + lanes
            return np.where(idx < kend, colidx[np.minimum(idx, kend - 1)], 0)

        def load(ks):  # the chunk's blocks and the shared gather of p, clamped at the span's end
            kk = np.minimum(ks + np.arange(CH), clamp)
            return B[kk], x[:, cv[kk - cbase]]  # (CH, 7, 7), (m, CH, 7)

        rbase, row = rA, rA
        rpv = row_ends(rbase)
        k1 = int(rpv[0])
        cbase = k0
        cv, cvn = window(cbase), window(cbase + 64)
        vc, xc = load(k0)
        u0 = kbeg % CH if defect == "first_row_chunk_pos" else kbeg - k0
        pi = xc[:, u0].copy()
        acc = np.zeros((m, 7), dtype=dt)

        def row_end(row, last):
            y = acc.copy()
            if not (last and defect == "lam_skip_last_row"):
                y = y + lam[:, None] * pi
            q[:, row] = y

        for k in range(k0, kend, CH):
            kn = k + CH
            if kn < kend:
                if kn - cbase >= 64:
                    cbase += 64
                    if defect != "window_stale":
                        cv = cvn
                    cvn = window(cbase + 64)
                vn, xn = load(kn)
            for u in range(CH):
                kk = k + u
                if not (kbeg <= kk < kend):
                    continue
                if kk == k1:
                    row_end(row, False)
                    row += 1
                    if defect != "lam_prev_p":
                        pi = xc[:, u].copy()
                    acc = np.zeros((m, 7), dtype=dt)
                    if row - rbase >= 64:
                        rbase += 64
                        if defect != "rowend_no_refill":
                            rpv = row_ends(rbase)
                    k1 = int(rpv[row - rbase])
                if kk - k0 == 64 and defect == "skip_64":
                    continue
                t = np.einsum("rc,sc->sr", vc[u], xc[:, u])
                acc = acc + t
                if kk - k0 == 64 and defect == "dup_64":
                    acc = acc + t
            if kn < kend:
                vc, xc = vn, xn
        row_end(row, True)
    return q.reshape(m, -1)
