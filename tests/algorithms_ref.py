"""numpy restatement of the Gauss-Newton and dogleg rules of DESIGN.md 5h (g2o's OptimizationAlgorithmGaussNewton and
OptimizationAlgorithmDogleg) on the CPU oracle: H and b from oracle.Graph.build_dense, chi2 from oracle.Graph.chi2,
a dense Cholesky solve (its failure is the factorisation's non-positive pivot), S <- exp(h) S through
oracle.sim3_exp / sim3_mul.  Test infrastructure only: tests/test_gpu_algorithms.py compares the library with it."""
import numpy as np

from oracle import oracle as O

STEP_SD, STEP_GN, STEP_DL = 1, 2, 3


def _oplus(OG, h, opt):
    free = np.flatnonzero(OG.fixed == 0)
    for k, v in enumerate(free):
        OG.states[v] = O.sim3_mul(O.sim3_exp(h[7 * k:7 * k + 7], opt), OG.states[v])


def _solve(H, b, lam):
    """(ok, x) of (H + lam I) x = b by Cholesky; ok False where the factorisation meets a non-positive pivot."""
    A = H + lam * np.eye(H.shape[0]) if lam else H
    try:
        Lc = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return False, None
    return True, np.linalg.solve(Lc.T, np.linalg.solve(Lc, b))


def gauss_newton(OG, iters, opt):
    """Runs in place on OG.states; returns (iterations, [dict(chi2_before, chi2_after)]) -- 0 iterations on Fail."""
    out = []
    for _ in range(iters):
        chi = OG.chi2(opt)
        H, b = OG.build_dense(opt)
        ok, x = _solve(H, b, 0.0)
        if not ok:
            out.append(dict(chi2_before=chi, chi2_after=chi))
            return 0, out
        _oplus(OG, x, opt)
        out.append(dict(chi2_before=chi, chi2_after=OG.chi2(opt)))
    return len(out), out


def dogleg(OG, iters, opt, delta_init=1e4, max_trials=100, lambda_init=1e-7, lambda_factor=10.0):
    """Runs in place on OG.states; returns (iterations, per-iteration dicts) -- 0 iterations on Fail."""
    delta, lam_c, was_pd = delta_init, lambda_init, True
    out = []
    for _ in range(iters):
        rec = dict(delta_before=delta, lambda_=0.0, chi2_before=None)
        chi = OG.chi2(opt)
        rec["chi2_before"] = chi
        H, b = OG.build_dense(opt)
        Hb = H @ b
        alpha = (b @ b) / (b @ Hb)
        hsd = alpha * b
        hsd_norm = np.linalg.norm(hsd)
        while True:
            lam = 0.0 if was_pd else lam_c
            ok, hgn = _solve(H, b, lam)
            was_pd = was_pd and ok
            if not was_pd:
                if ok:
                    rec["lambda_"] = lam
                    lam_c = max(1e-12, lam_c / (0.5 * lambda_factor))
                else:
                    lam_c *= lambda_factor
                    if lam_c > 1e3:
                        rec.update(chi2_after=chi, was_pd=was_pd, failed=True)
                        out.append(rec)
                        return 0, out
            if ok:
                break
        hgn_norm = np.linalg.norm(hgn)
        tries, good, rho = 0, False, 0.0
        while True:
            tries += 1
            if hgn_norm < delta:
                hdl, step = hgn, STEP_GN
            elif hsd_norm > delta:
                hdl, step = delta / hsd_norm * hsd, STEP_SD
            else:
                d = hgn - hsd
                c = hsd @ d
                bma2 = d @ d
                d2 = delta * delta - hsd @ hsd
                if c <= 0:
                    beta = (-c + np.sqrt(c * c + bma2 * d2)) / bma2
                else:
                    beta = d2 / (c + np.sqrt(c * c + bma2 * d2))
                hdl, step = hsd + beta * (hgn - hsd), STEP_DL
            gain = 2.0 * (b @ hdl) - hdl @ (H @ hdl)
            saved = OG.states.copy()
            _oplus(OG, hdl, opt)
            new = OG.chi2(opt)
            if abs(gain) < 1e-12:
                gain = 1e-12
            rho = (chi - new) / gain
            if rho > 0:
                chi, good = new, True
            else:
                OG.states[:] = saved
            if rho > 0.75:
                delta = max(delta, 3.0 * np.linalg.norm(hdl))
            elif rho < 0.25:
                delta *= 0.5
            if good or tries >= max_trials:
                break
        rec.update(chi2_after=chi, trials=tries, step=step, delta_after=delta, rho=rho, alpha=alpha,
                   norm_sd=hsd_norm, norm_gn=hgn_norm, norm_dl=np.linalg.norm(hdl), was_pd=was_pd)
        out.append(rec)
        if not good:
            break
    return len(out), out


# ---------------------------------------------------------------------------------------------- the dogleg's operators
# Restatements for tests/test_gpu_dogleg_operators.py and tests/test_dogleg_rule.py (dtype-generic, np.longdouble the
# reference): the six scalars of an iteration with their magnitudes, and the step rule of DESIGN.md 5h.
LD = np.longdouble


def dogleg_scalars(rowptr, colidx, blocks, b, g, j0=None, j1=None, dt=LD):
    """(values, magnitudes), six each in the device's order: b.b, b^T H b, g.g, b.g, (Hb).g, g^T H g.  The four dots
    of k_dl_dots (b.b, g.g, b.g, (Hb).g) run over the entries [j0, j1), the two quadratic forms over every row; a
    magnitude is the same sum with every term replaced by its absolute value (sum |v_i| |H_ij| |w_j|)."""
    import pcg_ref as P
    b, g = np.asarray(b, dtype=dt), np.asarray(g, dtype=dt)
    j0 = 0 if j0 is None else j0
    j1 = b.shape[0] if j1 is None else j1
    (Hb, Hg), (Mb, Mg) = P.bcsr_apply(rowptr, colidx, blocks, 0.0, np.stack([b, g]), dt)
    r = slice(j0, j1)
    ab, ag = np.abs(b), np.abs(g)
    val = [(b[r] * b[r]).sum(), (b * Hb).sum(), (g[r] * g[r]).sum(), (b[r] * g[r]).sum(), (Hb[r] * g[r]).sum(),
           (g * Hg).sum()]
    mag = [(b[r] * b[r]).sum(), (ab * Mb).sum(), (g[r] * g[r]).sum(), (ab[r] * ag[r]).sum(), (Mb[r] * ag[r]).sum(),
           (ag * Mg).sum()]
    return np.array(val, dtype=dt), np.array(mag, dtype=dt)


def dogleg_rule(s, delta, dt=LD):
    """The step rule of DESIGN.md 5h, item 4, from the six scalars: dict(alpha, norm_sd, norm_gn, step, ca, cg, beta,
    c, bma2, d2) for h_dl = ca b + cg h_gn (beta, c, bma2, d2: None unless a dogleg step)."""
    bb, bHb, gg, bg = (dt(x) for x in s[:4])
    delta = dt(delta)
    alpha = bb / bHb
    nsd, ngn = abs(alpha) * np.sqrt(bb), np.sqrt(gg)
    out = dict(alpha=alpha, norm_sd=nsd, norm_gn=ngn, beta=None, c=None, bma2=None, d2=None)
    if ngn < delta:
        out.update(step=STEP_GN, ca=dt(0), cg=dt(1))
    elif nsd > delta:
        out.update(step=STEP_SD, ca=delta / nsd * alpha, cg=dt(0))
    else:
        hsd2 = alpha * alpha * bb
        c = alpha * bg - hsd2
        bma2 = gg - 2 * alpha * bg + hsd2
        d2 = delta * delta - hsd2
        root = np.sqrt(c * c + bma2 * d2)
        beta = (-c + root) / bma2 if c <= 0 else d2 / (c + root)
        out.update(step=STEP_DL, ca=(1 - beta) * alpha, cg=beta, beta=beta, c=c, bma2=bma2, d2=d2)
    return out


def dogleg_step_model(s, ca, cg, dt=LD):
    """(||h_dl||^2, linearGain = 2 b.h - h^T H h) of h = ca b + cg h_gn with their magnitudes, from the six scalars."""
    bb, bHb, gg, bg, hbg, gHg = (dt(x) for x in s)
    ca, cg = dt(ca), dt(cg)
    dl2 = ca * ca * bb + 2 * ca * cg * bg + cg * cg * gg
    dl2_mag = ca * ca * bb + 2 * abs(ca * cg * bg) + cg * cg * gg
    gain = 2 * (ca * bb + cg * bg) - (ca * ca * bHb + 2 * ca * cg * hbg + cg * cg * gHg)
    gain_mag = 2 * (abs(ca) * bb + abs(cg * bg)) + ca * ca * abs(bHb) + 2 * abs(ca * cg * hbg) + cg * cg * abs(gHg)
    return dl2, dl2_mag, gain, gain_mag
