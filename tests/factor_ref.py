"""The exact block Cholesky, its solves and the selected inversion (direct_kernels.hpp, selinv_kernels.hpp) restated in
numpy on the host plan (Graph.direct_plan / Graph.marginal_plan), vectorised per level.  Two uses:

  * restate(P, vals, b, lam, dt): the whole computation in one number format.  np.longdouble is the reference of the
    pins; float64 walks every list in the kernel's order -- sources, products (seven multiply-subtracts each), the
    backward solve's bord / brow, the selected inversion's za / zt / zl -- and is the noise gauge and what the seeded
    defects (MUTATIONS) are applied to.
  * check(P, vals, b, lam, d): the LOCAL checks of DESIGN.md "How the exact factorisation is tested as an operator".
    Every quantity of a read-out d (Graph.debug_factor, or a restatement) is compared with its long-double value
    computed from d's own inputs to that quantity, bit for bit -- vals, Aperm and the already-final L, Dinv, y, xp, Z --
    against gamma(k) times the same expression in absolute values.  Conditioning never enters, the bound holds for any
    order of summation and any FMA contraction, and a wrong block is named.  A ratio <= 1 passes.

Blocks are [s, r, c]; the plan's numbering throughout (column j of L is block row perm[j] of the system)."""
import numpy as np

import lm_ref as R

LD = np.longdouble
U = R.U
SUB = LD(2) ** -1074  # the smallest subnormal: what a product that underflows may lose (twice the half spacing)

MUTATIONS = ("product_dropped", "last_piece_dropped", "pa_pb_swapped", "lambda_everywhere", "lambda_omitted",
             "second_source_dropped", "dinv_untransposed", "y_without_products", "back_65th_dropped",
             "z_untransposed", "z_9th_dropped", "z0_omitted", "z_mirror_wrong")


def plan_of(G, max_pairs=30_000_000):
    """direct_plan and marginal_plan of a graph as one dict, plus lcol, the products' targets and the backward solve's
    order bord / brow (the selected inversion's diagonal blocks list their column in that order: selinv.cpp)."""
    P = G.direct_plan(max_pairs=max_pairs)
    M = G.marginal_plan(max_pairs=max_pairs)
    for k in ("perm", "colptr", "lrow", "gptr", "lcolp"):
        assert np.array_equal(P[k], M[k]), k
    P.update({k: M[k] for k in ("zptr", "za", "zt", "zl", "nprod")})
    return finish_plan(P)


def finish_plan(P):
    nb, nL = P["nb"], P["nL"]
    cp = P["colptr"]
    P["lcol"] = np.repeat(np.arange(nb, dtype=np.int32), np.diff(cp))
    P["isdiag"] = P["lrow"] == P["lcol"]
    P["np"] = np.diff(P["pairptr"])
    P["nsrc"] = np.diff(P["srcptr"])
    P["pcol"] = P["lcol"][P["pa"]] if P["npairs"] else np.zeros(0, np.int32)
    bord = np.arange(nL, dtype=np.int32)
    for j in range(nb):
        z0 = P["zptr"][cp[j]]
        bord[cp[j] + 1:cp[j + 1]] = P["zl"][z0:z0 + cp[j + 1] - cp[j] - 1]
    P["bord"], P["brow"] = bord, P["lrow"][bord]
    assert all(sorted(bord[cp[j] + 1:cp[j + 1]]) == list(range(cp[j] + 1, cp[j + 1])) for j in range(nb))
    return P


def _ordinals(ptr, sel=None):
    """For r = 0, 1, ...: (the items of `sel` (all) that have an r-th list entry, the entries' positions ptr + r)."""
    sel = np.arange(len(ptr) - 1) if sel is None else np.asarray(sel)
    cnt = ptr[sel + 1] - ptr[sel]
    for r in range(int(cnt.max()) if len(cnt) else 0):
        m = cnt > r
        yield r, np.nonzero(m)[0], ptr[sel[m]] + r


def _chol7(a, dt):
    """k_ldl's 7x7 Cholesky and triangular inverse, batched, operation by operation: (L, Linv, bad pivot anywhere)."""
    a = a.copy()
    n = a.shape[0]
    bad = np.zeros(n, bool)
    big = np.finfo(np.float64).max
    for k in range(7):
        d = a[:, k, k].copy()
        for m in range(k):
            d -= a[:, k, m] * a[:, k, m]
        with np.errstate(invalid="ignore"):
            nok = ~(d > 0) | ~(d < big)
        bad |= nok
        d = np.where(nok, dt(1), d)
        lkk = np.sqrt(d)
        inv = dt(1) / lkk
        a[:, k, k] = lkk
        for rr in range(k + 1, 7):
            v = a[:, rr, k].copy()
            for m in range(k):
                v -= a[:, rr, m] * a[:, k, m]
            a[:, rr, k] = v * inv
    Lf = np.tril(a)
    wi = np.zeros_like(Lf)
    for cc in range(7):
        for rr in range(cc, 7):
            v = np.full(n, 1 if rr == cc else 0, dtype=dt)
            for m in range(cc, rr):
                v -= Lf[:, rr, m] * wi[:, m, cc]
            wi[:, rr, cc] = v / Lf[:, rr, rr]
    return Lf, wi, bad


def _mm_t(acc, A, B, sub=True):
    """acc -+= A B^T entry by entry in the kernel's order: seven multiply-adds."""
    for mm in range(7):
        t = A[:, :, mm, None] * B[:, None, :, mm]
        acc = acc - t if sub else acc + t
    return acc


def restate(P, vals, b, lam, dt=np.float64, selinv=True, mut=None, mut_arg=None):
    """dict(Aperm, bp, L, Dinv, y, xp, x, fail, Z): what Graph.debug_factor returns, in `dt`.  mut: one of MUTATIONS;
    mut_arg: the products (indices into pa) a dropping defect leaves out."""
    nb, nL = P["nb"], P["nL"]
    vals = np.asarray(vals, dtype=dt).reshape(-1, 7, 7)
    b = np.asarray(b, dtype=dt).reshape(nb, 7)
    lam = dt(lam)
    cp, lcol, isd = P["colptr"], P["lcol"], P["isdiag"]
    eye = np.eye(7, dtype=dt)
    drop = set() if mut_arg is None else set(int(k) for k in mut_arg)
    Aperm = np.zeros((nL, 7, 7), dtype=dt)
    for r, it, pos in _ordinals(P["srcptr"]):
        if mut == "second_source_dropped" and r == 1:
            continue
        Aperm[it] = Aperm[it] + vals[P["src"][pos]]
    bp = b[P["perm"]]
    Lb = np.zeros((nL, 7, 7), dtype=dt)
    Dinv = np.zeros((nb, 7, 7), dtype=dt)
    y = np.zeros((nb, 7), dtype=dt)
    fail = False
    for l in range(P["nlevels"]):
        c0, c1 = P["lcolp"][l], P["lcolp"][l + 1]
        S = np.arange(cp[c0], cp[c1])
        raw = Aperm[S].copy()
        dg = isd[S]
        if mut == "lambda_everywhere":
            raw[dg] = raw[dg] + lam
        elif mut != "lambda_omitted":
            raw[dg] = raw[dg] + lam * eye
        tacc = np.zeros((len(S), 7, 7), dtype=dt)
        for r, it, pos in _ordinals(P["pairptr"], S):
            if drop:
                keep = np.array([int(k) not in drop for k in pos])
                it, pos = it[keep], pos[keep]
            A, B = Lb[P["pa"][pos]], Lb[P["pb"][pos]]
            if mut == "pa_pb_swapped":
                A, B = B, A
            raw[it] = _mm_t(raw[it], A, B)
            if mut != "y_without_products":
                tacc[it] = tacc[it] + Lb[P["pa"][pos]] * y[P["pcol"][pos]][:, None, :]
        # diagonal blocks: Cholesky, inverse, y
        cols = np.arange(c0, c1)
        di = np.nonzero(dg)[0]
        Lf, wi, bad = _chol7(raw[di], dt)
        fail = fail or bool(bad.any())
        Lb[cp[cols]] = Lf
        Dinv[cols] = wi
        ts = np.zeros((len(cols), 7), dtype=dt)
        for c in range(7):
            ts = ts + tacc[di][:, :, c]
        yraw = bp[cols] - ts
        yr = np.zeros((len(cols), 7), dtype=dt)
        for c in range(7):
            yr = yr + wi[:, :, c] * yraw[:, c, None]
        y[cols] = yr
        # phase C
        od = np.nonzero(~dg)[0]
        if len(od):
            D = Dinv[lcol[S[od]]]
            if mut == "dinv_untransposed":
                D = D.transpose(0, 2, 1)
            Lb[S[od]] = _mm_t(np.zeros((len(od), 7, 7), dtype=dt), raw[od], D, sub=False)
    out = dict(Aperm=Aperm, bp=bp, L=Lb, Dinv=Dinv, y=y, fail=int(fail))
    # backward solve: levels downwards, a column's blocks in the order bord / brow
    xp = np.zeros((nb, 7), dtype=dt)
    for l in range(P["nlevels"] - 1, -1, -1):
        cols = np.arange(P["lcolp"][l], P["lcolp"][l + 1])
        t = np.zeros((len(cols), 7, 7), dtype=dt)
        ptr = np.concatenate([cp[cols] + 1, [0]])  # (per column: the list starts behind its diagonal block)
        cnt = cp[cols + 1] - cp[cols] - 1
        for r in range(int(cnt.max()) if len(cnt) else 0):
            if mut == "back_65th_dropped" and r == 64:
                continue
            it = np.nonzero(cnt > r)[0]
            pos = ptr[it] + r
            t[it] = t[it] + Lb[P["bord"][pos]] * xp[P["brow"][pos]][:, :, None]
        tr = np.zeros((len(cols), 7), dtype=dt)
        for r in range(7):
            tr = tr + t[:, r, :]
        z = y[cols] - tr
        xr = np.zeros((len(cols), 7), dtype=dt)
        for c in range(7):
            xr = xr + Dinv[cols][:, c, :] * z[:, c, None]
        xp[cols] = xr
    x = np.zeros((nb, 7), dtype=dt)
    x[P["perm"]] = xp
    out.update(xp=xp, x=x)
    if not selinv:
        return out
    Z = np.zeros((nL, 7, 7), dtype=dt)

    def zblocks(S, diag):
        acc = np.zeros((len(S), 7, 7), dtype=dt)
        for r, it, pos in _ordinals(P["zptr"], S):
            if mut == "z_9th_dropped" and r == 8:
                continue
            Zo = Z[P["za"][pos]]
            tr = P["zt"][pos] == 1
            if mut != "z_untransposed":
                Zo = np.where(tr[:, None, None], Zo.transpose(0, 2, 1), Zo)
            acc[it] = _mm_t(acc[it], Zo, Lb[P["zl"][pos]].transpose(0, 2, 1), sub=False)
        D = Dinv[lcol[S]]
        z0 = D.transpose(0, 2, 1) if diag and mut != "z0_omitted" else np.zeros_like(D)
        z = _mm_t(np.zeros_like(acc), z0 - acc, D.transpose(0, 2, 1), sub=False)
        if diag:  # the lower triangle, mirrored
            lo = np.tril(z) if mut != "z_mirror_wrong" else np.triu(z).transpose(0, 2, 1)
            z = lo + np.tril(lo, -1).transpose(0, 2, 1)
        Z[S] = z

    for l in range(P["nlevels"] - 1, -1, -1):
        c0, c1 = P["lcolp"][l], P["lcolp"][l + 1]
        S = np.arange(cp[c0], cp[c1])
        zblocks(S[~isd[S]], False)
        zblocks(S[isd[S]], True)
    out["Z"] = Z
    return out


# ---- the local checks ----
def _ratio(err, tol, what):
    """max err / tol; an entry with a zero bound must be exact, and nothing that is held may be NaN or infinite (a
    NaN in a block makes its own bound NaN: neither comparison below would see it)."""
    assert np.isfinite(err).all() and np.isfinite(tol).all(), \
        f"{what}: non-finite value or bound (first: block {np.argwhere(~(np.isfinite(err) & np.isfinite(tol)))[0]})"
    bad = (tol == 0) & (err != 0)
    assert not bad.any(), f"{what}: an entry with a zero bound is not exact (first: block {np.argwhere(bad)[0]})"
    nz = tol > 0
    return float((err[nz] / tol[nz]).max()) if nz.any() else 0.0


def _worst(err, tol):
    q = np.where(tol > 0, err / np.where(tol > 0, tol, 1), 0).reshape(err.shape[0], -1).max(1)
    return int(np.argmax(q))


def _seg_products(ptr, ia, ib, A, B, n, tb=True):
    """(sum, sum of magnitudes) per item of A[ia[k]] op(B[ib[k]]) over k in ptr[s] .. ptr[s + 1], in long double."""
    out, mag = np.zeros((n, 7, 7), dtype=LD), np.zeros((n, 7, 7), dtype=LD)
    for r, it, pos in _ordinals(ptr):
        a, bb = A[ia[pos]] if ia is not None else A[pos], B[ib[pos]]
        if tb:
            bb = bb.transpose(0, 2, 1)
        out[it] += a @ bb
        mag[it] += np.abs(a) @ np.abs(bb)
    return out, mag


def DT_of(D):
    return D.transpose(0, 2, 1)


def _under(nprod, absD):
    """Underflow allowance of (a sum of nprod products) times D, entry (r, c): every product may lose SUB, the sum's
    loss passes through column c of |D|, and the seven products with D lose SUB each.  Matters only where fill blocks
    have decayed to the subnormal range (a long cycle at lambda = 1e3); bounds of ordinary blocks do not see it."""
    return SUB * (np.asarray(nprod, dtype=LD)[:, None, None] * (np.ones((7, 7), dtype=LD) @ absD) + 7)


def residual_blocks(P, d, lam):
    """(R, mag_raw) of every block of L from the read-out's own operands: Aperm + lambda I - sum L[pa] L[pb]^T."""
    Ld = np.asarray(d["L"], dtype=LD)
    S, M = _seg_products(P["pairptr"], P["pa"], P["pb"], Ld, Ld, P["nL"])
    lamI = np.where(P["isdiag"][:, None, None], LD(lam) * np.eye(7, dtype=LD), LD(0))
    Ap = np.asarray(d["Aperm"], dtype=LD)
    return Ap + lamI - S, np.abs(Ap) + lamI + M


def pivots(Rd, mag, npd):
    """Long-double Cholesky of the diagonal blocks' R with a first-order running error bound of every pivot
    d_k = R_kk - sum_m l_km^2 as float64 arithmetic would leave it: R's entries carry gamma(7 np + 2) mag_raw, every
    inner product of k terms gamma(k + 1) of its magnitude, a square root and a division one rounding each, and the
    errors of the l_km used propagate by the product rule.  Returns (pivots, bounds, bounds doubled for safety) up to
    and including each block's first non-positive pivot; later ones are NaN."""
    n = Rd.shape[0]
    a = Rd.copy()
    e = R.gamma_k(7 * npd + 2)[:, None, None] * mag  # error of the stored entry
    piv, bnd = np.full((n, 7), np.nan, dtype=LD), np.full((n, 7), np.nan, dtype=LD)
    alive = np.ones(n, bool)
    u = LD(U)
    for k in range(7):
        dk = a[:, k, k].copy()
        mg = np.abs(a[:, k, k])
        ek = e[:, k, k].copy()
        for m in range(k):
            dk -= a[:, k, m] ** 2
            mg += a[:, k, m] ** 2
            ek += 2 * np.abs(a[:, k, m]) * e[:, k, m]
        ek += R.gamma_k(k + 1) * mg
        piv[alive, k] = dk[alive]
        bnd[alive, k] = ek[alive]
        with np.errstate(invalid="ignore"):
            alive &= dk > 0
        dk = np.where(alive, dk, 1)
        lkk = np.sqrt(dk)
        elkk = ek / (2 * lkk) + u * lkk
        a[:, k, k] = lkk
        e[:, k, k] = elkk
        for rr in range(k + 1, 7):
            v = a[:, rr, k].copy()
            mv = np.abs(a[:, rr, k])
            ev = e[:, rr, k].copy()
            for m in range(k):
                v -= a[:, rr, m] * a[:, k, m]
                mv += np.abs(a[:, rr, m] * a[:, k, m])
                ev += np.abs(a[:, rr, m]) * e[:, k, m] + np.abs(a[:, k, m]) * e[:, rr, m]
            ev += R.gamma_k(k + 2) * mv
            a[:, rr, k] = v / lkk
            e[:, rr, k] = ev / lkk + np.abs(v / lkk) * (elkk / lkk + u)
    return piv, bnd, 2 * bnd


def fail_expected(P, d, lam):
    """(must fail, must pass, columns whose own pivots fail) from the long-double pivots of every column's R."""
    with np.errstate(all="ignore"):  # (the garbage behind a failed pivot may overflow)
        Rb, mag = residual_blocks(P, d, lam)
        dg = P["colptr"][:-1]
        piv, _, bnd = pivots(Rb[dg], mag[dg], P["np"][dg])
    seen = ~np.isnan(piv)
    with np.errstate(invalid="ignore"):
        neg = seen & ((piv < -bnd) | ((bnd == 0) & (piv <= 0)) | np.isnan(np.where(seen, piv, 0)))
        pos = seen & (piv > bnd)
    nanR = np.isnan(Rb[dg]).any((1, 2))  # (a NaN anywhere fails the comparison d > 0)
    between = seen & ~neg & ~pos
    bad_cols = neg.any(1) | nanR
    return bool(bad_cols.any()), bool((pos | ~seen).all() and not nanR.any()), bad_cols, int(between.sum())


def check(P, vals, b, lam, d, with_solve=True, with_selinv=None, exempt=None):
    """Ratios error / bound of every row of the bound table, {row: (ratio, worst block)}.  exempt: columns (bool, nb)
    left out of the rows L, Dinv and y -- a column whose pivots fail and the ancestors that read its blocks (a failed
    pivot is replaced by 1: what follows is garbage that may leave the range of float64).  Every other column is still
    held, its reference being computed from the read-out's own operands; the backward solve and the selected inversion
    start at the root and are checked only when nothing is exempt."""
    nb, nL = P["nb"], P["nL"]
    cp, lcol, isd = P["colptr"], P["lcol"], P["isdiag"]
    with_selinv = "Z" in d if with_selinv is None else with_selinv
    exempt = np.zeros(nb, bool) if exempt is None else exempt
    out = {}
    g = R.gamma_k
    dev = {k: np.asarray(d[k], dtype=LD) for k in ("Aperm", "bp", "L", "Dinv", "y")}
    # Aperm: the sum of its source blocks, nsrc - 1 additions (the first lands on 0.0)
    v = np.asarray(vals, dtype=LD).reshape(-1, 7, 7)
    ref, mag = np.zeros((nL, 7, 7), dtype=LD), np.zeros((nL, 7, 7), dtype=LD)
    for r, it, pos in _ordinals(P["srcptr"]):
        ref[it] += v[P["src"][pos]]
        mag[it] += np.abs(v[P["src"][pos]])
    err, tol = np.abs(dev["Aperm"] - ref), g(np.maximum(P["nsrc"] - 1, 0))[:, None, None] * mag
    out["Aperm"] = (_ratio(err, tol, "Aperm"), _worst(err, tol))
    assert np.array_equal(np.asarray(d["bp"]), np.asarray(b, dtype=np.float64).reshape(nb, 7)[P["perm"]]), "bp != b[perm]"
    out["bp"] = (0.0, 0)
    with np.errstate(all="ignore"):
        Rb, mraw = residual_blocks(P, d, lam)
    npd = P["np"]
    dg = cp[:-1]
    keep = ~exempt
    Ld, Di = dev["L"][dg], dev["Dinv"]
    low = np.tril(np.ones((7, 7), bool))
    # diagonal L(j,j): L L^T against the lower triangle of R; Higham's Theorem 10.3 (n + 1 = 8) plus the accumulation
    # of R: Aperm + lambda, then 7 np multiply-subtracts -- 7 np + 1 roundings of the first term, one to spare
    assert (np.asarray(d["L"])[dg][:, ~low] == 0).all() and (np.asarray(d["Dinv"])[:, ~low] == 0).all(), \
        "strict upper triangle of L(j,j) / Dinv not exactly zero"
    err = np.abs(Ld @ Ld.transpose(0, 2, 1) - Rb[dg])
    tol = g(8) * (np.abs(Ld) @ np.abs(Ld).transpose(0, 2, 1)) + g(7 * npd[dg] + 2)[:, None, None] * mraw[dg]
    err, tol = np.where(low, err, 0)[keep], np.where(low, tol, 1)[keep]
    out["Ldiag"] = (_ratio(err, tol, "Ldiag"), int(np.nonzero(keep)[0][_worst(err, tol)]) if keep.any() else 0)
    # Dinv: columns by forward substitution, Higham's Theorem 8.5: |L x - e| <= gamma(7) |L| |x|
    err = np.abs(Ld @ Di - np.eye(7, dtype=LD))[keep]
    tol = (g(7) * (np.abs(Ld) @ np.abs(Di)))[keep]
    out["Dinv"] = (_ratio(err, tol, "Dinv"), int(np.nonzero(keep)[0][_worst(err, tol)]) if keep.any() else 0)
    # off-diagonal L(i,j) = raw Dinv^T: the raw block's first term sees 7 np roundings, a product's 7 np + 1, the
    # seven multiply-adds of the triangular product 7 more: 7 np + 8
    od = np.nonzero(~isd)[0]
    od = od[keep[lcol[od]]]
    if len(od):
        DT = Di[lcol[od]].transpose(0, 2, 1)
        err = np.abs(dev["L"][od] - Rb[od] @ DT)
        tol = g(7 * npd[od] + 8)[:, None, None] * (mraw[od] @ np.abs(DT)) + _under(7 * npd[od], np.abs(DT))
        out["Loff"] = (_ratio(err, tol, "Loff"), int(od[_worst(err, tol)]))
    # y_j = Dinv (bp_j - sum L(j,k) y_k): np chained products (np roundings of the first), 6 + 1 + 7 for the sum over
    # c, the subtraction and the product with Dinv: np + 14; a leaf column has no products, the chain and the sums are
    # exact zeros: 8, the bare triangular product's
    yd = dev["y"]
    s, m = np.zeros((nb, 7), dtype=LD), np.zeros((nb, 7), dtype=LD)
    for r, it, pos in _ordinals(P["pairptr"], dg):
        Lk, yk = dev["L"][P["pa"][pos]], yd[P["pcol"][pos]]
        s[it] += (Lk @ yk[:, :, None])[:, :, 0]
        m[it] += (np.abs(Lk) @ np.abs(yk)[:, :, None])[:, :, 0]
    ref = (Di @ (dev["bp"] - s)[:, :, None])[:, :, 0]
    mag = (np.abs(Di) @ (np.abs(dev["bp"]) + m)[:, :, None])[:, :, 0]
    err, tol = np.abs(yd - ref), g(np.where(npd[dg] > 0, npd[dg] + 14, 8))[:, None] * mag + _under(7 * npd[dg], np.abs(DT_of(Di)))[:, 0, :]
    err, tol = err[keep], tol[keep]
    out["y"] = (_ratio(err, tol, "y"), int(np.nonzero(keep)[0][_worst(err, tol)]) if keep.any() else 0)
    assert not (exempt.any() and (with_solve or with_selinv)), "the solve and the inverse start at the root"
    if with_solve:
        # xp_j = Dinv^T (y_j - sum L(i,j)^T xp_i): noff chained products, 6 + 1 + 1 + 6: noff + 14; a root has no
        # products, the chain and the sums are exact zeros: the 8 of a bare triangular product
        xd = np.asarray(d["xp"], dtype=LD)
        noff = np.diff(cp) - 1
        s, m = np.zeros((nb, 7), dtype=LD), np.zeros((nb, 7), dtype=LD)
        optr = np.stack([cp[:-1] + 1, cp[1:]], 1)
        for r in range(int(noff.max()) if nb else 0):
            it = np.nonzero(noff > r)[0]
            pos = optr[it, 0] + r
            LT, xi = dev["L"][pos].transpose(0, 2, 1), xd[P["lrow"][pos]]
            s[it] += (LT @ xi[:, :, None])[:, :, 0]
            m[it] += (np.abs(LT) @ np.abs(xi)[:, :, None])[:, :, 0]
        DT = Di.transpose(0, 2, 1)
        ref = (DT @ (yd - s)[:, :, None])[:, :, 0]
        mag = (np.abs(DT) @ (np.abs(yd) + m)[:, :, None])[:, :, 0]
        err, tol = np.abs(xd - ref), g(np.where(noff > 0, noff + 14, 8))[:, None] * mag + _under(7 * noff, np.abs(Di))[:, 0, :]
        out["xp"] = (_ratio(err, tol, "xp"), _worst(err, tol))
        assert np.array_equal(np.asarray(d["x"]).reshape(nb, 7)[P["perm"]], np.asarray(d["xp"]), equal_nan=True), \
            "x[perm[j]] != xp[j]"
    if with_selinv:
        # Z[s] = (Z0 - sum op(Z[za]) L[zl]) Dinv: 7 np multiply-adds (7 np roundings of the first term), the
        # subtraction, seven more: 7 np + 8
        Zd = np.asarray(d["Z"], dtype=LD)
        nz = np.diff(P["zptr"])
        opZ = np.where((P["zt"] == 1)[:, None, None], Zd[P["za"]].transpose(0, 2, 1), Zd[P["za"]])
        s, m = _seg_products(P["zptr"], None, P["zl"], opZ, dev["L"], nL, tb=False)
        D = Di[lcol]
        z0 = np.where(isd[:, None, None], D.transpose(0, 2, 1), LD(0))
        ref = (z0 - s) @ D
        mag = (np.abs(z0) + m) @ np.abs(D)
        err, tol = np.abs(Zd - ref), g(7 * nz + 8)[:, None, None] * mag + _under(7 * nz, np.abs(D))
        # (a diagonal block stores its lower triangle twice: the upper one is held by the symmetry below)
        up = isd[:, None, None] & ~low[None]
        err, tol = np.where(up, 0, err), np.where(up, 1, tol)
        out["Z"] = (_ratio(err, tol, "Z"), _worst(err, tol))
        Zdg = np.asarray(d["Z"])[dg]
        assert np.array_equal(Zdg, Zdg.transpose(0, 2, 1)), "a diagonal block of Z is not exactly symmetric"
    return out


def singular_expected(P, vals, rowptr, d):
    """k_selinv_pivots, exactly: some L(j,j)(r,r)^2 is not above 1e-13 max |H_dd| -- two float64 products and a
    comparison, nothing a compiler may contract -- with max |H_dd| over the scalar diagonal of the diagonal blocks."""
    v = np.asarray(vals, dtype=np.float64).reshape(-1, 7, 7)
    maxdiag = np.abs(np.diagonal(v[rowptr[:-1]], axis1=1, axis2=2)).max()
    l = np.diagonal(np.asarray(d["L"])[P["colptr"][:-1]], axis1=1, axis2=2)
    return int((~(l * l > 1e-13 * maxdiag)).any())


# ---- blocks of the inverse outside the pattern (cov_kernels.hpp) ----
def root_paths(T, Lb, Dinv, cols, dt):
    """{j: (path, W(., j) on it)} by k_cov_paths' recursion in `dt` (cov_ref.replay_paths, any number format): the
    operands are the read-out's L and Dinv, so float64 is the noise gauge and long double the reference."""
    Lb, Dinv = np.asarray(Lb, dtype=dt), np.asarray(Dinv, dtype=dt)
    out = {}
    for j in cols:
        path = T.path(j)
        at = {k: t for t, k in enumerate(path)}
        acc = np.zeros((len(path), 7, 7), dtype=dt)
        acc[0] = np.eye(7, dtype=dt)
        for t, m in enumerate(path):
            acc[t] = Dinv[m] @ acc[t]
            for s in range(T.colptr[m] + 1, T.colptr[m + 1]):
                acc[at[int(T.lrow[s])]] -= Lb[s] @ acc[t]
        out[j] = (path, acc)
    return out


def pair_block(T, W, a, b, dt):
    """Z(a, b) = sum over the common suffix of the two root paths of W(k, a)^T W(k, b); no common ancestor: zero."""
    k = T.lca(a, b)
    Z = np.zeros((7, 7), dtype=dt)
    if k < 0:
        return Z, 0
    n = int(T.depth[k]) + 1
    (pa, wa), (pb, wb) = W[a], W[b]
    for t in range(n):
        Z += wa[len(pa) - n + t].T @ wb[len(pb) - n + t]
    return Z, n


# ---- dense pins (tests/test_factor_ref.py) ----
def dense_of(rowptr, colidx, vals, lam):
    nb = len(rowptr) - 1
    rows = np.repeat(np.arange(nb), np.diff(rowptr))
    M = np.zeros((nb, 7, nb, 7))
    for k in range(len(colidx)):
        M[rows[k], :, colidx[k], :] += vals[k]
    return M.reshape(7 * nb, 7 * nb) + lam * np.eye(7 * nb)
