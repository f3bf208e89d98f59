"""Independent numpy restatement of the batched homography stage (sim3opt_homography_batch, include/sim3opt.h;
HomographyInit::Compute of the reference): hypotheses from the SVD null space of the 8 x 9 system, as the reference
takes them; the refinement's normal equations summed and solved in long double; the decomposition from
numpy.linalg.svd; the median from a sort; the sampler the stated one.  It shares no linear algebra with
sim3opt_amd/csrc/homography_math.hpp (closed form, Cholesky, Jacobi).  The error of a correspondence is written in the
order of operations the header states, so that a point's side of a threshold is the same question for both.

`defect` seeds one-line defects (tests/test_homography_ref.py shows that each is noticed)."""
import numpy as np

MASK64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
DEFAULTS = dict(max_pixel_error=5.0, seed=0, iterations=300, refine_rounds=5, min_points=10)
OK, FEW_POINTS, NO_HYPOTHESIS, NO_INLIERS, DEGENERATE = 0, 1, 2, 3, 4
COLLINEAR_MIN = 1e-9
LD = np.longdouble


def splitmix64(x):
    z = (x + GOLDEN) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def sample(seed, h, n):
    """four distinct indices below n: draw j picks among the n - j not yet taken"""
    out = []
    for j in range(4):
        i = splitmix64((seed + (4 * h + j + 1) * GOLDEN) & MASK64) % (n - j)
        for s in sorted(out):
            if s <= i:
                i += 1
        out.append(i)
    return out


def normalise(uv, f, cx, cy):
    return np.stack([(uv[:, 0] - cx) / f, (uv[:, 1] - cy) / f], axis=1)


def sq_error(H, x0, x1, f):
    """e2 [px^2] of correspondences x0, x1 (n, 2) under H (..., 3, 3) -> (..., n), and the projective depth"""
    H = np.asarray(H, dtype=float)
    h = lambda i, j: H[..., i, j][..., None]
    with np.errstate(all="ignore"):
        p0 = (h(0, 0) * x0[:, 0] + h(0, 1) * x0[:, 1]) + h(0, 2)
        p1 = (h(1, 0) * x0[:, 0] + h(1, 1) * x0[:, 1]) + h(1, 2)
        p2 = (h(2, 0) * x0[:, 0] + h(2, 1) * x0[:, 1]) + h(2, 2)
        ex = f * (x1[:, 0] - p0 / p2)
        ey = f * (x1[:, 1] - p1 / p2)
        return ex * ex + ey * ey, p2


def mlesac_cost(e2, max2):
    """(the sum in long double, the capped terms)"""
    with np.errstate(invalid="ignore"):
        capped = np.where(e2 < max2, e2, max2)
    return capped.astype(LD).sum(axis=-1).astype(float), capped


def inliers_of(e2, max2, defect=None):
    with np.errstate(invalid="ignore"):
        return e2 <= max2 if defect == "inlier_le" else e2 < max2


def sample_valid(q0, q1):
    """no triangle of three of the four points with twice its area at most COLLINEAR_MIN, in either view"""
    for q in (q0, q1):
        for tri in ((0, 1, 2), (3, 1, 2), (0, 3, 2), (0, 1, 3)):
            a, b, c = q[list(tri)]
            if not abs((b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])) > COLLINEAR_MIN:
                return False
    return True


def four_point(q0, q1):
    """HomographyFromMatches of four correspondences: the right null vector of the 8 x 9 system, Frobenius norm 1"""
    M = np.zeros((9, 9))
    for k in range(4):
        x, y = q0[k]
        u, v = q1[k]
        M[2 * k] = [x, y, 1, 0, 0, 0, -x * u, -y * u, -u]
        M[2 * k + 1] = [0, 0, 0, x, y, 1, -x * v, -y * v, -v]
    H = np.linalg.svd(M)[2][8].reshape(3, 3)
    return H / np.linalg.norm(H)


def hypotheses(uv0, uv1, f, cx, cy, opts):
    """dict of sample (H, 4), valid (H,), H (H, 3, 3; the identity where not valid), cost (H,; 0 where not valid),
    e2 (H, n)"""
    x0, x1 = normalise(uv0, f, cx, cy), normalise(uv1, f, cx, cy)
    n, nh = len(x0), opts["iterations"]
    smp = np.array([sample(opts["seed"], h, n) for h in range(nh)])
    valid, Hs = np.zeros(nh, dtype=bool), np.tile(np.eye(3), (nh, 1, 1))
    for h in range(nh):
        q0, q1 = x0[smp[h]], x1[smp[h]]
        if sample_valid(q0, q1):
            Hh = four_point(q0, q1)
            if np.isfinite(Hh).all():
                valid[h], Hs[h] = True, Hh
    e2, _ = sq_error(Hs, x0, x1, f)
    cost, _ = mlesac_cost(e2, opts["max_pixel_error"] ** 2)
    return dict(sample=smp, valid=valid, H=Hs, cost=np.where(valid, cost, 0.0), e2=e2)


def best_hypothesis(hyp):
    """smallest cost, then smallest index, among the valid; -1 if none"""
    idx = np.where(hyp["valid"])[0]
    return int(idx[np.argmin(hyp["cost"][idx])]) if len(idx) else -1  # (argmin: the first of equals)


def sigma_squared(e2, defect=None):
    """Tukey::FindSigmaSquared"""
    m = len(e2)
    srt = np.sort(e2)
    rank = (m + 1) // 2 - 1 if defect == "median_rank" else m // 2
    sigma = 4.6851 * (1.4826 * (1 + 5.0 / (m * 2 - 6)) * np.sqrt(srt[rank]))
    return float(sigma * sigma)


def solve_ld(M, b):
    """Gaussian elimination with partial pivoting in long double"""
    M, b = M.astype(LD).copy(), b.astype(LD).copy()
    n = len(b)
    with np.errstate(all="ignore"):
        for c in range(n):
            p = c + int(np.argmax(np.abs(M[c:, c])))
            M[[c, p]], b[[c, p]] = M[[p, c]], b[[p, c]]
            for r in range(c + 1, n):
                k = M[r, c] / M[c, c]
                M[r] -= k * M[c]
                b[r] -= k * b[c]
        x = np.zeros(n, dtype=LD)
        for r in range(n - 1, -1, -1):
            x[r] = (b[r] - M[r, r + 1:] @ x[r + 1:]) / M[r, r]
    return x.astype(float)


def refine_round(H, x0, x1, f, inl, defect=None):
    """RefineHomographyWithInliers once: (sigma^2, the new H)"""
    a, b = x0[inl], x1[inl]
    e2, _ = sq_error(H, a, b, f)
    s2 = sigma_squared(e2, defect)
    with np.errstate(all="ignore"):
        w = np.where(e2 > s2, 0.0, (1.0 - e2 / s2) ** 2)
    u = np.concatenate([a, np.ones((len(a), 1))], axis=1).astype(LD)
    Hl = H.astype(LD)
    p = u @ Hl.T
    den = p[:, 2]
    err = LD(f) * (b.astype(LD) - p[:, :2] / den[:, None])
    J = np.zeros((len(a), 2, 9), dtype=LD)
    J[:, 0, 0:3] = u / den[:, None]
    J[:, 1, 3:6] = u / den[:, None]
    J[:, 0, 6:9] = -u * (p[:, 0] / (den * den))[:, None]
    J[:, 1, 6:9] = -u * (p[:, 1] / (den * den))[:, None]
    J *= LD(f)
    wl = w.astype(LD)
    M = np.einsum("n,nri,nrj->ij", wl, J, J)
    if defect != "no_prior":
        M = M + np.eye(9, dtype=LD)
    g = np.einsum("n,nri,nr->i", wl, J, err)
    return s2, H + solve_ld(M, g).reshape(3, 3)


def refine(H, x0, x1, f, inl, rounds, max2, defect=None):
    """dict of sigma2 (rounds,), H (rounds, 3, 3) after every round"""
    s2s, Hs = [], []
    for _ in range(rounds):
        if defect == "inliers_recomputed":
            inl = inliers_of(sq_error(H, x0, x1, f)[0], max2)
        s2, H = refine_round(H, x0, x1, f, inl, defect)
        s2s.append(s2)
        Hs.append(H)
    return dict(sigma2=np.array(s2s), H=np.array(Hs).reshape(-1, 3, 3))


def signed_svd(H):
    """numpy's SVD with every column of V signed so that its component of largest magnitude (the first such) is
    positive, the columns of U following"""
    U, d, Vt = np.linalg.svd(H)
    V = Vt.T.copy()
    U = U.copy()
    for j in range(3):
        if V[int(np.argmax(np.abs(V[:, j]))), j] < 0:
            V[:, j], U[:, j] = -V[:, j], -U[:, j]
    return U, np.abs(d), V


def decompose(H, defect=None):
    """DecomposeHomography: a list of eight dict(R, t, n, d), or None (not case 1, or non-finite)"""
    if not np.isfinite(H).all():
        return None
    U, d, V = signed_svd(H)
    d1, d2, d3 = (d * d if defect == "d_squared" else d)
    if not (d1 != d2 and d2 != d3):
        return None
    s = np.linalg.det(U) * np.linalg.det(V)
    x1 = np.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3))
    x3 = np.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
    e1, e3 = [1.0, -1.0, 1.0, -1.0], [1.0, 1.0, -1.0, -1.0]
    out = []
    for k in range(8):
        a, c = e1[k % 4], e3[k % 4]
        Rp = np.eye(3)
        if k < 4:
            sn = (d1 - d3) * x1 * x3 * a * c / d2
            cs = (d1 * x3 * x3 + d3 * x1 * x1) / d2
            Rp[0, 0], Rp[0, 2], Rp[2, 0], Rp[2, 2] = cs, -sn, sn, cs
            tp = np.array([(d1 - d3) * x1 * a, 0.0, (d1 - d3) * (x3 if defect == "eq14_sign" else -x3) * c])
            dd = s * d2
        else:
            Rp = -Rp
            sn = (d1 + d3) * x1 * x3 * a * c / d2
            cs = (d3 * x1 * x1 - d1 * x3 * x3) / d2
            Rp[0, 0], Rp[0, 2], Rp[2, 0], Rp[2, 2] = cs, sn, sn, -cs
            tp = np.array([(d1 + d3) * x1 * a, 0.0, (d1 + d3) * x3 * c])
            dd = -s * d2
        out.append(dict(R=s * U @ Rp @ V.T, t=U @ tp, n=V @ np.array([x1 * a, 0.0, x3 * c]), d=dd))
    return out if all(np.isfinite(np.concatenate([o["R"].ravel(), o["t"], o["n"], [o["d"]]])).all() for o in out) else None


def keep(ids, counts, k, defect=None):
    """the first k of ids by larger count, then by smaller id"""
    tie = (lambda i: -ids[i]) if defect == "tie_rule" else (lambda i: ids[i])
    order = sorted(range(len(ids)), key=lambda i: (-counts[i], tie(i)))[:k]
    return [ids[i] for i in order], [counts[i] for i in order]


def sampson_sum(R, t, x0, x1, limit, defect=None):
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    E = tx @ R
    u0 = np.concatenate([x0, np.ones((len(x0), 1))], axis=1)
    u1 = np.concatenate([x1, np.ones((len(x1), 1))], axis=1)
    a, b = u0 @ E.T, u1 @ E
    with np.errstate(all="ignore"):
        d = (u1 * a).sum(1) ** 2 / (a[:, 0] ** 2 + a[:, 1] ** 2 + b[:, 0] ** 2 + b[:, 1] ** 2)
        if defect != "sampson_cap":
            d = np.where(d > limit, limit, d)
    return float(d.astype(LD).sum())


def choose(H, x0, x1, inl, max2, defect=None):
    """DecomposeHomography + ChooseBestDecomposition: dict of status and, with status OK, decompositions, counts_first
    (8), kept (4), counts_second (4), choice, ambiguous, sampson (2), R, t, and the margins vis_first, vis_second (the
    tested quantities over the inliers)"""
    dec = decompose(H, defect)
    if dec is None:
        return dict(status=DEGENERATE)
    a = x0[inl]
    num = (H[2, 0] * a[:, 0] + H[2, 1] * a[:, 1]) + H[2, 2]
    v1 = np.array([num / o["d"] for o in dec])
    c1 = [int((v > 0).sum()) for v in v1]
    kept, _ = keep(list(range(8)), c1, 4, defect)
    v2 = np.array([((a[:, 0] * dec[k]["n"][0] + a[:, 1] * dec[k]["n"][1]) + dec[k]["n"][2]) / dec[k]["d"] for k in kept])
    c2 = [int((v > 0).sum()) for v in v2]
    two, s2 = keep(kept, c2, 2, defect)
    with np.errstate(all="ignore"):
        ratio = np.float64(-s2[1]) / np.float64(-s2[0])
    ambiguous = not ratio < 0.9
    sums, choice = [0.0, 0.0], two[0]
    if ambiguous:
        sums = [sampson_sum(dec[k]["R"], dec[k]["t"], x0, x1, 4 * max2, defect) for k in two]
        choice = two[0] if sums[0] <= sums[1] else two[1]
    return dict(status=OK, decompositions=dec, counts_first=np.array(c1), kept=np.array(kept), counts_second=np.array(c2),
                two=two, ratio=float(ratio), choice=choice, ambiguous=ambiguous, sampson=np.array(sums),
                R=dec[choice]["R"], t=dec[choice]["t"], n=dec[choice]["n"], d=dec[choice]["d"], vis_first=v1,
                vis_second=v2)


def solve(uv0, uv1, f, cx, cy, opts, defect=None):
    """HomographyInit::Compute of one problem: dict of status and what the stages left"""
    n = len(uv0)
    if n < opts["min_points"]:
        return dict(status=FEW_POINTS)
    hyp = hypotheses(uv0, uv1, f, cx, cy, opts)
    best = best_hypothesis(hyp)
    if best < 0:
        return dict(status=NO_HYPOTHESIS, hyp=hyp, best=-1)
    x0, x1 = normalise(uv0, f, cx, cy), normalise(uv1, f, cx, cy)
    max2 = opts["max_pixel_error"] ** 2
    Hm = hyp["H"][best]
    inl = inliers_of(hyp["e2"][best], max2, defect)
    out = dict(hyp=hyp, best=best, H_mlesac=Hm, mask=inl, n_inliers=int(inl.sum()), cost=float(hyp["cost"][best]))
    if inl.sum() < 4:
        return dict(out, status=NO_INLIERS)
    ref = refine(Hm, x0, x1, f, inl, opts["refine_rounds"], max2, defect)
    Hr = ref["H"][-1] if opts["refine_rounds"] else Hm
    ch = choose(Hr, x0, x1, inl, max2, defect)
    return dict(out, refine=ref, H_refined=Hr, **ch)


def quat_to_R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
