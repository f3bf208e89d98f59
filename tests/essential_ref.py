"""Independent numpy restatement of the batched essential-matrix RANSAC (sim3opt_essential_batch, include/sim3opt.h)
with a different solver: the null space by SVD, the ten cubics expanded as polynomials, and the solutions as
eigenvectors of the 10 x 10 action matrix (Stewenius' formulation of the five-point problem), so that it shares no
polynomial root finder with sim3opt_amd/csrc/essential_math.hpp.  Pose recovery is numpy.linalg.svd; the depths are the
linear least-squares triangulation of the definition, through a pseudo-inverse.  Sampler, Sampson error and the best
rule are restated from the definitions in the header, not from the .hpp.

`defect` seeds one-line defects (tests/test_essential_ref.py shows that each is noticed)."""
import numpy as np

MASK64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
DEFAULTS = dict(threshold=1.0, distance_threshold=50.0, seed=0, iterations=1000, min_points=9)
OK, FEW_POINTS, NO_HYPOTHESIS, NO_POSE = 0, 1, 2, 3


def splitmix64(x):
    z = (x + GOLDEN) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def sample(seed, h, n, defect=None):
    """six distinct indices below n: draw j picks among the n - j not yet taken"""
    out, taken = [], []
    for j in range(6):
        i = splitmix64((seed + (6 * h + j + 1) * GOLDEN) & MASK64) % (n - j)
        if defect != "sampler_skip":
            for s in sorted(taken):
                if s <= i:
                    i += 1
        out.append(i)
        taken.append(i)
    return out


def normalise(uv, f, cx, cy):
    return np.stack([(uv[:, 0] - cx) / f, (uv[:, 1] - cy) / f], axis=1)


def sampson(E, x0, x1, defect=None):
    """e2 of correspondences x0, x1 (n, 2) under E (..., 3, 3), in the order of operations the header states -> (..., n)"""
    E = np.asarray(E)
    if defect == "E_transposed":
        E = np.swapaxes(E, -1, -2)
    e = lambda i, j: E[..., i, j][..., None]
    u0, v0, u1, v1 = x0[:, 0], x0[:, 1], x1[:, 0], x1[:, 1]
    with np.errstate(all="ignore"):
        a0 = (e(0, 0) * u0 + e(0, 1) * v0) + e(0, 2)
        a1 = (e(1, 0) * u0 + e(1, 1) * v0) + e(1, 2)
        a2 = (e(2, 0) * u0 + e(2, 1) * v0) + e(2, 2)
        b0 = (e(0, 0) * u1 + e(1, 0) * v1) + e(2, 0)
        b1 = (e(0, 1) * u1 + e(1, 1) * v1) + e(2, 1)
        d = (u1 * a0 + v1 * a1) + a2
        den = a0 * a0 + a1 * a1
        if defect != "sampson_half_denominator":
            den = (den + b0 * b0) + b1 * b1
        return (d * d) / den


# ---- polynomials in x, y, z of degree <= 1, 2, 3 by monomial tables (variable 3 is the constant 1) ----
MONO3 = [(0, 0, 0), (0, 0, 1), (0, 0, 2), (0, 1, 1), (0, 1, 2), (0, 2, 2), (1, 1, 1), (1, 1, 2), (1, 2, 2), (2, 2, 2),
         (0, 0, 3), (0, 1, 3), (0, 2, 3), (1, 1, 3), (1, 2, 3), (2, 2, 3), (0, 3, 3), (1, 3, 3), (2, 3, 3), (3, 3, 3)]
# x^3 x^2y x^2z xy^2 xyz xz^2 y^3 y^2z yz^2 z^3 | x^2 xy xz y^2 yz z^2 x y z 1
MONO2 = [(a, b) for a in range(4) for b in range(a, 4)]
T2 = np.array([[MONO2.index(tuple(sorted((a, b)))) for b in range(4)] for a in range(4)])
T3 = np.array([[MONO3.index(tuple(sorted(MONO2[m] + (c,)))) for c in range(4)] for m in range(10)])


def mul11(p, q):
    out = np.zeros(np.broadcast(p[..., 0], q[..., 0]).shape + (10,))
    for a in range(4):
        for b in range(4):
            out[..., T2[a, b]] += p[..., a] * q[..., b]
    return out


def mul21(p, q):
    out = np.zeros(np.broadcast(p[..., 0], q[..., 0]).shape + (20,))
    for m in range(10):
        for c in range(4):
            out[..., T3[m, c]] += p[..., m] * q[..., c]
    return out


def constraint_matrix(N, defect=None):
    """N (H, 4, 3, 3): the basis.  -> (H, 10, 20) in MONO3's column order: det E, then 2 E E^T E - tr(E E^T) E"""
    Ep = np.moveaxis(N, 1, -1)  # (H, 3, 3, 4): entry (i, j) as a polynomial
    e = lambda i, j: Ep[:, i, j]
    det = mul21(mul11(e(1, 1), e(2, 2)) - mul11(e(1, 2), e(2, 1)), e(0, 0)) \
        - mul21(mul11(e(1, 0), e(2, 2)) - mul11(e(1, 2), e(2, 0)), e(0, 1)) \
        + mul21(mul11(e(1, 0), e(2, 1)) - mul11(e(1, 1), e(2, 0)), e(0, 2))
    EEt = sum(mul11(Ep[:, :, None, k], Ep[:, None, :, k]) for k in range(3))  # (H, 3, 3, 10)
    tr = EEt[:, 0, 0] + EEt[:, 1, 1] + EEt[:, 2, 2]
    EEtE = sum(mul21(EEt[:, :, k, None, :], Ep[:, None, k, :, :]) for k in range(3))  # (H, 3, 3, 20)
    factor = 1.0 if defect == "trace_factor_1" else 2.0
    rows = factor * EEtE - mul21(tr[:, None, None, :], Ep)
    return np.concatenate([det[:, None, :], rows.reshape(-1, 9, 20)], axis=1)


ACTION = {  # variable -> (rows of -C for the six quadratic basis monomials, then the basis index of v * (x, y, z, 1))
    "x": ([0, 1, 2, 3, 4, 5], [0, 1, 2, 6]),
    "y": ([1, 3, 4, 6, 7, 8], [1, 3, 4, 7]),
}


def solutions(N, variable="x", defect=None):
    """Per hypothesis the real solutions (x, y, z) of the ten cubics: list of (k, 3) arrays, and whether the reduction
    was possible."""
    M = constraint_matrix(N, defect)
    H = M.shape[0]
    out, ok = [], np.ones(H, dtype=bool)
    rows, units = ACTION[variable]
    for h in range(H):
        try:
            with np.errstate(all="ignore"):
                C = np.linalg.solve(M[h, :, :10], M[h, :, 10:])
            if not np.isfinite(C).all():
                raise np.linalg.LinAlgError
        except np.linalg.LinAlgError:
            ok[h] = False
            out.append(np.zeros((0, 3)))
            continue
        At = np.zeros((10, 10))
        At[:6] = -C[rows]
        for r, u in zip(range(6, 10), units):
            At[r, u] = 1.0
        w, v = np.linalg.eig(At)
        real = w.imag == 0
        with np.errstate(all="ignore"):
            s = (v[6:9, real] / v[9, real]).real.T
        out.append(s[np.isfinite(s).all(axis=1)])
    return out, ok


def null_basis(x0, x1):
    """x0, x1 (H, 5, 2) -> (H, 4, 3, 3), or None rows flagged False where the system has no four-dimensional null space"""
    one = np.ones(x0.shape[:2])
    A = np.stack([x1[..., 0] * x0[..., 0], x1[..., 0] * x0[..., 1], x1[..., 0], x1[..., 1] * x0[..., 0],
                  x1[..., 1] * x0[..., 1], x1[..., 1], x0[..., 0], x0[..., 1], one], axis=-1)
    _, s, vt = np.linalg.svd(A)
    return vt[:, 5:].reshape(-1, 4, 3, 3), s[:, 4] > 1e-12 * s[:, 0]


def hypotheses(uv0, uv1, f, cx, cy, opts, defect=None, variable="x"):
    """Every hypothesis of one problem: dict of sample (H, 6), valid, n_solutions, E (H, 3, 3; zero where not valid),
    e2 (H, n), count, cost."""
    x0, x1 = normalise(uv0, f, cx, cy), normalise(uv1, f, cx, cy)
    n, H = x0.shape[0], opts["iterations"]
    smp = np.array([sample(opts["seed"], h, n, defect) for h in range(H)])
    N, full = null_basis(x0[smp[:, :5]], x1[smp[:, :5]])
    sols, ok = solutions(N, variable, defect)
    E = np.zeros((H, 3, 3))
    valid, nsol = np.zeros(H, dtype=bool), np.zeros(H, dtype=np.int32)
    for h in range(H):
        pts = np.concatenate([x0[smp[h]], x1[smp[h]]], axis=1)
        if not (full[h] and ok[h]) or len(np.unique(pts, axis=0)) < 6 or len(sols[h]) == 0:  # (a repeated point)
            continue
        s = sols[h]
        Es = s[:, 0, None, None] * N[h, 0] + s[:, 1, None, None] * N[h, 1] + s[:, 2, None, None] * N[h, 2] + N[h, 3]
        Es = Es / np.sqrt((Es ** 2).sum(axis=(1, 2)))[:, None, None]
        Es = Es[np.isfinite(Es).all(axis=(1, 2))]
        nsol[h] = len(Es)
        if len(Es) == 0:
            continue
        p = smp[h, 5]
        e6 = sampson(Es, x0[p:p + 1], x1[p:p + 1])[:, 0]
        if defect == "ignore_sixth":
            e6 = np.arange(len(Es), dtype=float)
        if not np.isfinite(e6).any():
            continue
        E[h] = Es[np.nanargmin(np.where(np.isfinite(e6), e6, np.inf))]
        valid[h] = True
    thr = opts["threshold"] if defect == "threshold_not_normalised" else opts["threshold"] / f
    e2 = sampson(E, x0, x1, defect)
    with np.errstate(invalid="ignore"):
        inl = (e2 <= thr * thr) & valid[:, None]
    return dict(sample=smp, valid=valid, n_solutions=nsol, E=E, e2=e2, count=inl.sum(1).astype(np.int32),
                cost=np.where(inl, e2, 0.0).sum(1))


def best_hypothesis(hyp, defect=None):
    """largest count, then smallest cost, then smallest index; -1 without a valid one"""
    best = -1
    for h in np.where(hyp["valid"])[0]:
        if best < 0 or hyp["count"][h] > hyp["count"][best] or \
                (hyp["count"][h] == hyp["count"][best] and defect != "tie_ignores_cost" and hyp["cost"][h] < hyp["cost"][best]):
            best = int(h)
    return best


def skew(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


def candidates(E, defect=None):
    """The four (R, t) of E in the header's order, by SVD: t spans the left null space, its largest component (the
    first such) positive; Ra has E = +s [t]x Ra, Rb has E = -s [t]x Rb.  None when E has no such direction."""
    if not np.isfinite(E).all() or not np.abs(E).max() > 0:
        return None
    U, _, Vt = np.linalg.svd(E)
    t = U[:, 2].copy()
    if t[np.argmax(np.abs(t))] < 0:
        t = -t
    W = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    Rs = [U @ W @ Vt, U @ W.T @ Vt]
    Rs = [R if np.linalg.det(R) > 0 else -R for R in Rs]
    Ra, Rb = Rs if (E * (skew(t) @ Rs[0])).sum() > 0 else Rs[::-1]
    if defect == "t_sign_23":
        return [(Ra, t), (Rb, t), (Ra, t), (Rb, t)]
    return [(Ra, t), (Rb, t), (Ra, -t), (Rb, -t)]


def depths(R, t, x0, x1):
    """(z0, z1) (n,) each: the least-squares solution of z0 R x0 - z1 x1 = -t per correspondence"""
    h0 = np.concatenate([x0, np.ones((len(x0), 1))], axis=1)
    h1 = np.concatenate([x1, np.ones((len(x1), 1))], axis=1)
    A = np.stack([h0 @ R.T, -h1], axis=2)  # (n, 3, 2)
    with np.errstate(all="ignore"):
        try:
            z = np.linalg.pinv(A, rcond=1e-15) @ (-t)
        except np.linalg.LinAlgError:
            z = np.full((len(x0), 2), np.nan)
    return z[:, 0], z[:, 1]


def recover_pose(E, x0, x1, inl, dist, defect=None):
    """dict of candidates (list of (R, t) or None), z (4, n, 2), voted (4, n) bool, votes (4,), winner, mask (n,)"""
    cand = candidates(E, defect)
    n = len(x0)
    z, voted = np.full((4, n, 2), np.nan), np.zeros((4, n), dtype=bool)
    if cand is not None:
        for c, (R, t) in enumerate(cand):
            z0, z1 = depths(R, t, x0, x1)
            z[c, :, 0], z[c, :, 1] = z0, z1
            with np.errstate(invalid="ignore"):
                v = (z0 > 0) & (z1 > 0)
                if defect != "no_distance_threshold":
                    v &= (z0 < dist) & (z1 < dist)
            voted[c] = v & inl
    votes = voted.sum(1).astype(np.int32)
    winner = int(np.argmax(votes))  # (the first of equals)
    return dict(candidates=cand, z=z, voted=voted, votes=votes, winner=winner, mask=voted[winner])


def R_to_quat(R):
    """unit quaternion x y z w with w >= 0"""
    K = np.array([[R[0, 0] - R[1, 1] - R[2, 2], R[1, 0] + R[0, 1], R[2, 0] + R[0, 2], R[2, 1] - R[1, 2]],
                  [R[1, 0] + R[0, 1], R[1, 1] - R[0, 0] - R[2, 2], R[2, 1] + R[1, 2], R[0, 2] - R[2, 0]],
                  [R[2, 0] + R[0, 2], R[2, 1] + R[1, 2], R[2, 2] - R[0, 0] - R[1, 1], R[1, 0] - R[0, 1]],
                  [R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], R[0, 0] + R[1, 1] + R[2, 2]]]) / 3.0
    w, v = np.linalg.eigh(K)
    q = v[:, -1]
    return q if q[3] >= 0 else -q


def quat_to_R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def solve(uv0, uv1, f, cx, cy, opts, defect=None):
    """One problem: dict of status, hyp, best, E, R, t, pose (7,), mask_hypothesis, mask, n_inliers, rec"""
    n = uv0.shape[0]
    out = dict(status=FEW_POINTS, hyp=None, best=-1, E=np.zeros((3, 3)), R=np.eye(3), t=np.zeros(3),
               pose=np.array([0.0, 0, 0, 1, 0, 0, 0]), mask_hypothesis=np.zeros(n, dtype=bool),
               mask=np.zeros(n, dtype=bool), n_inliers=0, rec=None)
    if n < opts["min_points"]:
        return out
    hyp = hypotheses(uv0, uv1, f, cx, cy, opts, defect)
    best = best_hypothesis(hyp, defect)
    out.update(hyp=hyp, best=best, status=NO_HYPOTHESIS)
    if best < 0:
        return out
    x0, x1 = normalise(uv0, f, cx, cy), normalise(uv1, f, cx, cy)
    thr = opts["threshold"] if defect == "threshold_not_normalised" else opts["threshold"] / f
    with np.errstate(invalid="ignore"):
        inl = hyp["e2"][best] <= thr * thr
    rec = recover_pose(hyp["E"][best], x0, x1, inl, opts["distance_threshold"], defect)
    R, t = rec["candidates"][rec["winner"]] if rec["candidates"] is not None else (np.eye(3), np.zeros(3))
    out.update(status=OK if rec["votes"][rec["winner"]] > 0 else NO_POSE, E=hyp["E"][best], R=R, t=t,
               pose=np.concatenate([R_to_quat(R), t]), mask_hypothesis=inl, mask=rec["mask"],
               n_inliers=int(rec["mask"].sum()), rec=rec)
    return out
