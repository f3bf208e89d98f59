"""Problems of the bundle-adjustment operator tests (tests/test_ba_ref.py on the host, tests/test_gpu_ba_operators.py on
the device) and the PATH CONDITIONS they exist for: each case is there because it drives a kernel of
sim3opt_amd/csrc/ba.hip through one particular path; `facts` measures that from a pattern and the dimensions -- the
host test hands it the restated pattern, the GPU test the one the DEVICE reports --, `check_path` asserts it.

  lists ........ hand-built, 11 cameras.  The pair lists behind the reduced blocks (k_ba_reduced's 64-lane stride) are
                 exactly 0 (the diagonal block of a free camera nobody observes with), 1, 63, 64, 65 and >= 129 pairs
                 long; one point is seen once, one twice by the same camera; nblk % 4 != 0 (the last workgroup is not
                 full); cameras 1 and 10 are fixed, camera 1 shares a point with the free camera 0 (an off-diagonal
                 block with one fixed side).
  branches ..... 8 groups of 3 cameras whose base orientations are I, R_x, R_y, R_z of pi -/+ 0.05 and R_y(2.0), each
                 group on a short baseline with 60 points 8 .. 30 m in front: the cameras fall on all four branches of
                 Eigen's matrix->quaternion rule (R_to_quat in k_ba_update), w takes both signs.
  pcg_1 ... pcg_1030 ... street problems of the oracle's generator with 1, 16, 17, 146, 147 and 1030 cameras: k_ba_pcg's
                 thread-stride loops start at 7 nc > 1024 (147 cameras), the D^-1 loop's at nc > 1024, a wave's second
                 pass over the rows at nc > 16 (uneven at 17).  pcg_1030 is only ever run with an iteration cap <= 20.
  pcg_1030_raw . the generator's 1030-camera problem as it comes (pcg_1030 leaves out the points that start next to a
                 camera, see _pcg): at RAW_LAMBDA_REL a diagonal block of S has a negative pivot -- k_ba_pcg's `!spd`
                 flag at nc > 1024, and the reduced system's kernels at a cancellation of ten digits.
  big_chi_4, big_chi_16 ... a 20-camera street problem's observations tiled 4 and 16 times (fresh pixel noise per copy):
                 more than 256 partial sums for k_ba_final (n_obs > 65 536), k_ba_chi2's grid-stride loop
                 (n_obs > 262 144).  chi2 only.
  big_scale .... 4 cameras, 87 400 points each seen once: k_ba_scale's grid-stride loop (3 np > 262 144).  Used through
                 the update read-out with a supplied step; nothing is solved at that size.
  tiny ......... 8 cameras, 2 points: nc > 3 np, the shared thread index of k_ba_update.
"""
import numpy as np

from oracle import ba_oracle as BO
import ba_ref as BR

F, CX, CY = 718.856, 607.1928, 185.2157
PCG_SIZES = {"pcg_1": 1, "pcg_16": 16, "pcg_17": 17, "pcg_146": 146, "pcg_147": 147, "pcg_1030": 1030}
CASES = ("lists", "branches") + tuple(PCG_SIZES) + ("pcg_1030_raw", "big_chi_4", "big_chi_16", "big_scale", "tiny")
RAW_LAMBDA_REL = 1e-10  # pcg_1030_raw: the damping, relative to the largest diagonal entry, at which S loses definiteness
LISTS_FIXED = (1, 10)
LISTS_LENGTHS = (0, 1, 63, 64, 65)
BRANCH_BASES = (("I", None, 0.0), ("x-", 0, np.pi - 0.05), ("x+", 0, np.pi + 0.05), ("y-", 1, np.pi - 0.05),
                ("y+", 1, np.pi + 0.05), ("z-", 2, np.pi - 0.05), ("z+", 2, np.pi + 0.05), ("y2", 1, 2.0))
BRANCH_OF_BASE = dict(I=3, y2=3, **{"x-": 0, "x+": 0, "y-": 1, "y+": 1, "z-": 2, "z+": 2})  # 3 = the trace branch
PCG_CAP_MAX = 20  # the largest iteration cap pcg_1030 may be run with


def _project(cams, pts, oc, op):
    X = np.einsum("nij,nj->ni", BO.quat_to_R(cams[oc, :4]), pts[op]) + cams[oc, 4:]
    return np.stack([F * X[:, 0] / X[:, 2] + CX, F * X[:, 1] / X[:, 2] + CY], axis=1), X[:, 2]


def _perturb(rng, cams, pts, rot=0.003, trans=0.05, point=0.2):
    """The generator's perturbed start: a small rotation from the left, translation and point noise."""
    n = cams.shape[0]
    upd = np.concatenate([rng.standard_normal((n, 3)) * rot, rng.standard_normal((n, 3)) * trans], axis=1)
    P0 = BO.Problem(cams, pts, [0], [0], [[0, 0]])
    c0, _ = P0.apply(cams, pts, np.concatenate([upd.ravel(), np.zeros(pts.size)]))
    return c0, pts + rng.standard_normal(pts.shape) * point


def _rot(axis, angle):
    if axis is None:
        return np.eye(3)
    c, s = np.cos(angle), np.sin(angle)
    i, j, k = axis, (axis + 1) % 3, (axis + 2) % 3
    M = np.zeros((3, 3))
    M[i, i] = 1
    M[j, j] = M[k, k] = c
    M[k, j], M[j, k] = s, -s
    return M


def _cams_of(Rc2w, centre):
    """(n, 7) T_w2c of cameras with camera-to-world rotations Rc2w (n, 3, 3) at the centres (n, 3)."""
    Rw2c = np.transpose(Rc2w, (0, 2, 1))
    q = BO.R_to_quat(Rw2c)
    return np.concatenate([q / np.linalg.norm(q, axis=1, keepdims=True), -np.einsum("nij,nj->ni", Rw2c, centre)], axis=1)


def _lists():
    rng = np.random.default_rng(101)
    nc = 11
    centre = np.stack([0.4 * np.arange(nc), 0.05 * np.sin(np.arange(nc)), 0.1 * np.cos(np.arange(nc))], axis=1)
    cams = _cams_of(np.tile(np.eye(3), (nc, 1, 1)), centre)
    shared = [(0, 1, 1), (2, 3, 63), (3, 4, 64), (4, 5, 65), (5, 6, 130)]  # (camera, camera, common points)
    oc, op, n = [], [], 0
    for a, b, m in shared:
        for _ in range(m):
            oc += [a, b]
            op += [n, n]
            n += 1
    oc += [7, 7, 7, 8, 10]  # a point seen once (7), a point seen twice by 7 and once by 8, a private point of 10
    op += [n, n + 1, n + 1, n + 1, n + 2]
    n += 3
    oc, op = np.array(oc), np.array(op)
    pts = np.stack([rng.uniform(-5, 7, n), rng.uniform(-2.5, 2.5, n), rng.uniform(8, 30, n)], axis=1)
    uv, depth = _project(cams, pts, oc, op)
    assert (depth > 4).all()
    uv = uv + rng.standard_normal(uv.shape) * 0.5
    bad = rng.random(len(uv)) < 0.03
    uv[bad] += rng.standard_normal((int(bad.sum()), 2)) * 40.0
    c0, p0 = _perturb(rng, cams, pts)
    P = BO.Problem(c0, p0, oc, op, uv)
    P.fixed[list(LISTS_FIXED)] = True
    return P


def _branches():
    rng = np.random.default_rng(202)
    Rs, cs, pts, oc, op = [], [], [], [], []
    for gi, (_, axis, angle) in enumerate(BRANCH_BASES):
        Rg = _rot(axis, angle)
        origin = np.array([100.0 * gi, 0.0, 0.0])
        p = np.stack([rng.uniform(-6, 6, 60), rng.uniform(-2.5, 2.5, 60), rng.uniform(8, 30, 60)], axis=1)
        for k in range(3):
            Rs.append(Rg)
            cs.append(origin + Rg @ np.array([0.5 * k, 0.0, 0.0]))
            oc += [3 * gi + k] * 60
            op += list(range(60 * gi, 60 * gi + 60))
        pts.append(origin + p @ Rg.T)
    cams, pts = _cams_of(np.array(Rs), np.array(cs)), np.concatenate(pts)
    oc, op = np.array(oc), np.array(op)
    uv, depth = _project(cams, pts, oc, op)
    assert (depth > 4).all()
    uv = uv + rng.standard_normal(uv.shape) * 0.5  # (no gross outliers here: the other cases carry them)
    c0, p0 = _perturb(rng, cams, pts)
    P = BO.Problem(c0, p0, oc, op, uv)
    P.fixed[::3] = True  # the first camera of each group
    return P


def _street(n_cams, n_points, seed):
    d = BO.synthetic(n_cams=n_cams, n_points=n_points, seed=seed)
    return BO.Problem(d["cams"], d["points"], d["obs_cam"], d["obs_point"], d["obs_uv"])


def _pcg(nc, raw=False):
    if nc == 1:  # the generator keeps points seen twice: one camera of a pair, its points then seen once
        Q = _street(2, 60, 3)
        keep = Q.oc == 0
        ids, op = np.unique(Q.op[keep], return_inverse=True)
        return BO.Problem(Q.cams[:1], Q.points[ids], Q.oc[keep], op, Q.uv[keep])
    n_points = {16: 150, 17: 150, 146: 500, 147: 500, 1030: 3600}[nc]
    Q = _street(nc, n_points, 5)
    if raw:
        return Q
    # The generator perturbs T_w2c's rotation, which turns a camera about the WORLD origin: 2 km down the street the
    # start is metres off and some points start next to (or behind) a camera that observes them.  Their Jacobians are
    # huge (largest diagonal entry 2e13 against a median of 2e4), and at a damping small enough to leave block-Jacobi CG
    # anything to do the camera's diagonal block of S, A^T A - Y Hpp_inv Y^T, cancels from 1e13 to lambda ~ 2e3: the
    # relative error of Hpp_inv (2e-5 from the cofactor formula at kappa_1 = 7e7, inside its bound) decides its sign,
    # S is not positive definite and the solver reports `fail` -- that is pcg_1030_raw, kept as a case of its own.
    # For the iterates the points starting within 1 m of a camera's plane leave the problem (118 of 2 484 at 1030
    # cameras, none below that; every camera stays observed: asserted with the path condition).
    _, depth = _project(Q.cams, Q.points, Q.oc, Q.op)
    near = np.zeros(Q.points.shape[0], dtype=bool)
    near[Q.op[np.abs(depth) < 1.0]] = True
    keep = ~near[Q.op]
    ids, op = np.unique(Q.op[keep], return_inverse=True)
    return BO.Problem(Q.cams, Q.points[ids], Q.oc[keep], op, Q.uv[keep])


def _tiled(times):
    Q = _street(20, 1500, 1)
    rng = np.random.default_rng(303 + times)
    n = len(Q.oc)
    uv = np.tile(Q.uv, (times, 1))
    uv[n:] += rng.standard_normal((n * (times - 1), 2)) * 2.0  # fresh noise: Huber in- and outliers in every copy
    return BO.Problem(Q.cams, Q.points, np.tile(Q.oc, times), np.tile(Q.op, times), uv)


def _big_scale():
    rng = np.random.default_rng(404)
    nc, n = 4, 87400
    cams = _cams_of(np.tile(np.eye(3), (nc, 1, 1)), np.stack([0.5 * np.arange(nc), np.zeros(nc), np.zeros(nc)], axis=1))
    pts = np.stack([rng.uniform(-6, 6, n), rng.uniform(-2.5, 2.5, n), rng.uniform(8, 30, n)], axis=1)
    oc, op = np.arange(n) % nc, np.arange(n)
    uv, _ = _project(cams, pts, oc, op)
    c0, p0 = _perturb(rng, cams, pts, point=0.05)
    return BO.Problem(c0, p0, oc, op, uv + rng.standard_normal(uv.shape) * 0.5)


def _tiny():
    rng = np.random.default_rng(505)
    nc = 8
    cams = _cams_of(np.tile(np.eye(3), (nc, 1, 1)), np.stack([0.4 * np.arange(nc), np.zeros(nc), np.zeros(nc)], axis=1))
    pts = np.array([[0.5, -0.3, 12.0], [2.0, 0.8, 20.0]])
    oc, op = np.repeat(np.arange(nc), 2), np.tile([0, 1], nc)
    uv, _ = _project(cams, pts, oc, op)
    c0, p0 = _perturb(rng, cams, pts)
    return BO.Problem(c0, p0, oc, op, uv + rng.standard_normal(uv.shape) * 0.5)


_cache = {}


def problem(name):
    """The case's problem (an oracle Problem; built once, do not modify)."""
    if name not in _cache:
        if name == "lists":
            P = _lists()
        elif name == "branches":
            P = _branches()
        elif name in PCG_SIZES:
            P = _pcg(PCG_SIZES[name])
        elif name == "pcg_1030_raw":
            P = _pcg(1030, raw=True)
        elif name.startswith("big_chi_"):
            P = _tiled(int(name[8:]))
        elif name == "big_scale":
            P = _big_scale()
        elif name == "tiny":
            P = _tiny()
        else:
            raise KeyError(name)
        _cache[name] = P
    return _cache[name]


def facts(P, rptr, bcol, dims):
    """What a pattern (the device's, or the restated one) and the dimensions make of a case's problem; rptr = None:
    the dimensions alone."""
    nc, npt, no = (int(v) for v in dims)
    if rptr is None:  # (cases that exist for their sizes alone)
        return dict(nc=nc, np=npt, no=no, seen_once=int((np.bincount(P.op, minlength=npt) == 1).sum()))
    rptr, bcol = np.asarray(rptr), np.asarray(bcol)
    lists = BR.pair_lists(P.oc, P.op, nc)
    assert np.array_equal(lists["rptr"], rptr) and np.array_equal(lists["bcol"], bcol)  # the pattern the lists belong to
    assert np.array_equal(bcol[rptr[:-1]], np.arange(nc))  # the diagonal block first in every row
    brow = lists["brow"]
    fixed = np.asarray(P.fixed, dtype=bool)
    fb = fixed[brow] | fixed[bcol]
    free_len = np.diff(lists["sptr"])[~fb]
    seen = np.bincount(P.op, minlength=npt)
    twice = np.bincount(P.op * nc + P.oc, minlength=npt * nc).max()
    return dict(nc=nc, np=npt, no=no, nblk=int(bcol.shape[0]), free_lengths=sorted(set(int(v) for v in free_len)),
                max_len=int(free_len.max()) if free_len.size else 0, seen_once=int((seen == 1).sum()),
                same_camera_twice=int(twice), one_side_fixed=int((fixed[brow] != fixed[bcol]).sum()),
                n_fixed=int(fixed.sum()), cams_observed=int((np.bincount(P.oc, minlength=nc) > 0).sum()))


def check_path(name, f):
    """The condition case `name` exists for, asserted on facts(...)."""
    if name == "lists":
        assert all(m in f["free_lengths"] for m in LISTS_LENGTHS) and f["max_len"] >= 129, f
        assert f["seen_once"] >= 1 and f["same_camera_twice"] == 2 and f["nblk"] % 4 != 0, f
        assert f["n_fixed"] == 2 and f["one_side_fixed"] >= 2, f
    elif name == "branches":
        assert (f["nc"], f["np"], f["no"]) == (24, 480, 1440), f
    elif name in PCG_SIZES:
        nc = PCG_SIZES[name]
        assert f["nc"] == nc and f["cams_observed"] == nc, f
        assert (7 * nc > 1024) == (nc >= 147) and (nc > 1024) == (name == "pcg_1030"), f
        assert (nc > 16 and nc % 16 != 0) == (name in ("pcg_17", "pcg_146", "pcg_147", "pcg_1030")), f
    elif name == "pcg_1030_raw":
        assert f["nc"] == 1030 > 1024 and f["cams_observed"] == 1030, f
    elif name == "big_chi_4":
        assert 65536 < f["no"] <= 262144, f      # > 256 partial sums, one pass of the grid
    elif name == "big_chi_16":
        assert f["no"] > 262144, f               # the grid-stride loop of k_ba_chi2
    elif name == "big_scale":
        assert 3 * f["np"] > 262144 and f["seen_once"] == f["np"], f
    elif name == "tiny":
        assert f["nc"] > 3 * f["np"], f
    else:
        raise KeyError(name)


def describe(name, f):
    return f"[ba-op] {name}: " + ", ".join(f"{k} {v}" for k, v in f.items())


# ---------------------------------------------------------------------------------------------- supplied steps
def update_steps(P, seed=7):
    """Steps (name -> dx_c (nc, 7), dx_p (np, 3)) for the update test on `branches`: omega = 0; |omega| just below
    and just above the small-angle threshold 1e-5 with |upsilon| ~ 1 (the two V formulas differ by ~ 5e-7 there);
    |omega| ~ 0.3; |omega| = pi - 1e-3; `carry_<b>`: for every camera a rotation that takes it from
    where it is onto the axis-angle pi - 0.05 orientation of branch b (so cameras of the trace branch land on the
    other three), and `back`: the rotation that takes every camera to the identity (the cameras of the other three
    branches land on the trace branch)."""
    rng = np.random.default_rng(seed)
    nc, npt = P.cams.shape[0], P.points.shape[0]

    def mk(omega, ups=None):
        x = np.zeros((nc, 7))
        x[:, :3] = omega
        x[:, 3:6] = rng.standard_normal((nc, 3)) if ups is None else ups
        return x, rng.standard_normal((npt, 3)) * 0.1

    unit = rng.standard_normal((nc, 3))
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    steps = {"omega0": mk(0.0), "below": mk(0.99e-5 * unit), "above": mk(1.01e-5 * unit), "mid": mk(0.3 * unit),
             "near_pi": mk((np.pi - 1e-3) * unit)}
    Rcur = BO.quat_to_R(P.cams[:, :4])
    for b in range(3):
        steps[f"carry_{b}"] = mk(_log(_rot(b, np.pi - 0.05) @ np.transpose(Rcur, (0, 2, 1))))  # exp(w) R = target
    steps["back"] = mk(_log(np.transpose(Rcur, (0, 2, 1))))                                    # exp(w) R = I
    return steps


def _log(Rm):
    """Rotation vectors of (n, 3, 3) rotations with angles away from 0 and pi (enough for the cases above)."""
    Rm = np.broadcast_to(Rm, (Rm.shape[0] if Rm.ndim == 3 else 1, 3, 3))
    th = np.arccos(np.clip((np.trace(Rm, axis1=1, axis2=2) - 1) / 2, -1, 1))
    v = np.stack([Rm[:, 2, 1] - Rm[:, 1, 2], Rm[:, 0, 2] - Rm[:, 2, 0], Rm[:, 1, 0] - Rm[:, 0, 1]], axis=1)
    s = np.sin(th)
    ok = s > 1e-9
    return np.where(ok[:, None], v * (th / np.where(ok, 2 * s, 1))[:, None], 0.0)


# ---------------------------------------------------------------------------------------------- PCG iterates
ITERATE_CAPS = (1, 2, 5, 20)
ITERATE_LAMBDA_REL = 1e-6   # damping relative to the largest diagonal entry: block-Jacobi CG still moves at k = 20
ITERATE_FLOOR = 1e-6        # smallest |r_k|_M / |r_0|_M the reference may reach at the largest cap
PCG_REL_TOL = 1e-150        # tol^2 = 1e-300 is a normal double and no iterate comes near it: the cap stops the solve

