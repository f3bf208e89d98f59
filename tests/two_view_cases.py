"""Two-view problems for the batched refinement (sim3opt_ba_batch, BAOptimize of kittiDetector.h:845-954) and
their reference runs through oracle/ba_oracle.py's Problem (camera 0 fixed, Huber 3, lambda_0 = 50, 5 trials, 10
iterations -- the detector's configuration).  Shared by tests/test_two_view_batch.py (CPU: the cases are stable)
and tests/test_gpu_two_view_batch.py (GPU: the kernel reproduces them); every reference run is made once per process.

A case is (n_points, seed), or (n_points, seed, gauge): the same problem in a world moved by GAUGES[gauge], where
camera 0 is not the identity and camera 1 sits on another branch of the matrix -> quaternion rule (BRANCH_CASES).
Camera 0 sits at the identity, camera 1 a few degrees of yaw and about a metre
away; the points lie 6-40 m ahead; observations carry 0.5 px noise, about 5 % of the points a gross outlier in one
view; the start (camera 1 and the depths of the points) is perturbed so that the first iterations move.

Trial counts are a discontinuous function of the inputs.  A case enters the lists below only if the oracle's
trial counts survive a relative 1e-13 perturbation of its inputs, and if that perturbation moves none of the oracle's
per-observation chi2 by more than 2e-8 relative -- a fifth of the 1e-7 they are compared at: a reference that answers
input noise of 1e-13 with more cannot carry that comparison (tests/test_two_view_batch.py asserts both for every
case and every option set used).  A case that does not is replaced by another seed, never compared more loosely:
(65, 16) was, whose run without a robust kernel moves one observation's chi2 by 6e-8 under the perturbation.
"""
import functools

import numpy as np

from oracle import ba_oracle as BO

FOCAL, CX, CY = 718.856, 607.1928, 185.2157
DEFAULTS = dict(max_iters=10, huber_delta=3.0, pixel_noise=1.0, tau=1e-5, user_lambda_init=50.0, max_trials=5,
                outlier_chi2=5.995)

# (points, seed).  One iteration: around one, two and three passes of the kernel's 256-thread stride, the detector's
# largest candidate (1047 points, five passes; seed 22 was tried first and moves an observation's chi2 by 5.5e-8 under
# the perturbation), and the degenerate sizes 1 and 2 (whose full traces are rounding noise: chi2 reaches zero).
ONE_ITERATION_CASES = ((1, 11), (2, 12), (5, 13), (63, 14), (64, 15), (65, 24), (255, 17), (256, 18), (257, 19),
                       (513, 20), (1047, 23))
WHOLE_RUN_CASES = ONE_ITERATION_CASES[2:]
# more workgroups than compute units: 30 distinct small problems, cycled to 300
MANY_CASES = tuple((5 + (7 * k) % 16, 100 + k) for k in range(30))
# the option sets of the whole-run comparisons (merged over DEFAULTS)
OPTION_SETS = (dict(), dict(huber_delta=0.0), dict(pixel_noise=2.0), dict(user_lambda_init=0.0))


def _yaw_w2c(yaw):
    c, s = np.cos(yaw), np.sin(yaw)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]).T


def _project(R, t, p):
    X = p @ R.T + t
    return np.stack([FOCAL * X[:, 0] / X[:, 2] + CX, FOCAL * X[:, 1] / X[:, 2] + CY], axis=1)


def _axis_rotation(axis, angle):
    c, s = np.cos(angle), np.sin(angle)
    i, j, k = axis, (axis + 1) % 3, (axis + 2) % 3
    G = np.zeros((3, 3))
    G[i, i], G[j, j], G[j, k], G[k, j], G[k, k] = 1.0, c, -s, s, c
    return G


# The gauges of BRANCH_CASES: the world moved by (G, t_g), name -> G.  A rotation by nearly pi about an axis puts a
# camera that looks along the old axes on that axis' branch of Eigen's matrix -> quaternion rule, with w of either
# sign on the two sides of pi; R_y(2) leaves the trace barely positive.
GAUGES = {"x-": _axis_rotation(0, np.pi - 0.05), "x+": _axis_rotation(0, np.pi + 0.05),
          "y-": _axis_rotation(1, np.pi - 0.05), "y+": _axis_rotation(1, np.pi + 0.05),
          "z-": _axis_rotation(2, np.pi - 0.05), "z+": _axis_rotation(2, np.pi + 0.05), "y2": _axis_rotation(1, 2.0)}
GAUGE_SHIFT = np.array([3.0, -2.0, 5.0])
# gauge -> the branch (0, 1, 2 = x, y, z, 3 = trace) camera 1 starts AND ends on; tests assert it on the host
GAUGE_BRANCH = {"x-": 0, "x+": 0, "y-": 1, "y+": 1, "z-": 2, "z+": 2, "y2": 3}
BRANCH_BASE = (65, 24)
# case (65, 24) re-expressed in each moved world: camera 0 is no longer the identity
BRANCH_CASES = tuple(BRANCH_BASE + (g,) for g in GAUGES)

# the read-out's batch: around one wavefront, the first point of wavefront 3 (193), one to five passes of the
# 256-thread stride (1047 = the detector's largest candidate)
READOUT_CASES = ((1, 11), (2, 12), (5, 13), (63, 14), (64, 15), (65, 24), (193, 21), (255, 17), (256, 18), (257, 19),
                 (513, 20), (1047, 23))


def _regauged(case, G):
    """The case in the world moved by (G, GAUGE_SHIFT): points -> G p + t_g, cameras -> T o (G, t_g)^-1."""
    out = dict(case)
    for k in ("points", "points_true"):
        out[k] = case[k] @ G.T + GAUGE_SHIFT
    for k in ("cam0", "cam1", "cam1_true"):
        Rn = BO.quat_to_R(case[k][:4]) @ G.T
        out[k] = np.concatenate([BO.R_to_quat(Rn), case[k][4:] - Rn @ GAUGE_SHIFT])
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def make_case(n, seed, gauge=None):
    """dict: cam0, cam1 (7,), points (n, 3), uv0, uv1 (n, 2) -- the start -- and cam1_true, points_true.  gauge: a key
    of GAUGES, the same problem in a moved world."""
    if gauge is not None:
        return _regauged(make_case(n, seed), GAUGES[gauge])
    rng = np.random.default_rng(seed)
    z = rng.uniform(6.0, 40.0, n)
    pts = np.stack([z * rng.uniform(-0.55, 0.55, n), z * rng.uniform(-0.18, 0.18, n), z], axis=1)
    yaw = np.deg2rad(rng.uniform(2.0, 5.0)) * rng.choice([-1.0, 1.0])
    R1 = _yaw_w2c(yaw)
    t1 = -R1 @ np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.05, 0.05), rng.uniform(0.7, 1.2)])
    uv0 = _project(np.eye(3), np.zeros(3), pts) + 0.5 * rng.standard_normal((n, 2))
    uv1 = _project(R1, t1, pts) + 0.5 * rng.standard_normal((n, 2))
    bad = rng.random(n) < 0.05
    view = rng.random(n) < 0.5
    gross = 40.0 * rng.standard_normal((n, 2))
    uv0[bad & view] += gross[bad & view]
    uv1[bad & ~view] += gross[bad & ~view]
    # the start: camera 1 and the depths perturbed
    dq = np.concatenate([0.004 * rng.standard_normal(3), [1.0]])
    dq /= np.linalg.norm(dq)
    Rs = BO.quat_to_R(dq) @ R1
    cam1 = np.concatenate([BO.R_to_quat(Rs), t1 + 0.05 * rng.standard_normal(3)])
    cam1[:4] /= np.linalg.norm(cam1[:4])
    cam1_true = np.concatenate([BO.R_to_quat(R1), t1])
    start = pts * (1.0 + 0.04 * rng.standard_normal(n))[:, None]
    out = dict(cam0=np.array([0.0, 0, 0, 1, 0, 0, 0]), cam1=cam1, points=start, uv0=uv0, uv1=uv1,
               cam1_true=cam1_true, points_true=pts)
    for v in out.values():
        v.setflags(write=False)
    return out


def perturbed(case, rel=1e-13, seed=999):
    """The case with every input number moved by a relative `rel` (camera 0 stays the identity)."""
    rng = np.random.default_rng(seed)
    out = dict(case)
    for k in ("cam1", "points", "uv0", "uv1"):
        out[k] = case[k] * (1.0 + rel * rng.uniform(-1.0, 1.0, case[k].shape))
    return out


def oracle_problem(case, opts):
    n = case["points"].shape[0]
    P = BO.Problem(np.stack([case["cam0"], case["cam1"]]), case["points"], np.tile([0, 1], n),
                   np.repeat(np.arange(n), 2), np.stack([case["uv0"], case["uv1"]], axis=1).reshape(-1, 2),
                   focal=FOCAL, cx=CX, cy=CY, huber=opts["huber_delta"], pixel_noise=opts["pixel_noise"])
    P.fixed[0] = True
    return P


def run_oracle(case, opts):
    """The reference run: dict with chi2_before (robust, at the start), active_before / active_after (g2o's
    activeChi2), trace (per iteration: chi2, lam, trials, rho), cam1, points, edge_chi2 (n, 2)."""
    P = oracle_problem(case, opts)
    e = P.residuals()
    out = dict(chi2_before=P.chi2(), active_before=float(P.omega * (e * e).sum()))
    out["trace"] = P.optimize(opts["max_iters"], tau=opts["tau"], max_trials=opts["max_trials"],
                              lam0=opts["user_lambda_init"])
    e = P.residuals()
    out["edge_chi2"] = (P.omega * (e * e).sum(1)).reshape(-1, 2)
    out["active_after"] = float(out["edge_chi2"].sum())
    out["cam1"], out["points"] = P.cams[1].copy(), P.points.copy()
    return out


def merged(**kw):
    o = dict(DEFAULTS)
    o.update(kw)
    return o


@functools.lru_cache(maxsize=None)
def _reference(case, opt_items):
    return run_oracle(make_case(*case), merged(**dict(opt_items)))


def reference(*case_and_opts):
    """reference(*case) or reference(*case, opt_items): run_oracle of the case (n, seed) or (n, seed, gauge) under
    DEFAULTS + dict(opt_items), computed once; do not modify the result."""
    if isinstance(case_and_opts[-1], tuple):
        return _reference(tuple(case_and_opts[:-1]), case_and_opts[-1])
    return _reference(tuple(case_and_opts), ())


def run_oracle_continued(case, opts, iters=(4, 6)):
    """optimize() with max_iters = iters[0], then again with iters[1] from where it stopped, each call starting at
    lambda_0 and ni = 2 as a fresh sim3opt_ba_batch_optimize does: list of dicts (trace, cam1, points, edge_chi2,
    chi2_before, active_before, active_after), one per call."""
    P = oracle_problem(case, opts)
    out = []
    for n in iters:
        e = P.residuals()
        r = dict(chi2_before=P.chi2(), active_before=float(P.omega * (e * e).sum()))
        r["trace"] = P.optimize(n, tau=opts["tau"], max_trials=opts["max_trials"], lam0=opts["user_lambda_init"])
        e = P.residuals()
        r["edge_chi2"] = (P.omega * (e * e).sum(1)).reshape(-1, 2)
        r["active_after"] = float(r["edge_chi2"].sum())
        r["cam1"], r["points"] = P.cams[1].copy(), P.points.copy()
        out.append(r)
    return out


CONTINUED_CASES = ((65, 24), (257, 19))
CONTINUED_ITERS = (4, 6)


@functools.lru_cache(maxsize=None)
def continued_reference(n, seed):
    return run_oracle_continued(make_case(n, seed), DEFAULTS, CONTINUED_ITERS)


def degenerate_case(seed=31, n=12, bad=7):
    """A problem whose sums are not finite: camera 1 has the identity rotation and t_z = -p_z of point `bad`, so that
    X_z = 0 exactly in camera 1 (p_z + (-p_z) is exact) and the projection divides by zero."""
    c = {k: np.array(v) for k, v in make_case(n, seed).items()}
    c["cam1"] = np.array([0.0, 0.0, 0.0, 1.0, 0.3, -0.02, -c["points"][bad, 2]])
    return c


NEAR_POINT = (193, 21, 192, 0.02)


def near_point_case():
    """Case (193, 21) with point 192 -- the one point wavefront 3 owns -- pulled along its ray from camera 0 to a depth
    of 2 cm: its H_pp (about (f / z)^2 = 1e9) is then larger than every diagonal entry of camera 1's sum A_1^T A_1, so
    that computeLambdaInit's maximum is a POINT's, and the fourth wavefront's (tests assert both on the host)."""
    n, seed, i, depth = NEAR_POINT
    c = {k: np.array(v) for k, v in make_case(n, seed).items()}
    c["points"][i] *= depth / c["points"][i, 2]
    return c


def arrays_of(cs):
    """batch_arrays for case dicts."""
    ptr = np.concatenate([[0], np.cumsum([c["points"].shape[0] for c in cs])]).astype(np.int32)
    cat = lambda k: np.concatenate([c[k] for c in cs])
    return dict(point_ptr=ptr, cam0=np.stack([c["cam0"] for c in cs]), cam1=np.stack([c["cam1"] for c in cs]),
                points=cat("points"), uv0=cat("uv0"), uv1=cat("uv1"))


def normalised(cams):
    """Cameras (n, 7) with unit quaternions, by the statements of sim3opt_ba_batch_set_problems (the sum of squares left
    to right, one square root, four divisions): what the kernel computes with.  The handle returns camera 1 so, and
    camera 0 as given."""
    c = np.array(cams, dtype=np.float64).reshape(-1, 7)
    q = c[:, :4].copy()
    nq = np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
    c[:, :4] = q / nq[:, None]
    return c


def ref_batch(arrays, cams1=None, points=None, opts=DEFAULTS):
    """tests/ba_ref.py's TwoViewBatch of set_problems arrays, at the estimate (cams1, points) if given."""
    import ba_ref as BR
    return BR.TwoViewBatch(arrays["point_ptr"], arrays["cam0"], arrays["cam1"] if cams1 is None else cams1,
                           arrays["points"] if points is None else points, arrays["uv0"], arrays["uv1"], FOCAL, CX,
                           CY, huber=opts["huber_delta"], pixel_noise=opts["pixel_noise"])


def trial_steps(cam1):
    """Supplied camera steps [omega, upsilon] for the read-out, name -> (n, 6), for n cameras cam1 (n, 7) that sit on
    the branches GAUGE_BRANCH lists (BRANCH_CASES in order): omega = 0; |omega| on either side of SE3Quat::exp's 1e-5;
    0.3; pi - 1e-3; and carry_next / carry_prev, the rotation that takes camera k onto the start rotation of the
    first camera of the next / previous branch (x -> y -> z -> trace -> x), so that every pair of neighbouring
    branches is crossed in both directions."""
    from scipy.spatial.transform import Rotation
    n = cam1.shape[0]
    rng = np.random.default_rng(77)
    axis = rng.standard_normal((n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    ups = 0.05 * rng.standard_normal((n, 3))
    steps = {name: np.concatenate([th * axis, ups], axis=1)
             for name, th in (("omega0", 0.0), ("below", 0.99e-5), ("above", 1.01e-5), ("mid", 0.3),
                              ("near_pi", np.pi - 1e-3))}
    branch = [GAUGE_BRANCH[g] for g in GAUGES]
    Rc = BO.quat_to_R(cam1[:, :4])
    first = {b: Rc[branch.index(b)] for b in range(4)}
    for name, d in (("carry_next", 1), ("carry_prev", -1)):
        om = np.stack([Rotation.from_matrix(first[(branch[k] + d) % 4] @ Rc[k].T).as_rotvec() for k in range(n)])
        steps[name] = np.concatenate([om, ups], axis=1)
    return steps


def batch_arrays(cases):
    """The flat arrays sim3opt_ba_batch_set_problems takes, for a list of (n, seed)."""
    return arrays_of([make_case(*c) for c in cases])


def quat_dist(a, b):
    """max over rows of min(|a - b|, |a + b|): q and -q are one rotation"""
    a, b = np.atleast_2d(a), np.atleast_2d(b)
    return float(np.minimum(np.abs(a - b).max(1), np.abs(a + b).max(1)).max())
