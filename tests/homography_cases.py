"""Planar two-view scenes for the batched homography stage (sim3opt_homography_batch, HomographyInit::Compute of
kittiDetector.h:1387-1443) and their reference runs through tests/homography_ref.py.  Shared by
tests/test_homography_ref.py (CPU: the conditions the GPU comparisons rest on hold for every run listed here) and
tests/test_gpu_homography_batch.py (GPU: the kernel reproduces them); every reference run is made once per process.

A case is (n_points, seed) or (n_points, seed, "dup") at the fixture's intrinsics (f = 718.856): the points lie on a
tilted plane 6-40 m ahead of camera 0, camera 1 is a few degrees of yaw and pitch and about a metre away, both views'
pixels carry 0.3 px noise; from 63 points on, a quarter of camera 1's pixels is moved by a gross error of 40 px.  "dup"
repeats every fourth match once (the next row is a copy), so that squared errors tie.  A (case, options) pair enters
RUNS only if tests/test_homography_ref.py's conditions hold for it; one that does not is replaced by another seed,
never compared more loosely.
"""
import functools

import numpy as np

import homography_ref as HR

FOCAL, CX, CY = 718.856, 607.1928, 185.2157
LDS_POINTS = 1072  # homography_batch.hip stages the correspondences of a problem in LDS up to this many
CHUNK = 256        # ... and makes, then scores, this many hypotheses at a time
NOISE_PX, OUTLIER_SHARE = 0.3, 0.25
# the comparisons run 64 hypotheses unless a run says otherwise
OPTS = dict(HR.DEFAULTS, iterations=64)

# (points, seed): the default's smallest 10, around one wavefront's 64 lanes, around one pass of the 256-thread stride,
# around the LDS staging cap; then the duplicated matches
SIZE_CASES = ((10, 1), (63, 1), (64, 1), (65, 1), (255, 1), (256, 1), (257, 1),
              (LDS_POINTS - 1, 1), (LDS_POINTS, 1), (LDS_POINTS + 1, 1), (66, 2, "dup"))
# hypothesis counts: one, one below / at / one above the chunk, two chunks + 1, and once the default
ITERATION_COUNTS = (1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1, 300)
ITERATION_CASE = {1: (65, 1), 300: (257, 2)}


def opt_items(**kw):
    return tuple(sorted(kw.items()))


# every (case, options over OPTS) the GPU file compares against the reference
RUNS = tuple((c, ()) for c in SIZE_CASES) + \
    tuple((ITERATION_CASE.get(h, (65, 1)), opt_items(iterations=h)) for h in ITERATION_COUNTS) + \
    (((65, 1), opt_items(seed=4242)), ((255, 2), opt_items(max_pixel_error=2.0)))


def merged(items=()):
    o = dict(OPTS)
    o.update(dict(items))
    return o


def rot_xyz(rx, ry, rz):
    cx_, sx = np.cos(rx), np.sin(rx)
    cy_, sy = np.cos(ry), np.sin(ry)
    cz, sz = np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx_, -sx], [0, sx, cx_]])
    Ry = np.array([[cy_, 0, sy], [0, 1, 0], [-sy, 0, cy_]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def project(R, t, X):
    Y = X @ R.T + t
    return np.stack([FOCAL * Y[:, 0] / Y[:, 2] + CX, FOCAL * Y[:, 1] / Y[:, 2] + CY], axis=1)


@functools.lru_cache(maxsize=None)
def make_case(n, seed, dup=None):
    """dict: uv0, uv1 (n, 2), R_true (3, 3), t_true (3,; unit), n_true (3,; the plane's unit normal in camera 0's
    frame), outlier (n,) bool, points (n, 3) in camera 0's frame"""
    rng = np.random.default_rng(9000 + seed)
    a = rng.uniform(0.5, 1.0) * rng.choice([-1.0, 1.0])
    b, z0 = rng.uniform(-0.3, 0.3), rng.uniform(12.0, 16.0)
    xn, yn = rng.uniform(-0.55, 0.55, n), rng.uniform(-0.18, 0.18, n)
    z = z0 / (1.0 - a * xn - b * yn)  # the plane z = z0 + a x + b y
    pts = np.stack([z * xn, z * yn, z], axis=1)
    R = rot_xyz(np.deg2rad(rng.uniform(-1.0, 1.0)), np.deg2rad(rng.uniform(2.0, 5.0)) * rng.choice([-1.0, 1.0]),
                np.deg2rad(rng.uniform(-1.0, 1.0)))
    t = -R @ np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.1, 0.1), rng.uniform(0.7, 1.2)])
    uv0 = project(np.eye(3), np.zeros(3), pts) + NOISE_PX * rng.standard_normal((n, 2))
    uv1 = project(R, t, pts) + NOISE_PX * rng.standard_normal((n, 2))
    bad = (rng.random(n) < OUTLIER_SHARE) & (n >= 63)
    ang = rng.uniform(0.0, 2.0 * np.pi, n)
    uv1[bad] += 40.0 * np.stack([np.cos(ang), np.sin(ang)], axis=1)[bad]
    if dup:
        for k in range(0, n - 1, 4):
            uv0[k + 1], uv1[k + 1], bad[k + 1], pts[k + 1] = uv0[k], uv1[k], bad[k], pts[k]
    normal = np.array([-a, -b, 1.0])
    out = dict(uv0=uv0, uv1=uv1, R_true=R, t_true=t / np.linalg.norm(t), n_true=normal / np.linalg.norm(normal),
               scale=float(np.linalg.norm(t)), outlier=bad, points=pts)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def perturbed(case, rel, seed=999):
    """The case with every pixel moved by a relative `rel`."""
    rng = np.random.default_rng(seed)
    out = dict(case)
    for k in ("uv0", "uv1"):
        out[k] = case[k] * (1.0 + rel * rng.uniform(-1.0, 1.0, case[k].shape))
    return out


def run_reference(case, opts, defect=None):
    return HR.solve(case["uv0"], case["uv1"], FOCAL, CX, CY, opts, defect)


@functools.lru_cache(maxsize=None)
def reference(case, items=()):
    """homography_ref.solve of `case` under OPTS + dict(items), computed once; do not modify the result."""
    return run_reference(make_case(*case), merged(items))


def same_up_to_sign(Ha, Hb):
    """max |Ha -+ Hb| per matrix, (H,)"""
    a, b = Ha.reshape(-1, 9), Hb.reshape(-1, 9)
    return np.minimum(np.abs(a - b).max(1), np.abs(a + b).max(1))


@functools.lru_cache(maxsize=None)
def conditioning(case, items=()):
    """Per hypothesis of reference(case, items), bool: a relative 1e-13 perturbation of the pixels leaves its validity as
    it is and moves H by less than 1e-10."""
    opts, c = merged(items), make_case(*case)
    ref = reference(case, items)["hyp"]
    m = perturbed(c, 1e-13)
    moved = HR.hypotheses(m["uv0"], m["uv1"], FOCAL, CX, CY, opts)
    return (ref["valid"] == moved["valid"]) & (same_up_to_sign(ref["H"], moved["H"]) < 1e-10)


def normalised(case):
    return HR.normalise(case["uv0"], FOCAL, CX, CY), HR.normalise(case["uv1"], FOCAL, CX, CY)


def batch_arrays(cases):
    """The flat arrays sim3opt_homography_batch_set_problems takes, for a list of cases."""
    return arrays_of([(make_case(*c)["uv0"], make_case(*c)["uv1"]) for c in cases])


def arrays_of(parts):
    """flat arrays of a list of (uv0, uv1)"""
    return dict(point_ptr=np.concatenate([[0], np.cumsum([len(a) for a, _ in parts])]).astype(np.int32),
                uv0=np.concatenate([a for a, _ in parts]), uv1=np.concatenate([b for _, b in parts]))


def rot_angle(Ra, Rb):
    return float(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1.0) / 2.0, -1.0, 1.0)))


def angle(a, b):
    return float(np.arccos(np.clip(np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b)), -1.0, 1.0)))


def truth_errors(R, t, n, c):
    """(rotation, direction of t, plane normal up to sign) against the planted truth [rad]"""
    an = angle(n, c["n_true"])
    return rot_angle(R, c["R_true"]), angle(t, c["t_true"]), min(an, np.pi - an)


def true_homography(c):
    """R + t n^T / d of the planted scene (the plane is n . X = d in camera 0's frame), Frobenius norm 1"""
    d = float(c["n_true"] @ c["points"][0])
    H = c["R_true"] + np.outer(c["t_true"] * c["scale"], c["n_true"]) / d
    return H / np.linalg.norm(H)


@functools.lru_cache(maxsize=None)
def score_matrices(case):
    """what the scoring operator is given for a case, (P, 3, 3): the planted H, every hypothesis of the reference, the
    identity"""
    return np.concatenate([true_homography(make_case(*case))[None], reference(case)["hyp"]["H"], np.eye(3)[None]])


def mirror_index(k):
    """the decomposition of -H that is decomposition k of H"""
    return (k & 4) | (3 - (k & 3))


WIDE_UNAMBIGUOUS, WIDE_AMBIGUOUS = (0, 1, 3, 9), (4, 5)


@functools.lru_cache(maxsize=None)
def wide_scene(seed, n=80):
    """A plane seen under a wide angle (camera-plane coordinates up to 1.5) and a baseline of about half its distance,
    view 1 = the planted homography of view 0 plus 0.3 px noise: dict of uv0, uv1, H (Frobenius norm 1), R_true,
    t_true (unit), n_true.  Here the second visibility test tells the two Faugeras-Lustman solutions apart for the seeds
    of WIDE_UNAMBIGUOUS (dRatio < 0.9) and does not for WIDE_AMBIGUOUS."""
    rng = np.random.default_rng(9200 + seed)
    x0 = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.0, 1.0, n)], axis=1)
    nrm = np.array([rng.uniform(-0.6, 0.6), rng.uniform(-0.6, 0.6), 1.0])
    nrm /= np.linalg.norm(nrm)
    R = rot_xyz(*np.deg2rad(rng.uniform(-8, 8, 3)))
    t = rng.uniform(-0.6, 0.6, 3)
    H = R + np.outer(t, nrm)  # (the plane at distance 1)
    p = np.concatenate([x0, np.ones((n, 1))], axis=1) @ H.T
    uv0 = FOCAL * x0 + [CX, CY]
    uv1 = FOCAL * (p[:, :2] / p[:, 2:]) + [CX, CY] + NOISE_PX * rng.standard_normal((n, 2))
    return dict(uv0=uv0, uv1=uv1, H=H / np.linalg.norm(H), R_true=R, t_true=t / np.linalg.norm(t), n_true=nrm)


def supplied_problems():
    """What the decomposition operator is given, a list of dict(uv0, uv1, H, mask): the wide scenes of both branches
    under both signs of H with every point an inlier, two listed cases with the restatement's refined H and inliers,
    and the identity (exactly degenerate) on a listed case's points."""
    out = []
    for seed in WIDE_UNAMBIGUOUS + WIDE_AMBIGUOUS:
        w = wide_scene(seed)
        for sign in (1.0, -1.0):
            out.append(dict(uv0=w["uv0"], uv1=w["uv1"], H=sign * w["H"], mask=np.ones(len(w["uv0"]), dtype=bool)))
    for case in ((65, 1), (257, 1)):
        c, ref = make_case(*case), reference(case)
        out.append(dict(uv0=c["uv0"], uv1=c["uv1"], H=ref["H_refined"], mask=ref["mask"]))
    c = make_case(65, 1)
    out.append(dict(uv0=c["uv0"], uv1=c["uv1"], H=np.eye(3), mask=np.ones(65, dtype=bool)))
    return out


def reference_choice(p, max_pixel_error=OPTS["max_pixel_error"], defect=None):
    x0, x1 = HR.normalise(p["uv0"], FOCAL, CX, CY), HR.normalise(p["uv1"], FOCAL, CX, CY)
    return HR.choose(p["H"], x0, x1, np.asarray(p["mask"], dtype=bool), max_pixel_error ** 2, defect)


NO_INLIERS_ERROR = 1e-200  # a max_pixel_error whose square is zero: nothing is an inlier, every cost is zero
CAP_ERROR = 0.001          # ... and one at which the Sampson cap 4 max_pixel_error^2 (camera-plane units) binds


def cap_problem():
    """wide scene 4 with ten of view 1's pixels moved by 40 px: their Sampson errors exceed 4 x CAP_ERROR^2"""
    w = wide_scene(4)
    uv1 = np.array(w["uv1"])
    uv1[:10] += 40.0
    return dict(uv0=w["uv0"], uv1=uv1, H=w["H"], mask=np.ones(len(uv1), dtype=bool))


def degenerate_problems():
    """(uv0, uv1) of: twelve pixels on one line in both views (no sample is valid); twelve times the same pixel pair
    (likewise); nine points of a healthy case (fewer than min_points)."""
    s = np.arange(12.0)
    line0 = np.stack([300.0 + 40.0 * s, 100.0 + 10.0 * s], axis=1)
    line1 = np.stack([320.0 + 38.0 * s, 110.0 + 9.5 * s], axis=1)
    same0, same1 = np.tile([[650.0, 200.0]], (12, 1)), np.tile([[640.0, 190.0]], (12, 1))
    c = make_case(65, 1)
    return [(line0, line1), (same0, same1), (np.array(c["uv0"][:9]), np.array(c["uv1"][:9]))]


def scattered_problem(n=40, seed=5):
    """pixels with no relation between the views: the best homography has fewer than four inliers at 0.05 px"""
    rng = np.random.default_rng(9100 + seed)
    uv0 = np.stack([rng.uniform(100, 1100, n), rng.uniform(40, 330, n)], axis=1)
    uv1 = np.stack([rng.uniform(100, 1100, n), rng.uniform(40, 330, n)], axis=1)
    return uv0, uv1
