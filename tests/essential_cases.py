"""Two-view scenes for the batched essential-matrix RANSAC (sim3opt_essential_batch, ExtractCameras of
kittiDetector.h:279-293) and their reference runs through tests/essential_ref.py.  Shared by
tests/test_essential_ref.py (CPU: the conditions the GPU comparisons rest on hold for every run listed here) and
tests/test_gpu_essential_batch.py (GPU: the kernel reproduces them); every reference run is made once per process.

A case is (n_points, seed) at the fixture's intrinsics (f = 718.856): camera 1 a few degrees of yaw and pitch and about
a metre from camera 0, the points 6-40 m ahead of camera 0, both views' pixels with 0.3 px noise; from 63 points on, a
quarter of camera 1's pixels is moved by a gross error of 40 px.  A (case, options) pair enters RUNS only if
tests/test_essential_ref.py's conditions hold for it; one that does not is replaced by another seed, never compared
more loosely.
"""
import functools

import numpy as np

import essential_ref as ER

FOCAL, CX, CY = 718.856, 607.1928, 185.2157
LDS_POINTS = 1072  # essential_batch.hip stages the correspondences of a problem in LDS up to this many
CHUNK = 16         # ... and makes, then scores, this many hypotheses at a time
NOISE_PX, OUTLIER_SHARE = 0.3, 0.25
# the comparisons run 100 hypotheses unless a run says otherwise, and with min_points = 6 so that the 6-point problem runs
OPTS = dict(ER.DEFAULTS, iterations=100, min_points=6)

# (points, seed): the exact fit 6, the default's smallest 9, around one wavefront's 64 lanes, around one pass of the
# 256-thread stride, and around the LDS staging cap
SIZE_CASES = ((6, 5), (9, 1), (63, 3), (64, 4), (65, 5), (255, 1), (256, 1), (257, 1),
              (LDS_POINTS - 1, 2), (LDS_POINTS, 10), (LDS_POINTS + 1, 1))
# hypothesis counts: one, one below / at / one above the chunk, two chunks + 1, and once the default
ITERATION_COUNTS = (1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1, 1000)
ITERATION_CASE = (65, 5)


def opt_items(**kw):
    return tuple(sorted(kw.items()))


# every (case, options over OPTS) the GPU file compares against the reference
# (seeds chosen by the conditions on the restatement alone: the 1000 hypotheses run on another case than the smaller
# counts)
RUNS = tuple((c, ()) for c in SIZE_CASES) + \
    tuple((ITERATION_CASE if h < 1000 else (65, 2), opt_items(iterations=h)) for h in ITERATION_COUNTS) + \
    (((65, 5), opt_items(seed=4242)), ((255, 6), opt_items(threshold=2.0, distance_threshold=30.0)))
# Known limit of the kernel's solver, asserted as such wherever hypotheses are compared: run -> hypotheses,
# well-conditioned by the restatement, of which the kernel's arithmetic finds fewer real solutions than the restatement
# (two solutions nearly coincide in the coordinate the degree-10 polynomial is in, and its root pair comes out
# complex).  For these the chosen E must still be the restatement's within the limit, and the count no larger.
KNOWN_FEWER_SOLUTIONS = {((65, 5), opt_items(seed=4242)): (33,)}


def exact_count_mask(case, items, well):
    """`well` without the hypotheses of KNOWN_FEWER_SOLUTIONS: where the number of real solutions is compared exactly"""
    out = well.copy()
    out[list(KNOWN_FEWER_SOLUTIONS.get((case, items), ()))] = False
    return out


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
def make_case(n, seed):
    """dict: uv0, uv1 (n, 2), R_true (3, 3), t_true (3,, unit), outlier (n,) bool, points (n, 3) in camera 0's frame"""
    rng = np.random.default_rng(7000 + seed)
    z = rng.uniform(6.0, 40.0, n)
    pts = np.stack([z * rng.uniform(-0.55, 0.55, n), z * rng.uniform(-0.18, 0.18, n), z], axis=1)
    R = rot_xyz(np.deg2rad(rng.uniform(-1.0, 1.0)), np.deg2rad(rng.uniform(2.0, 5.0)) * rng.choice([-1.0, 1.0]),
                np.deg2rad(rng.uniform(-1.0, 1.0)))
    t = -R @ np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.1, 0.1), rng.uniform(0.7, 1.2)])
    uv0 = project(np.eye(3), np.zeros(3), pts) + NOISE_PX * rng.standard_normal((n, 2))
    uv1 = project(R, t, pts) + NOISE_PX * rng.standard_normal((n, 2))
    bad = (rng.random(n) < OUTLIER_SHARE) & (n >= 63)
    ang = rng.uniform(0.0, 2.0 * np.pi, n)
    uv1[bad] += 40.0 * np.stack([np.cos(ang), np.sin(ang)], axis=1)[bad]
    out = dict(uv0=uv0, uv1=uv1, R_true=R, t_true=t / np.linalg.norm(t), scale=float(np.linalg.norm(t)), outlier=bad,
               points=pts)
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
    return ER.solve(case["uv0"], case["uv1"], FOCAL, CX, CY, opts, defect)


@functools.lru_cache(maxsize=None)
def reference(n, seed, items=()):
    """essential_ref.solve of case (n, seed) under OPTS + dict(items), computed once; do not modify the result."""
    return run_reference(make_case(n, seed), merged(items))


def same_up_to_sign(Ea, Eb):
    """max |Ea -+ Eb| per hypothesis, (H,)"""
    a, b = Ea.reshape(len(Ea), -1), Eb.reshape(len(Eb), -1)
    return np.minimum(np.abs(a - b).max(1), np.abs(a + b).max(1))


@functools.lru_cache(maxsize=None)
def conditioning(n, seed, items=()):
    """Per hypothesis of reference(n, seed, items), bool: the action matrices of x and of y give the same solution
    count and the same chosen E to 1e-10, and a relative 1e-13 perturbation of the pixels leaves validity and the
    number of real solutions as they are and moves the chosen E by less than 1e-10.
    Of the two action matrices' solution sets only the size and the chosen member are compared, not every member: this
    calls more hypotheses well-conditioned than a comparison of the whole sets would, so the kernel is held to the
    restatement on more of them, not fewer."""
    opts, c = merged(items), make_case(n, seed)
    ref = reference(n, seed, items)["hyp"]
    other = ER.hypotheses(c["uv0"], c["uv1"], FOCAL, CX, CY, opts, variable="y")
    m = perturbed(c, 1e-13)
    moved = ER.hypotheses(m["uv0"], m["uv1"], FOCAL, CX, CY, opts)
    well = np.ones(len(ref["valid"]), dtype=bool)
    for o in (other, moved):
        well &= (ref["valid"] == o["valid"]) & (ref["n_solutions"] == o["n_solutions"])
        well &= same_up_to_sign(ref["E"], o["E"]) < 1e-10
    return well


def batch_arrays(cases):
    """The flat arrays sim3opt_essential_batch_set_problems takes, for a list of (n, seed)."""
    cs = [make_case(*c) for c in cases]
    ptr = np.concatenate([[0], np.cumsum([c["uv0"].shape[0] for c in cs])]).astype(np.int32)
    return dict(point_ptr=ptr, uv0=np.concatenate([c["uv0"] for c in cs]), uv1=np.concatenate([c["uv1"] for c in cs]))


def rot_angle(Ra, Rb):
    return float(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1.0) / 2.0, -1.0, 1.0)))


def true_essential(case):
    E = ER.skew(case["t_true"]) @ case["R_true"]
    return E / np.linalg.norm(E)


@functools.lru_cache(maxsize=None)
def score_matrices(n, seed):
    """The matrices the scoring operator is given for case (n, seed), (P, 3, 3): the truth, every hypothesis of the
    reference (zero where it has none) and the truth with a zero row, whose denominators can vanish."""
    c, hyp = make_case(n, seed), reference(n, seed)["hyp"]
    zero_row = true_essential(c).copy()
    zero_row[2] = 0.0
    return np.concatenate([true_essential(c)[None], hyp["E"], zero_row[None]])


def reference_scores(case, Es, opts=OPTS):
    """(count (P,), cost (P,), e2 (P, n)) of essential_ref's scoring of Es (P, 3, 3)"""
    x0, x1 = ER.normalise(case["uv0"], FOCAL, CX, CY), ER.normalise(case["uv1"], FOCAL, CX, CY)
    e2 = ER.sampson(Es, x0, x1)
    thr = opts["threshold"] / FOCAL
    with np.errstate(invalid="ignore"):
        inl = e2 <= thr * thr
    return inl.sum(1), np.where(inl, e2, 0.0).sum(1), e2


def swapped(case):
    """The case with the views' roles exchanged: the pose is the inverse, so t points the other way."""
    R, t = case["R_true"].T, -case["R_true"].T @ case["t_true"]
    return dict(case, uv0=case["uv1"], uv1=case["uv0"], R_true=R, t_true=t)


def far_scene(seed=31, n=40):
    """Points 60-80 baselines away, noise-free: in front of both cameras under the true pose, but beyond
    distance_threshold = 50 under every candidate."""
    rng = np.random.default_rng(7000 + seed)
    z = rng.uniform(60.0, 80.0, n)
    pts = np.stack([z * rng.uniform(-0.5, 0.5, n), z * rng.uniform(-0.15, 0.15, n), z], axis=1)
    R = rot_xyz(0.01, 0.05, -0.01)
    t = -R @ np.array([0.3, 0.05, 0.9])
    t = t / np.linalg.norm(t)
    return dict(uv0=project(np.eye(3), np.zeros(3), pts), uv1=project(R, t, pts), R_true=R, t_true=t,
                outlier=np.zeros(n, dtype=bool), points=pts)


POSE_CASE = (65, 5)


@functools.lru_cache(maxsize=None)
def pose_problems():
    """What the pose operator is given, a list of dict(uv0, uv1, E, mask): the planted E of POSE_CASE and of the same
    case with the views exchanged, each under both signs -- the true pose is then each of the four candidates once --
    on the points that are no gross outliers, and the far scene, no point of which votes for anything."""
    out = []
    base = make_case(*POSE_CASE)
    for c in (base, swapped(base)):
        for sign in (1.0, -1.0):
            out.append(dict(uv0=c["uv0"], uv1=c["uv1"], E=sign * true_essential(c), mask=~c["outlier"], R_true=c["R_true"],
                            t_true=c["t_true"]))
    f = far_scene()
    out.append(dict(uv0=f["uv0"], uv1=f["uv1"], E=true_essential(f), mask=np.ones(len(f["uv0"]), dtype=bool),
                    R_true=f["R_true"], t_true=f["t_true"]))
    return out


def reference_pose(p, dist=OPTS["distance_threshold"], defect=None):
    x0, x1 = ER.normalise(p["uv0"], FOCAL, CX, CY), ER.normalise(p["uv1"], FOCAL, CX, CY)
    return ER.recover_pose(p["E"], x0, x1, p["mask"], dist, defect)


def degenerate_problems():
    """(uv0, uv1) of: a healthy problem in which point 1 repeats point 0; twelve pixels on one line in both views;
    twelve times the same pixel pair; eight good points of which point 1 repeats point 0 (with so few, the repeat is
    often a sample's sixth point)."""
    c = make_case(65, 5)
    dup0, dup1 = np.array(c["uv0"]), np.array(c["uv1"])
    dup0[1], dup1[1] = dup0[0], dup1[0]
    s = np.arange(12.0)
    line0 = np.stack([300.0 + 40.0 * s, 100.0 + 10.0 * s], axis=1)
    line1 = np.stack([320.0 + 38.0 * s, 110.0 + 9.5 * s], axis=1)
    same0, same1 = np.tile([[650.0, 200.0]], (12, 1)), np.tile([[640.0, 190.0]], (12, 1))
    good = np.where(~c["outlier"])[0][:8]
    few0, few1 = np.array(c["uv0"][good]), np.array(c["uv1"][good])
    few0[1], few1[1] = few0[0], few1[0]
    return [(dup0, dup1), (line0, line1), (same0, same1), (few0, few1)]


def arrays_of(parts):
    """flat arrays of a list of (uv0, uv1)"""
    return dict(point_ptr=np.concatenate([[0], np.cumsum([len(a) for a, _ in parts])]).astype(np.int32),
                uv0=np.concatenate([a for a, _ in parts]), uv1=np.concatenate([b for _, b in parts]))
