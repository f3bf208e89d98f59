"""PnP problems for the batched RANSAC (sim3opt_pnp_batch, cv::solvePnPRansac of kittiDetector.h:1300-1301) and their
reference runs through tests/pnp_ref.py.  Shared by tests/test_pnp_ref.py (CPU: the conditions the GPU comparisons
rest on hold for every run listed here) and tests/test_gpu_pnp_batch.py (GPU: the kernel reproduces them); every
reference run is made once per process.

A case is (n_points, seed), built like two_view_cases.make_case: camera 1 a few degrees of yaw and about a metre
from camera 0, the points 6-40 m ahead in camera 0's frame, camera 1's pixels with 0.5 px noise; from 63 points on, a
quarter of the pixels is moved by a gross error of 40 px.  A (case, options) pair enters RUNS only if
tests/test_pnp_ref.py's conditions hold for it; one that does not is replaced by another seed, never compared more
loosely.
"""
import functools

import numpy as np

import pnp_ref as PR
from oracle import ba_oracle as BO
from two_view_cases import CX, CY, FOCAL, _project, _yaw_w2c, quat_dist  # noqa: F401

LDS_POINTS = 1152  # pnp_batch.hip stages the points of a problem in LDS up to this many
OUTLIER_SHARE = 0.25
# the whole-solve comparisons run with min_points = 4, so that the 4- and 5-point problems run
OPTS = dict(PR.DEFAULTS, min_points=4)

# (points, seed): the exact fits 4 and 5, around one wavefront's 64 lanes, around one, and two, passes of the
# 256-thread stride, and around the LDS staging cap
SIZE_CASES = ((4, 1), (5, 27), (63, 3), (64, 4), (65, 5), (255, 13), (256, 7), (257, 8), (513, 9),
              (LDS_POINTS - 1, 10), (LDS_POINTS, 11), (LDS_POINTS + 1, 12))
# hypothesis counts: one, one per wavefront, a partial round of the wavefronts, the default, two chunks of 256
ITERATION_COUNTS = (1, 4, 5, 100, 257)
ITERATION_CASE = (65, 5)
# more workgroups than compute units: 30 distinct small problems, cycled to 300
MANY_CASES = tuple((9 + (7 * k) % 16, 200 + k) for k in range(30))


def opt_items(**kw):
    return tuple(sorted(kw.items()))


# every (case, options over OPTS) the GPU file compares against the reference
RUNS = tuple((c, ()) for c in SIZE_CASES) + \
    tuple((ITERATION_CASE, opt_items(iterations=h)) for h in ITERATION_COUNTS if h != 100) + \
    tuple((c, opt_items(refine_iters=0)) for c in SIZE_CASES[2:4])


def merged(items=()):
    o = dict(OPTS)
    o.update(dict(items))
    return o


@functools.lru_cache(maxsize=None)
def make_case(n, seed):
    """dict: points (n, 3), uv1 (n, 2), cam1_true (7,), outlier (n,) bool"""
    rng = np.random.default_rng(1000 + seed)
    z = rng.uniform(6.0, 40.0, n)
    pts = np.stack([z * rng.uniform(-0.55, 0.55, n), z * rng.uniform(-0.18, 0.18, n), z], axis=1)
    yaw = np.deg2rad(rng.uniform(2.0, 5.0)) * rng.choice([-1.0, 1.0])
    R1 = _yaw_w2c(yaw)
    t1 = -R1 @ np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.05, 0.05), rng.uniform(0.7, 1.2)])
    uv1 = _project(R1, t1, pts) + 0.5 * rng.standard_normal((n, 2))
    bad = (rng.random(n) < OUTLIER_SHARE) & (n >= 63)
    ang = rng.uniform(0.0, 2.0 * np.pi, n)
    uv1[bad] += 40.0 * np.stack([np.cos(ang), np.sin(ang)], axis=1)[bad]
    out = dict(points=pts, uv1=uv1, cam1_true=np.concatenate([BO.R_to_quat(R1), t1]), outlier=bad)
    for v in out.values():
        v.setflags(write=False)
    return out


def perturbed(case, rel, seed=999):
    """The case with every input number moved by a relative `rel`."""
    rng = np.random.default_rng(seed)
    out = dict(case)
    for k in ("points", "uv1"):
        out[k] = case[k] * (1.0 + rel * rng.uniform(-1.0, 1.0, case[k].shape))
    return out


def run_reference(case, opts, defect=None):
    return PR.solve(case["points"], case["uv1"], FOCAL, CX, CY, opts, defect)


@functools.lru_cache(maxsize=None)
def reference(n, seed, items=()):
    """pnp_ref.solve of case (n, seed) under OPTS + dict(items), computed once; do not modify the result."""
    return run_reference(make_case(n, seed), merged(items))


@functools.lru_cache(maxsize=None)
def conditioning(n, seed, items=()):
    """Per hypothesis of reference(n, seed, items): whether a relative 1e-12 perturbation of every input leaves its
    solution count and validity as they are and moves R and t by less than 1e-7 (bool array)."""
    ref = reference(n, seed, items)["hyp"]
    c = perturbed(make_case(n, seed), 1e-12)
    moved = PR.hypotheses(c["points"], c["uv1"], FOCAL, CX, CY, merged(items))
    well = (ref["valid"] == moved["valid"]) & (ref["n_solutions"] == moved["n_solutions"])
    well &= np.abs(ref["R"] - moved["R"]).reshape(len(well), -1).max(1) < 1e-7
    well &= np.abs(ref["t"] - moved["t"]).max(1) < 1e-7
    return well


def batch_arrays(cases):
    """The flat arrays sim3opt_pnp_batch_set_problems takes, for a list of (n, seed)."""
    cs = [make_case(*c) for c in cases]
    ptr = np.concatenate([[0], np.cumsum([c["points"].shape[0] for c in cs])]).astype(np.int32)
    return dict(point_ptr=ptr, points=np.concatenate([c["points"] for c in cs]),
                uv1=np.concatenate([c["uv1"] for c in cs]))


def rot_dist(qa, qb):
    """rotation angle [rad] between two unit quaternions"""
    d = abs(float(np.dot(qa, qb)))
    return 2.0 * np.arccos(min(1.0, d))


def flipped_pose(pose):
    """The camera turned half round about its y axis and moved 15 m ahead: some points in front, some behind."""
    R = np.diag([-1.0, 1.0, -1.0]) @ BO.quat_to_R(pose[:4])
    q = BO.R_to_quat(R)
    return np.concatenate([q / np.linalg.norm(q), np.diag([-1.0, 1.0, -1.0]) @ pose[4:] + [0.0, 0.0, 15.0]])


@functools.lru_cache(maxsize=None)
def score_poses(n, seed):
    """The poses the scoring operator is given for case (n, seed), (P, 7): the truth, every hypothesis of the
    reference (the identity where it has none) and a pose with points behind the camera."""
    c, hyp = make_case(n, seed), reference(n, seed)["hyp"]
    rows = [c["cam1_true"]] + [PR.pose_of(R, t) for R, t in zip(hyp["R"], hyp["t"])] + [flipped_pose(c["cam1_true"])]
    return np.stack(rows)


def reference_scores(case, poses, thr=OPTS["reproj_error"]):
    """(count (P,), cost (P,), e2 (P, n), z (P, n)) of pnp_ref's scoring of poses (P, 7)"""
    cnt, cost, E, Z = [], [], [], []
    for p in poses:
        R = BO.quat_to_R(p[:4])
        m, e2 = PR.inliers(R, p[4:], case["points"], case["uv1"], FOCAL, CX, CY, thr)
        cnt.append(int(m.sum())); cost.append(float(e2[m].sum())); E.append(e2)
        Z.append(PR.project_sqerr(R, p[4:], case["points"], case["uv1"], FOCAL, CX, CY)[1])
    return np.array(cnt), np.array(cost), np.stack(E), np.stack(Z)


# the refit operator's runs, (case, inliers kept, far start): the reference's best hypothesis on all its inliers, on
# the first six of them, and a start 0.8 rad and 5 m off, from which a trial is rejected
REFIT_RUNS = tuple((c, None, False) for c in SIZE_CASES[2:]) + ((SIZE_CASES[2], 6, False), ((257, 8), None, True))


def refit_input(case, keep, far):
    """(pose (7,), mask (n,) bool): the reference's best hypothesis of `case` and its inliers (the first `keep`)"""
    ref = reference(*case)
    hyp, b = ref["hyp"], ref["best"]
    mask = ref["mask_hypothesis"].copy()
    if keep is not None:
        mask[np.where(mask)[0][keep:]] = False
    pose = PR.pose_of(hyp["R"][b], hyp["t"][b])
    if far:
        dq = np.array([0.3 * np.sin(0.4), 0.9 * np.sin(0.4), 0.1 * np.sin(0.4), np.cos(0.4)])
        pose = PR.pose_of(BO.quat_to_R(dq / np.linalg.norm(dq)) @ BO.quat_to_R(pose[:4]), pose[4:] + [0.5, -0.3, 5.0])
    return pose, mask


@functools.lru_cache(maxsize=None)
def reference_refit(case, keep, far):
    pose, mask = refit_input(case, keep, far)
    c = make_case(*case)
    return PR.refit(pose, c["points"], c["uv1"], mask, FOCAL, CX, CY, OPTS)
