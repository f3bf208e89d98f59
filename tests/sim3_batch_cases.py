"""Scenes with a planted Sim(3) for the batched Sim(3) stage (sim3opt_sim3_batch) and their reference runs through
tests/sim3_batch_ref.py.  Shared by tests/test_sim3_batch_ref.py (CPU: the conditions the GPU comparisons rest on hold
for every run listed here) and tests/test_gpu_sim3_batch.py (GPU: the kernel reproduces them); every reference run is
made once per process.

A case is (n_matches, seed, kind): a cloud of points 10-20 map units ahead of camera 0, camera 1 related to it by the
planted C* = (R, t, s) with X1 = s R X0 + t -- s cycles through 0.5, 1, 2.3 with the seed, the rotation is a few
degrees for even seeds and about 2 rad for odd ones, t puts the cloud in front of camera 1 -- and the matches are the
pixels and depths of the points in both frames.  Kinds:
  "exact"      noise-free pixels (the property tests)
  "noisy"      0.3 px noise in both images; from 63 matches on a quarter of camera 1's pixels is moved by 40 px
  "dup"        "noisy" with every fourth match repeated once (the next row is a copy)
  "line"       every point on one line: no sample is a triangle (status 2)
  "behind"     "exact", but 40 % of the points lie behind camera 1 under C*: their pixel is the one the line through
               the centre meets and their depth is |z|, so only the sign of the depth tells them from inliers
A (case, options) pair enters RUNS only if tests/test_sim3_batch_ref.py's conditions hold for it; one that does not is
replaced by another seed, never compared more loosely.
"""
import functools

import numpy as np

import sim3_batch_ref as SR
from sim3opt_amd import sim3np

FOCAL, CX, CY = 718.856, 607.1928, 185.2157
LDS_POINTS = 1072  # sim3_batch.hip stages the matches of a problem in LDS up to this many
CHUNK = 128        # ... and makes, then scores, this many hypotheses at a time
NOISE_PX, OUTLIER_SHARE = 0.3, 0.25
SCALES = (0.5, 1.0, 2.3)
OPTS = dict(SR.DEFAULTS, iterations=64)  # the comparisons run 64 hypotheses unless a run says otherwise

SIZE_CASES = ((9, 1, "exact"), (10, 2, "exact"), (63, 1, "noisy"), (64, 2, "noisy"), (65, 3, "noisy"),
              (255, 1, "noisy"), (256, 2, "exact"), (257, 3, "noisy"), (LDS_POINTS - 1, 1, "noisy"),
              (LDS_POINTS, 2, "noisy"), (LDS_POINTS + 1, 3, "noisy"), (66, 2, "dup"), (80, 9, "behind"))
SMALL_CASES = ((3, 1, "exact"), (8, 2, "exact"))  # fewer than min_points: status 1
LINE_CASE = (12, 1, "line")
NOISY_CASES = tuple(c for c in SIZE_CASES if c[2] in ("noisy", "dup"))
ITERATION_COUNTS = (1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1, 300)
ITERATION_CASE = {1: (65, 2, "exact"), 300: (257, 3, "noisy")}


def opt_items(**kw):
    return tuple(sorted(kw.items()))


# every (case, options over OPTS) the GPU file compares against the reference
RUNS = tuple((c, ()) for c in SIZE_CASES) + \
    tuple((ITERATION_CASE.get(h, (65, 3, "noisy")), opt_items(iterations=h)) for h in ITERATION_COUNTS) + \
    (((65, 3, "noisy"), opt_items(seed=4242)), ((255, 1, "noisy"), opt_items(max_pixel_error=2.0)),
     ((257, 3, "noisy"), opt_items(huber_delta=0.4)), ((65, 3, "noisy"), opt_items(huber_delta=0.0)),
     ((64, 2, "noisy"), opt_items(pixel_noise=2.0)), ((10, 2, "exact"), opt_items(min_inliers=11)),
     ((66, 2, "dup"), opt_items(iterations=3)))  # (a weak best hypothesis: the refinement changes the inlier set)
# the batch that mixes all of them (options OPTS)
MIXED = SMALL_CASES + SIZE_CASES + (LINE_CASE,)


def merged(items=()):
    o = dict(OPTS)
    o.update(dict(items))
    return o


def rot_vec(w):
    return sim3np.quat_to_R(sim3np.exp(np.concatenate([w, np.zeros(4)]), fix_b=1)[:4])


def project(X):
    return np.stack([FOCAL * X[:, 0] / X[:, 2] + CX, FOCAL * X[:, 1] / X[:, 2] + CY], axis=1)


@functools.lru_cache(maxsize=None)
def make_case(n, seed, kind):
    """dict: uv0, uv1 (n, 2), depth0, depth1 (n,), C_true (8,), outlier (n,) bool, front (n,) bool"""
    rng = np.random.default_rng(7000 + 13 * seed + n)
    s = SCALES[seed % 3]
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    R = rot_vec(axis * (rng.uniform(1.8, 2.2) if seed % 2 else np.deg2rad(rng.uniform(2.0, 6.0))))
    c0 = np.array([0.0, 0.0, 15.0])
    X0 = c0 + rng.uniform(-1.0, 1.0, (n, 3)) * [5.0, 2.0, 5.0]
    if kind == "line":
        X0 = c0 + np.outer(np.linspace(-1.0, 1.0, n), [4.0, 1.0, 3.0])
    t = np.array([rng.uniform(-1.0, 1.0), rng.uniform(-0.3, 0.3), 15.0 * s]) - s * R @ c0
    X1 = s * X0 @ R.T + t
    if kind == "behind":  # 40 % of the points mirrored through camera 1's image plane; camera 0 still sees them
        X1[:int(0.4 * n), 2] *= -1.0
        X0 = (X1 - t) @ R / s
        assert (X0[:, 2] > 1.0).all(), "this seed puts a mirrored point behind camera 0: take another"
    front = X1[:, 2] > 0
    uv0, uv1 = project(X0), project(X1)
    depth0, depth1 = X0[:, 2].copy(), np.abs(X1[:, 2])
    bad = np.zeros(n, dtype=bool)
    if kind in ("noisy", "dup"):
        uv0 = uv0 + NOISE_PX * rng.standard_normal((n, 2))
        uv1 = uv1 + NOISE_PX * rng.standard_normal((n, 2))
        bad = (rng.random(n) < OUTLIER_SHARE) & (n >= 63)
        ang = rng.uniform(0.0, 2.0 * np.pi, n)
        uv1[bad] += 40.0 * np.stack([np.cos(ang), np.sin(ang)], axis=1)[bad]
    if kind == "dup":
        for k in range(0, n - 1, 4):
            uv0[k + 1], uv1[k + 1], depth0[k + 1], depth1[k + 1], bad[k + 1] = uv0[k], uv1[k], depth0[k], depth1[k], bad[k]
    q = sim3np.R_to_quat(R)
    out = dict(uv0=uv0, uv1=uv1, depth0=depth0, depth1=depth1,
               C_true=np.concatenate([q if q[3] >= 0 else -q, t, [s]]), outlier=bad, front=front)
    for v in out.values():
        v.setflags(write=False)
    return out


def run_reference(case, opts, defect=None):
    return SR.solve(case["uv0"], case["uv1"], case["depth0"], case["depth1"], FOCAL, CX, CY, opts, defect)


@functools.lru_cache(maxsize=None)
def reference(case, items=()):
    """sim3_batch_ref.solve of `case` under OPTS + dict(items), computed once; do not modify the result."""
    return run_reference(make_case(*case), merged(items))


def data_of(case):
    c = make_case(*case)
    return SR.data(c["uv0"], c["uv1"], c["depth0"], c["depth1"], FOCAL, CX, CY)


def batch_arrays(cases):
    """The flat arrays sim3opt_sim3_batch_set_problems takes, for a list of cases."""
    cs = [make_case(*c) for c in cases]
    out = dict(point_ptr=np.concatenate([[0], np.cumsum([len(c["uv0"]) for c in cs])]).astype(np.int32))
    for k in ("uv0", "uv1", "depth0", "depth1"):
        out[k] = np.concatenate([c[k] for c in cs])
    return out


def sim3_distance(Ca, Cb):
    """(rotation angle [rad], |ta - tb|, |log(sa / sb)|) between two similarities"""
    Ra, Rb = sim3np.quat_to_R(np.asarray(Ca[:4]) / np.linalg.norm(Ca[:4])), sim3np.quat_to_R(
        np.asarray(Cb[:4]) / np.linalg.norm(Cb[:4]))
    ang = float(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1.0) / 2.0, -1.0, 1.0)))
    return ang, float(np.linalg.norm(np.asarray(Ca[4:7]) - Cb[4:7])), abs(float(np.log(Ca[7] / Cb[7])))


def sim3_deviation(Ca, Cb):
    """one number for two similarities that should agree: max |Ca - Cb| over the entries, q up to sign, t relative
    to 1 + |t|"""
    a, b = np.asarray(Ca, dtype=np.float64), np.asarray(Cb, dtype=np.float64)
    dq = min(np.abs(a[..., :4] - b[..., :4]).max(), np.abs(a[..., :4] + b[..., :4]).max())
    dt = np.abs(a[..., 4:7] - b[..., 4:7]).max() / (1.0 + np.abs(b[..., 4:7]).max())
    return float(max(dq, dt, abs(a[..., 7] - b[..., 7]) / b[..., 7]))


def truth_errors(C, c):
    """(rotation [rad], |t - t*| / |t*|, |log s / s*|) against the planted C*"""
    ang, dt, ds = sim3_distance(C, c["C_true"])
    return ang, dt / float(np.linalg.norm(c["C_true"][4:7])), ds
