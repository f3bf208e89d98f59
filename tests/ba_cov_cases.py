"""Scenes of the bundle-adjustment covariance tests (tests/test_ba_cov_ref.py on the host,
tests/test_gpu_ba_covariances.py on the device), built with tests/ba_cases.py's helpers: identity-orientation cameras on
a line with a small sine offset, points 6 .. 25 m ahead, 0.5 px noise, the perturbed start of
_perturb(rot=0.002, trans=0.02, point=0.05); cameras 0 and 1 are fixed.

  cov_tracks ... 12 cameras 0.5 m apart, 60 points whose track lengths cycle 2, 3, 4, 8, 9, 12: k_ba_cov_points deals a
                 point's n^2 ordered observation pairs to the 64 lanes of a wavefront -- 8 observations are 64 pairs (one
                 pass), 9 are 81 (two), 12 are 144 (three).  Point 0 is seen by the fixed cameras 0 and 1 only, point 6
                 by the fixed camera 1 and the free camera 2.
  cov_small .... 6 cameras 1 m apart, 30 points, track lengths 2, 3, 6.
  lists, branches ... tests/ba_cases.py's (lists is singular at lambda = 0: a free camera nobody observes with, a point
                 seen once).

ACCURACY lists the (scene, lambda) pairs inside the comparison rule's condition (bound < 1e-3).
"""
import numpy as np

from oracle import ba_oracle as BO
import ba_cases as BC

TRACK_LENGTHS = (2, 3, 4, 8, 9, 12)
SMALL_LENGTHS = (2, 3, 6)
FIXED = (0, 1)
FIXED_ONLY_POINT, HALF_FIXED_POINT = 0, 6  # of cov_tracks
ACCURACY = (("cov_tracks", 0.0), ("cov_tracks", 1e-2), ("cov_tracks", 1.0), ("cov_small", 0.0), ("cov_small", 1.0),
            ("lists", 1.0), ("branches", 1e-2), ("branches", 1.0))


def _tracks(nc, npt, lengths, spacing, seed):
    rng = np.random.default_rng(seed)
    k = np.arange(nc)
    centre = np.stack([spacing * k, 0.05 * np.sin(k), 0.03 * np.sin(1.7 * k)], axis=1)
    cams = BC._cams_of(np.tile(np.eye(3), (nc, 1, 1)), centre)
    oc, op = [], []
    for p in range(npt):
        n = lengths[p % len(lengths)]
        first = (p // len(lengths)) % (nc - n + 1)
        oc += list(range(first, first + n))
        op += [p] * n
    oc, op = np.array(oc), np.array(op)
    span = spacing * (nc - 1)
    pts = np.stack([rng.uniform(-4, span + 4, npt), rng.uniform(-2.5, 2.5, npt), rng.uniform(6, 25, npt)], axis=1)
    uv, depth = BC._project(cams, pts, oc, op)
    assert (depth > 4).all()
    uv = uv + rng.standard_normal(uv.shape) * 0.5
    c0, p0 = BC._perturb(rng, cams, pts, rot=0.002, trans=0.02, point=0.05)
    P = BO.Problem(c0, p0, oc, op, uv)
    P.fixed[list(FIXED)] = True
    return P


_cache = {}


def problem(name):
    """The scene's problem (an oracle Problem; built once, do not modify)."""
    if name in ("lists", "branches"):
        return BC.problem(name)
    if name not in _cache:
        if name == "cov_tracks":
            _cache[name] = _tracks(12, 60, TRACK_LENGTHS, 0.5, 707)
        elif name == "cov_small":
            _cache[name] = _tracks(6, 30, SMALL_LENGTHS, 1.0, 808)
        else:
            raise KeyError(name)
    return _cache[name]


def check_tracks(P):
    """The conditions cov_tracks exists for."""
    n = np.bincount(P.op)
    assert sorted(set(n.tolist())) == sorted(TRACK_LENGTHS)
    fixed = np.asarray(P.fixed, dtype=bool)
    assert fixed[P.oc[P.op == FIXED_ONLY_POINT]].all() and (P.op == FIXED_ONLY_POINT).sum() == 2
    half = fixed[P.oc[P.op == HALF_FIXED_POINT]]
    assert half.sum() == 1 and half.size == 2


def requests(P):
    """Everything the accuracy test asks for: the camera pairs that share a point (every camera with itself, both
    orders of the others), all points, all observed (point, camera) pairs."""
    nc = P.cams.shape[0]
    share = np.zeros((nc, nc), dtype=bool)
    share[np.arange(nc), np.arange(nc)] = True
    for p in range(P.points.shape[0]):
        c = P.oc[P.op == p]
        share[np.ix_(c, c)] = True
    a, b = np.nonzero(share)
    cam_pairs = np.stack([a, b], axis=1).astype(np.int32)
    points = np.arange(P.points.shape[0], dtype=np.int32)
    pc = np.unique(np.stack([P.op, P.oc], axis=1), axis=0).astype(np.int32)
    return cam_pairs, points, pc
