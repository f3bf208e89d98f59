"""Real inputs for the loop-candidate stages: the first 45 PTAM keyframes of KITTI 00 (tests/golden/kitti00/keyframes45,
20 510 tracked observations with point ids, world points and poses), read through lib.read_keyframe_bin and used exactly
as stored -- the pixels keep PTAM's pixel-centre offset of (-0.5, -0.5) px against the pinhole projection of their own
map points.  Shared by tests/test_real_keyframes_ref.py (CPU: the figures, the conditions of the comparisons, the
margins against PTAM's poses) and tests/test_gpu_real_keyframes.py (GPU: the kernels on these inputs); everything is
built once per process and marked read-only.

pair_problems()  keyframe pairs 1 and 2 apart that share at least 60 point ids (86 problems of 68-502 points), the ids
                 joined with np.intersect1d, so in ascending-id order
track_problem()  45 frames, the pairs 1, 2 and 3 apart (129) and their id joins (19 942 matches) for TrackBatch
match_frames()   the frames as MatchBatch takes them, with descriptors made from the point ids

A pair problem is registered with each stage's case module under a key of that module's shape (key(stage, k)), so that
reference(), conditioning() and the GPU files' check_whole_solve run on it unchanged: make_case of pnp_cases,
essential_cases, homography_cases and sim3_batch_cases is wrapped to answer those keys and hands every other key on.

LISTED[stage]: problems (keyframe pair) that fail a condition of the index and mask equalities, with the reason.  They
are left out of those equalities only, never of the comparison with PTAM's pose.  At most 4 of the 86 per stage.
"""
import functools
import os

import numpy as np

import essential_cases as EC
import homography_cases as HC
import pnp_cases as PC
import sim3_batch_cases as SC
import two_view_cases as TC
from oracle import ba_oracle as BO
from sim3opt_amd import lib as L

KF_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kitti00", "keyframes45")
FOCAL, CX, CY = L.KITTI_FOCAL, L.KITTI_CX, L.KITTI_CY
WIDTH, HEIGHT = 1241, 376
MIN_SHARED, PAIR_GAPS, TRACK_GAPS = 60, (1, 2), (1, 2, 3)
DEPTH_SCALE = 1.3  # frame 1's depths for the Sim(3) stage: its map 1.3 times frame 0's, as after monocular drift
TAG = "kitti00"
STAGES = ("pnp", "essential", "homography", "sim3")
# the options the restatements were run under ("Why this is next"): essential_ref at 100 hypotheses, the others at
# their defaults; as items over each case module's OPTS
ITEMS = dict(pnp=(), essential=(), homography=HC.opt_items(iterations=300), sim3=SC.opt_items(iterations=300))
OPTIONS = dict(pnp=dict(), essential=dict(iterations=100), homography=dict(), sim3=dict())  # ... and for the handles
# TwoViewBatch runs BAOptimize's configuration for six iterations: on these problems the refinement has converged by
# the eighth, after which the number of trials of an iteration is decided by rounding (a relative 1e-13 on the inputs
# changes it on a third of the problems), and test_gpu_two_view_batch.py's rule compares the trial counts exactly
TWO_VIEW_ITEMS = (("max_iters", 6),)
LISTED = dict(pnp={}, essential={}, homography={}, sim3={})
LISTED_MAX = 4


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def frames():
    """The 45 keyframes in file order, each with its points in its own camera's frame (points_c, depth)."""
    out = []
    for name in sorted(os.listdir(KF_DIR)):
        d = L.read_keyframe_bin(os.path.join(KF_DIR, name))
        d["Rw2c"] = np.array(d["Rw2c"]).reshape(3, 3)
        d["points_c"] = d["points_w"] @ d["Rw2c"].T + d["twinc"]
        d["depth"] = np.ascontiguousarray(d["points_c"][:, 2])
        d["point_ids"] = d["point_ids"].astype(np.int64)
        out.append(_frozen(d))
    return tuple(out)


def project(X):
    return np.stack([FOCAL * X[:, 0] / X[:, 2] + CX, FOCAL * X[:, 1] / X[:, 2] + CY], axis=1)


def _pair(a, b):
    fr = frames()
    f0, f1 = fr[a], fr[b]
    ids, i0, i1 = np.intersect1d(f0["point_ids"], f1["point_ids"], return_indices=True)
    R = f1["Rw2c"] @ f0["Rw2c"].T
    t = f1["twinc"] - R @ f0["twinc"]
    return _frozen(dict(pair=(a, b), ids=ids, idx0=i0, idx1=i1, uv0=f0["obs_uv"][i0].copy(), uv1=f1["obs_uv"][i1].copy(),
                        X0=f0["points_c"][i0].copy(), depth0=f0["depth"][i0].copy(), depth1=f1["depth"][i1].copy(),
                        R_true=R, t_true=t))


@functools.lru_cache(maxsize=None)
def pair_problems():
    """tuple of dicts: pair (a, b), ids, idx0, idx1 (rows of the two keyframes), uv0, uv1 (n, 2) as stored, X0 (n, 3) the
    points in camera 0's frame, depth0, depth1 (n,), R_true, t_true: PTAM's relative pose, X1 = R X0 + t"""
    n = len(frames())
    out = [_pair(a, a + g) for g in PAIR_GAPS for a in range(n - g)]
    return tuple(p for p in out if len(p["ids"]) >= MIN_SHARED)


def rotation_angle(R):
    return float(np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0)))


@functools.lru_cache(maxsize=None)
def six():
    """Indices into pair_problems() of the six problems of the read-out, defect and chain tests: the smallest, the
    largest, the two largest rotations, and two at gap 2 (the first and the last that are none of those)."""
    P = pair_problems()
    size = [len(p["ids"]) for p in P]
    pick = [int(np.argmin(size)), int(np.argmax(size))]
    for k in np.argsort([-rotation_angle(p["R_true"]) for p in P]):
        if len(pick) < 4 and int(k) not in pick:
            pick.append(int(k))
    gap2 = [k for k, p in enumerate(P) if p["pair"][1] - p["pair"][0] == 2 and k not in pick]
    return tuple(pick + [gap2[0], gap2[-1]])


# ---- the pair problems as cases of each stage's module ----------------------------------------------------------------
def key(stage, k):
    """Problem k of pair_problems() as a case of `stage`'s case module: (n, seed) for pnp and essential, (n, seed, kind)
    for homography and sim3, the keyframe pair in place of the seed."""
    p = pair_problems()[k]
    n = len(p["ids"])
    return (n, (TAG,) + p["pair"]) if stage in ("pnp", "essential", "two_view") else (n, p["pair"], TAG)


def _problem_of(case):
    pair = case[1][1:] if len(case) == 2 else case[1]
    return next(p for p in pair_problems() if p["pair"] == tuple(pair))


def _is_real(case):
    return (len(case) == 2 and isinstance(case[1], tuple) and case[1][:1] == (TAG,)) or (len(case) == 3 and case[2] == TAG)


def _quat(R):
    return BO.R_to_quat(R[None])[0]


def _pnp_case(p):
    return dict(points=p["X0"], uv1=p["uv1"], cam1_true=np.concatenate([_quat(p["R_true"]), p["t_true"]]),
                outlier=np.zeros(len(p["ids"]), dtype=bool))


def _two_view_case(p):
    s = float(np.linalg.norm(p["t_true"]))
    return dict(uv0=p["uv0"], uv1=p["uv1"], R_true=p["R_true"], t_true=p["t_true"] / s, scale=s,
                outlier=np.zeros(len(p["ids"]), dtype=bool), points=p["X0"])


def _sim3_case(p):
    q = _quat(p["R_true"])
    C = np.concatenate([q if q[3] >= 0 else -q, DEPTH_SCALE * p["t_true"], [DEPTH_SCALE]])
    n = len(p["ids"])
    return dict(uv0=p["uv0"], uv1=p["uv1"], depth0=p["depth0"], depth1=DEPTH_SCALE * p["depth1"], C_true=C,
                outlier=np.zeros(n, dtype=bool), front=np.ones(n, dtype=bool))


def _register(mod, build):
    if getattr(mod.make_case, "answers_real_cases", False):
        return
    synthetic = mod.make_case

    @functools.lru_cache(maxsize=None)
    def make_case(*case):
        return _frozen(build(_problem_of(case))) if _is_real(case) else synthetic(*case)

    make_case.answers_real_cases = True
    mod.make_case = make_case


def _refine_case(p):
    """TwoViewBatch's problem: camera 0 the identity, camera 1 the PnP restatement's pose, points and pixels as above"""
    k = next(i for i, q in enumerate(pair_problems()) if q["pair"] == p["pair"])
    return dict(cam0=np.array([0.0, 0, 0, 1, 0, 0, 0]), cam1=np.array(reference("pnp", k)["pose"]), points=p["X0"],
                uv0=p["uv0"], uv1=p["uv1"])


for _mod, _build in ((PC, _pnp_case), (EC, _two_view_case), (HC, _two_view_case), (SC, _sim3_case), (TC, _refine_case)):
    assert (_mod.FOCAL, _mod.CX, _mod.CY) == (FOCAL, CX, CY)
    _register(_mod, _build)
MODULE = dict(pnp=PC, essential=EC, homography=HC, sim3=SC, two_view=TC)


def case_of(stage, k):
    return MODULE[stage].make_case(*key(stage, k))


def reference(stage, k):
    """The restatement's run of problem k under ITEMS[stage], made once per process by the stage's own reference()."""
    c = key(stage, k)
    if stage == "two_view":  # (ba_oracle in BAOptimize's configuration, from the PnP restatement's pose)
        return TC.reference(*c, TWO_VIEW_ITEMS)
    return MODULE[stage].reference(*c, ITEMS[stage]) if stage in ("pnp", "essential") else MODULE[stage].reference(c, ITEMS[stage])


def batch_arrays(stage, which=None):
    """The flat arrays `stage`'s handle takes in set_problems, for the problems `which` (default: all 86, ragged)."""
    which = range(len(pair_problems())) if which is None else which
    return MODULE[stage].batch_arrays([key(stage, k) for k in which])


def two_view_subset():
    """The problems TwoViewBatch is run on: the six, and every fourth of the 86 (the oracle's runs are what takes time)"""
    return tuple(sorted(set(six()) | set(range(0, len(pair_problems()), 4))))


def listed(stage, k):
    return pair_problems()[k]["pair"] in LISTED[stage]


# ---- the poses against PTAM's ----------------------------------------------------------------------------------------
def angle(a, b):
    return float(np.arccos(np.clip(np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b)), -1.0, 1.0)))


def pose_deviation(R, t, p):
    """(rotation angle [rad], |t - t*| / |t*|, angle between the directions of t and t* [rad]) against PTAM's pose"""
    return (rotation_angle(R @ p["R_true"].T), float(np.linalg.norm(t - p["t_true"]) / np.linalg.norm(p["t_true"])),
            angle(t, p["t_true"]))


def pose7_deviation(pose, p):
    return pose_deviation(BO.quat_to_R(np.asarray(pose)[None, :4])[0], np.asarray(pose)[4:], p)


def sim3_deviation(C, p):
    """(rotation [rad], |t - 1.3 t*| / |1.3 t*|, |s / 1.3 - 1|) of a similarity against PTAM's pose and the planted scale"""
    rot, dt, _ = pose_deviation(BO.quat_to_R(np.asarray(C)[None, :4])[0], np.asarray(C)[4:7] / DEPTH_SCALE, p)
    return rot, dt, abs(float(C[7]) / DEPTH_SCALE - 1.0)


# ---- the track problem -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def track_problem():
    """dict: kp_ptr, kp (float32 obs_uv), pairs (129, 2), match_ptr, query_idx, train_idx, depth0, depth1 (the map
    point's depth in each camera), states (45, 8) = (quat(Rw2c), twinc, 1), ids (the point id of every keypoint) and
    match_ids (of every match), points_w (the world point of every keypoint)"""
    fr = frames()
    n = len(fr)
    kp_ptr = np.concatenate([[0], np.cumsum([len(f["point_ids"]) for f in fr])]).astype(np.int32)
    pairs = [(a, a + g) for g in TRACK_GAPS for a in range(n - g)]
    joins = [np.intersect1d(fr[a]["point_ids"], fr[b]["point_ids"], return_indices=True) for a, b in pairs]
    match_ptr = np.concatenate([[0], np.cumsum([len(j[0]) for j in joins])]).astype(np.int32)
    states = np.stack([np.concatenate([_quat(f["Rw2c"]), f["twinc"], [1.0]]) for f in fr])
    return _frozen(dict(
        kp_ptr=kp_ptr, kp=np.concatenate([f["obs_uv"] for f in fr]).astype(np.float32),
        pairs=np.array(pairs, dtype=np.int32), match_ptr=match_ptr,
        query_idx=np.concatenate([j[1] for j in joins]).astype(np.int32),
        train_idx=np.concatenate([j[2] for j in joins]).astype(np.int32),
        depth0=np.concatenate([fr[a]["depth"][j[1]] for (a, _), j in zip(pairs, joins)]),
        depth1=np.concatenate([fr[b]["depth"][j[2]] for (_, b), j in zip(pairs, joins)]),
        states=states, ids=np.concatenate([f["point_ids"] for f in fr]),
        match_ids=np.concatenate([j[0] for j in joins]), points_w=np.concatenate([f["points_w"] for f in fr])))


def track_arrays():
    """(frames, matches, cameras, camera keywords) as TrackBatch's set_frames, set_matches and set_cameras take them"""
    t = track_problem()
    mt = {k: t[k] for k in ("pairs", "match_ptr", "query_idx", "train_idx", "depth0", "depth1")}
    return (t["kp_ptr"], t["kp"]), mt, (t["states"],), dict(focal=FOCAL, cx=CX, cy=CY)


# ---- the frames for MatchBatch ---------------------------------------------------------------------------------------
INTRINSICS = dict(focal=FOCAL, cx=CX, cy=CY, image_width=WIDTH, image_height=HEIGHT)


def descriptor(point_id):
    d = np.random.default_rng(int(point_id)).standard_normal(64)
    return d / np.linalg.norm(d)


@functools.lru_cache(maxsize=None)
def match_frames():
    """tuple of dicts kp, desc, obs_uv, obs_depth (float32) and ids: every keypoint is a map-point observation of its
    frame; the descriptor the data lack is a unit-norm Gaussian 64-vector seeded by the point id, plus 1e-3 of noise
    per view."""
    cache, out = {}, []
    for v, f in enumerate(frames()):
        for i in f["point_ids"]:
            if int(i) not in cache:
                cache[int(i)] = descriptor(i)
        d = np.stack([cache[int(i)] for i in f["point_ids"]])
        d = d + 1e-3 * np.random.default_rng(10 ** 6 + v).standard_normal(d.shape)
        uv = f["obs_uv"].astype(np.float32)
        out.append(_frozen(dict(kp=uv, desc=d.astype(np.float32), obs_uv=uv.copy(), obs_depth=f["depth"].astype(np.float32),
                                ids=f["point_ids"])))
    return tuple(out)


def filtered_join(a, b, options=None):
    """(query_idx, train_idx) of the id join of frames a and b that passes MatchBatch's border and skew filters, restated
    on the float32 pixels (kittiDetector.h:1101-1106), ascending in the query index"""
    import match_ref as MR
    o = dict(MR.DEFAULTS, **(options or {}))
    fa, fb = match_frames()[a], match_frames()[b]
    _, i0, i1 = np.intersect1d(fa["ids"], fb["ids"], return_indices=True)
    p0, p1 = fa["kp"][i0].astype(np.float64), fb["kp"][i1].astype(np.float64)
    r = o["border_ratio"]
    keep = (np.abs(p1[:, 0] - p0[:, 0]) < o["skew_x"] * WIDTH) & (np.abs(p1[:, 1] - p0[:, 1]) < o["skew_y"] * HEIGHT)
    for p in (p0, p1):
        keep &= (p[:, 0] >= r * WIDTH) & (p[:, 0] <= (1 - r) * WIDTH) & (p[:, 1] >= r * HEIGHT) & (p[:, 1] <= (1 - r) * HEIGHT)
    order = np.argsort(i0[keep])
    return i0[keep][order].astype(np.int32), i1[keep][order].astype(np.int32)


@functools.lru_cache(maxsize=None)
def chain_arrays(which):
    """What MatchBatch hands on for the problems `which` (a tuple) with knn_k = 1 and the border and skew filters open,
    restated in numpy: point_ptr, points0, uv0, uv1, depth0, depth1 of the whole id joins in ascending query index, from
    the float32 pixels and depths of match_frames().  These are other problems than pair_problems(): the points are the
    pixels' back-projections at the map depth, not the map points."""
    import match_ref as MR
    parts = []
    for k in which:
        a, b = pair_problems()[k]["pair"]
        fa, fb = match_frames()[a], match_frames()[b]
        _, i0, i1 = np.intersect1d(fa["ids"], fb["ids"], return_indices=True)
        q, t = i0[np.argsort(i0)], i1[np.argsort(i0)]
        z0 = MR.knn_depth(fa["kp"][q], fa["obs_uv"], fa["obs_depth"], 1)[0].astype(np.float64)
        z1 = MR.knn_depth(fb["kp"][t], fb["obs_uv"], fb["obs_depth"], 1)[0].astype(np.float64)
        uv0, uv1 = fa["kp"][q].astype(np.float64), fb["kp"][t].astype(np.float64)
        pts = np.stack([z0 * ((uv0[:, 0] - CX) / FOCAL), z0 * ((uv0[:, 1] - CY) / FOCAL), z0], axis=1)
        parts.append(dict(points0=pts, uv0=uv0, uv1=uv1, depth0=z0, depth1=z1))
    out = {f: np.concatenate([p[f] for p in parts]) for f in parts[0]}
    out["point_ptr"] = np.concatenate([[0], np.cumsum([len(p["depth0"]) for p in parts])]).astype(np.int32)
    return _frozen(out)
