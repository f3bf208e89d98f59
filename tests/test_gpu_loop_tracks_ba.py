"""End to end: the loop tracks hold a loop shut in the bundle adjustment.

A planted scene of two passes along one stretch: 12 cameras (6 a pass), 80 world points.  Each pass has its own copy of
the map points, as a map built by tracking has; the second pass's cameras and points carry a planted rigid drift, so the
map alone is consistent to the pixel and nothing in its cost knows of the drift.  Pixels are noise-free (rounded to the
float32 the keypoints are held in).  Matches join the passes: camera i of the first pass with cameras i and i + 1 of the
second, so a world point's observations in all twelve cameras become one track.

With the first pass's cameras fixed, bundle adjustment on the map alone leaves the second pass's camera centres at the
planted drift; with TrackBatch.ba_rows appended it brings them back.

Thresholds, chosen from oracle/ba_oracle.py alone (the CPU test below measures them again):
    map alone, ITERS = 15 iterations:  share of the drift left 1.000001 (oracle) -> required >= 0.99
    with the loop tracks, ITERS:       share of the drift left 4.1e-07 (oracle)  -> required <= 1e-3
The oracle has far more than a factor 10 to spare on both (it left 1.1e-03 after 10 iterations and 3.5e-05 after 12:
the iteration count matters; 4e-07 is where the float32 pixels stop it).  The device is held to the same thresholds and
measured 1.000001 and 4.13e-07."""
import numpy as np
import pytest

from oracle import ba_oracle as BO
from sim3opt_amd import lib as L
import track_ref as TR

ITERS = 15
SHARE_WITHOUT, SHARE_WITH = 0.99, 1e-3
F, CX, CY = 718.856, 607.1928, 185.2157
N_PASS, N_POINTS = 6, 80


def yaw_R(a):
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])


def scene():
    rng = np.random.default_rng(17)
    pts = np.stack([rng.uniform(-6, 6, N_POINTS), rng.uniform(-2, 2, N_POINTS), rng.uniform(20, 40, N_POINTS)], axis=1)
    true = np.zeros((2 * N_PASS, 7))
    for c in range(2 * N_PASS):
        i, second = c % N_PASS, c // N_PASS
        Rw2c = yaw_R(0.015 * i + 0.01 * second).T
        centre = np.array([0.2 * second + 0.1 * np.sin(i), 0.05 * second, 1.0 * i + 0.4 * second])
        true[c, :4], true[c, 4:] = BO.R_to_quat(Rw2c[None])[0], -Rw2c @ centre
    # the planted drift of the second pass: X' = D X + d for its points, and the cameras that see them alike
    D, d = yaw_R(0.03), np.array([0.9, -0.15, 0.6])
    cams = true.copy()
    for c in range(N_PASS, 2 * N_PASS):
        R = BO.quat_to_R(true[c, :4]) @ D.T
        cams[c, :4], cams[c, 4:] = BO.R_to_quat(R[None])[0], true[c, 4:] - R @ d
    points = np.concatenate([pts, pts @ D.T + d])  # the two copies: the second drifted
    X = np.einsum("cij,pj->cpi", BO.quat_to_R(true[:, :4]), pts) + true[:, None, 4:]
    uv = np.stack([F * X[..., 0] / X[..., 2] + CX, F * X[..., 1] / X[..., 2] + CY], axis=-1).astype(np.float32)
    assert (X[..., 2] > 4).all() and (uv[..., 0] > 0).all() and (uv[..., 0] < 1241).all()
    # every camera sees every point: keypoint p of camera c is point p (in a per-camera shuffle, so indices differ)
    perm = np.stack([rng.permutation(N_POINTS) for _ in range(2 * N_PASS)])  # perm[c, k]: the point of keypoint k
    inv = np.argsort(perm, axis=1)
    kp = np.concatenate([uv[c, perm[c]] for c in range(2 * N_PASS)])
    depth = np.stack([X[c, perm[c], 2] for c in range(2 * N_PASS)])
    oc = np.repeat(np.arange(2 * N_PASS), N_POINTS)
    op = np.concatenate([perm[c] + N_POINTS * (c // N_PASS) for c in range(2 * N_PASS)])
    pairs = [(i, N_PASS + j) for i in range(N_PASS) for j in (i, i + 1) if j < N_PASS]
    q = np.concatenate([inv[a] for a, _ in pairs])  # point p = 0 .. in both frames
    t = np.concatenate([inv[b] for _, b in pairs])
    return dict(true=true, cams=cams, points=points, obs_cam=oc.astype(np.int32), obs_point=op.astype(np.int32),
                obs_uv=kp.astype(np.float64), kp_ptr=np.arange(2 * N_PASS + 1, dtype=np.int32) * N_POINTS, kp=kp,
                pairs=np.array(pairs, dtype=np.int32), match_ptr=np.arange(len(pairs) + 1, dtype=np.int32) * N_POINTS,
                query_idx=q.astype(np.int32), train_idx=t.astype(np.int32),
                depth0=np.concatenate([depth[a, inv[a]] for a, _ in pairs]),
                depth1=np.concatenate([depth[b, inv[b]] for _, b in pairs]),
                states=np.concatenate([cams, np.ones((2 * N_PASS, 1))], axis=1),
                fixed=np.arange(2 * N_PASS) < N_PASS)


def centres(cams):
    return -np.einsum("cji,cj->ci", BO.quat_to_R(cams[:, :4]), cams[:, 4:])


def share_left(s, cams):
    """The largest distance of a second-pass camera centre from where it truly is, as a share of the planted one"""
    err = np.linalg.norm(centres(cams) - centres(s["true"]), axis=1)[N_PASS:]
    planted = np.linalg.norm(centres(s["cams"]) - centres(s["true"]), axis=1)[N_PASS:]
    assert planted.min() > 0.5
    return float(err.max() / planted.max())


def with_rows(s, rows):
    return (s["cams"], np.concatenate([s["points"], rows["points"]]), np.concatenate([s["obs_cam"], rows["obs_cam"]]),
            np.concatenate([s["obs_point"], rows["obs_point"]]), np.concatenate([s["obs_uv"], rows["obs_uv"]]))


def track_kwargs(s):
    return {k: s[k] for k in ("pairs", "match_ptr", "query_idx", "train_idx", "depth0", "depth1")}


def check_rows(s, rows):
    assert rows["points"].shape == (N_POINTS, 3) and len(rows["obs_cam"]) == 2 * N_PASS * N_POINTS
    assert rows["obs_point"].min() == 2 * N_POINTS and rows["obs_point"].max() == 3 * N_POINTS - 1
    # a track's point lies between the two copies of its world point
    mid = 0.5 * (s["points"][:N_POINTS] + s["points"][N_POINTS:])
    assert np.abs(np.sort(rows["points"], axis=0) - np.sort(mid, axis=0)).max() < 1e-3


def test_the_oracle_meets_the_thresholds_with_a_factor_ten_to_spare():
    """oracle/ba_oracle.py alone on the CPU, the rows from the host restatement"""
    s = scene()
    tr = L.TrackBatch.reference(s["kp_ptr"], s["kp"], states=s["states"], focal=F, cx=CX, cy=CY, **track_kwargs(s))
    assert (tr["status"] == TR.OK).all() and np.diff(tr["track_ptr"]).tolist() == [2 * N_PASS] * N_POINTS
    rows = TR.ba_rows(tr, s["kp_ptr"], s["kp"], point_base=2 * N_POINTS)
    check_rows(s, rows)
    shares = []
    for args in ((s["cams"], s["points"], s["obs_cam"], s["obs_point"], s["obs_uv"]), with_rows(s, rows)):
        P = BO.Problem(*args, focal=F, cx=CX, cy=CY)
        P.fixed = s["fixed"].copy()
        P.optimize(ITERS)
        shares.append(share_left(s, P.cams))
    print(f"oracle: share of the drift left after {ITERS} iterations: map alone {shares[0]:.6f}, with the loop tracks "
          f"{shares[1]:.3g}")
    assert shares[0] >= 1 - (1 - SHARE_WITHOUT) / 10 and shares[1] <= SHARE_WITH / 10


@pytest.mark.gpu
def test_loop_tracks_close_the_loop_in_the_bundle_adjustment():
    s = scene()
    T = L.TrackBatch(device=0)
    T.set_frames(s["kp_ptr"], s["kp"])
    T.set_matches(**track_kwargs(s))
    T.set_cameras(s["states"], focal=F, cx=CX, cy=CY)
    assert T.solve() == N_POINTS
    rows = T.ba_rows(point_base=2 * N_POINTS)
    T.close()
    check_rows(s, rows)
    shares = []
    for args in ((s["cams"], s["points"], s["obs_cam"], s["obs_point"], s["obs_uv"]), with_rows(s, rows)):
        B = L.BundleAdjuster(device=0)
        B.set_problem(*args, focal=F, cx=CX, cy=CY)
        B.set_fixed_cameras(s["fixed"])
        B.optimize(ITERS)
        shares.append(share_left(s, B.cameras()))
        B.close()
    print(f"device: share of the drift left after {ITERS} iterations: map alone {shares[0]:.6f}, with the loop tracks "
          f"{shares[1]:.3g}")
    assert shares[0] >= SHARE_WITHOUT and shares[1] <= SHARE_WITH
