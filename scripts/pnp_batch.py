"""Times the batched PnP RANSAC (sim3opt_pnp_batch: the start pose of every loop candidate in one launch) alone and
followed by the batched two-view refinement from its poses (sim3opt_ba_batch), and writes profiles/pnp_batch.json.

    python scripts/pnp_batch.py [--runs 11] [--out profiles/pnp_batch.json] [--numpy-reference]

The 118 problems take their point counts and the poses they are planted with from the 118 records of
tests/golden/kitti00/loopConstraints.txt (scripts/two_view_batch.py reads them).  The detector's own inputs are not
stored with the reference, so points and pixels are synthetic: seeded, 0.5 px noise, a quarter of camera 1's pixels
moved by a gross error of 40 px; the generator's parameters are recorded in the JSON.

Timing: host wall clock around calls that return after the device synchronise, warm, median over the runs; every run
re-submits its problems.  No speed-up is claimed: there is no earlier number for this step (OpenCV is not a
dependency of this project), and about 118 x 100 x 600 projections are microseconds of arithmetic -- the launch is
latency-bound.  What the PnP time is to be read against is the two-view refinement's time in the same run.
--numpy-reference also times tests/pnp_ref.py on the same problems, as context only: it is a test reference, not a
competitor.  For the kernel time, run this script once under `rocprofv3 --kernel-trace --stats` and put the
k_pnp_ransac row into the JSON's "kernel_trace" entry (scripts/README.md).  Needs a GPU; there is no fallback.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
os.environ.setdefault("SIM3OPT_PRELOAD_TORCH", "1")

from sim3opt_amd import lib as L  # noqa: E402
import two_view_batch as TV  # noqa: E402

GEN = dict(seed=20240612, depth_in_baselines=[6.0, 40.0], x_over_z=0.55, y_over_z=0.18, noise_px=0.5,
           outlier_fraction=0.25, outlier_px=40.0)
PNP_OPTS = dict(iterations=100, reproj_error=3.0, min_inliers=10, min_points=9, refine_iters=10, max_trials=5, tau=1e-5,
                seed=0)


def make_problems(records, gen=GEN):
    """dict of the PnP arrays (point_ptr, points, uv1), camera 0's pixels uv0 and the planted cam1_true (n, 7)"""
    rng = np.random.default_rng(gen["seed"])
    f, cx, cy = L.KITTI_FOCAL, L.KITTI_CX, L.KITTI_CY

    def proj(R, t, p):
        X = p @ R.T + t
        return np.stack([f * X[:, 0] / X[:, 2] + cx, f * X[:, 1] / X[:, 2] + cy], axis=1)

    ptr, pts, uv0, uv1, truth = [0], [], [], [], []
    for n, pose in records:
        base = float(np.linalg.norm(pose[4:]))
        z = base * rng.uniform(*gen["depth_in_baselines"], n)
        p = np.stack([z * rng.uniform(-gen["x_over_z"], gen["x_over_z"], n),
                      z * rng.uniform(-gen["y_over_z"], gen["y_over_z"], n), z], axis=1)
        a = proj(np.eye(3), np.zeros(3), p) + gen["noise_px"] * rng.standard_normal((n, 2))
        b = proj(TV.quat_to_R(pose[:4]), pose[4:], p) + gen["noise_px"] * rng.standard_normal((n, 2))
        bad, ang = rng.random(n) < gen["outlier_fraction"], rng.uniform(0.0, 2.0 * np.pi, n)
        b[bad] += gen["outlier_px"] * np.stack([np.cos(ang), np.sin(ang)], axis=1)[bad]
        ptr.append(ptr[-1] + n)
        pts.append(p); uv0.append(a); uv1.append(b); truth.append(pose)
    return dict(point_ptr=np.array(ptr, dtype=np.int32), points=np.concatenate(pts), uv0=np.concatenate(uv0),
                uv1=np.concatenate(uv1), cam1_true=np.stack(truth))


def run_pnp(pnp, P):
    pnp.set_problems(P["point_ptr"], P["points"], P["uv1"])
    return pnp.solve()


def run_both(pnp, ba, P, cam0):
    ok = run_pnp(pnp, P)
    ba.set_problems(point_ptr=P["point_ptr"], cam0=cam0, cam1=pnp.poses(), points=P["points"], uv0=P["uv0"],
                    uv1=P["uv1"])
    ba.optimize()
    return ok


def ms(t):
    return dict(median=1e3 * float(np.median(t)), min=1e3 * min(t), max=1e3 * max(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pnp_batch.json"))
    ap.add_argument("--numpy-reference", action="store_true", help="also time tests/pnp_ref.py (context only)")
    args = ap.parse_args()
    if args.runs < 5:
        ap.error("--runs: at least 5")
    records = TV.read_records()
    P = make_problems(records)
    counts = np.diff(P["point_ptr"])
    n = len(records)
    cam0 = np.tile([0.0, 0, 0, 1, 0, 0, 0], (n, 1))
    res = dict(problems=n, points_min=int(counts.min()), points_max=int(counts.max()), points_total=int(counts.sum()),
               generator=GEN, pnp_options=PNP_OPTS, two_view_options=TV.OPTS, runs=args.runs, warmup=args.warmup,
               timing="host wall clock around calls that return after the device synchronise; warm; median of runs; the "
                      "three measurements alternate; every run re-submits its problems",
               claim="none: there is no earlier number for this step and OpenCV is not on these machines; the launch "
                     "is latency-bound; read pnp_ms against two_view_ms of the same run")
    pnp, ba = L.PnpBatch(**PNP_OPTS), L.TwoViewBatch(**TV.OPTS)
    for _ in range(args.warmup):
        run_both(pnp, ba, P, cam0)
    tp, tb, tt = [], [], []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        run_pnp(pnp, P)
        tp.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        run_both(pnp, ba, P, cam0)
        tb.append(time.perf_counter() - t0)
        poses = pnp.poses()
        t0 = time.perf_counter()
        ba.set_problems(point_ptr=P["point_ptr"], cam0=cam0, cam1=poses, points=P["points"], uv0=P["uv0"], uv1=P["uv1"])
        ba.optimize()
        tt.append(time.perf_counter() - t0)
    res["pnp_ms"], res["pnp_then_two_view_ms"], res["two_view_ms"] = ms(tp), ms(tb), ms(tt)
    # what came out: statuses, inliers, and the distance of the poses from the planted ones (before / after the BA)
    s, (mask, cnt) = pnp.summary(), pnp.inliers()
    poses, refined = pnp.poses(), ba.cameras()[1]

    def off(c):
        dot = np.abs((c[:, :4] * P["cam1_true"][:, :4]).sum(1)).clip(max=1.0)
        base = np.linalg.norm(P["cam1_true"][:, 4:], axis=1)
        return dict(rotation_rad_max=float((2 * np.arccos(dot)).max()),
                    translation_over_baseline_max=float((np.abs(c[:, 4:] - P["cam1_true"][:, 4:]).max(1) / base).max()))

    res["result"] = dict(status_counts=[int((s["status"] == k).sum()) for k in range(4)],
                         inlier_share_min=float((cnt / counts).min()), inlier_share_max=float((cnt / counts).max()),
                         rms_px_max=float(s["rms_px"].max()),
                         refine_iterations_max=int(s["refine_iterations"].max()),
                         pnp_vs_truth=off(poses), two_view_vs_truth=off(refined))
    if args.numpy_reference:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import pnp_ref as PR
        t0 = time.perf_counter()
        for k in range(n):
            lo, hi = int(P["point_ptr"][k]), int(P["point_ptr"][k + 1])
            PR.solve(P["points"][lo:hi], P["uv1"][lo:hi], L.KITTI_FOCAL, L.KITTI_CX, L.KITTI_CY, PNP_OPTS)
        res["numpy_reference_ms"] = dict(once=1e3 * (time.perf_counter() - t0),
                                         note="tests/pnp_ref.py, one problem after the other: context only")
    res["kernel_trace"] = "not collected in this run (rocprofv3 --kernel-trace --stats, see the docstring)"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: res[k] for k in ("problems", "points_total", "pnp_ms", "pnp_then_two_view_ms", "two_view_ms",
                                          "result") if k in res}))


if __name__ == "__main__":
    main()
