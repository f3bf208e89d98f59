"""Times the batched homography stage (sim3opt_homography_batch: MLESAC, refinement, decomposition and choice of every
loop candidate in one launch) and writes profiles/homography_batch.json.

    python scripts/homography_batch.py [--runs 11] [--out profiles/homography_batch.json]

The 118 problems take their point counts and the poses they are planted with from the 118 records of
tests/golden/kitti00/loopConstraints.txt (scripts/two_view_batch.py reads them).  The detector's matched pixels are not
stored with the reference, so they are synthetic and planar: per problem a seeded plane 6-40 baselines ahead of camera
0, 0.3 px noise on both views, a quarter of camera 1's pixels moved by a gross error of 40 px; the generator's
parameters are recorded in the JSON.

Timing: host wall clock around calls that return after the device synchronise, warm, median over the runs; every run
re-submits its problems.  Nothing is known about this kernel's time: no target is set and NO SPEED-UP IS CLAIMED (TooN
and libCVD are absent, so the reference cannot be built here, and there is no earlier number for this step).  The same
run also times the other stages, each on the problems of its own script (scripts/essential_batch.py, pnp_batch.py,
two_view_batch.py, match_batch.py), next to the medians their profiles hold: evidence that they were left alone.

The pose errors against the planted truth: a plane alone leaves two Faugeras-Lustman solutions that explain the pixels
equally, and the reference's Sampson tie-break between them is decided by the noise, so the chosen pose is the planted
one in about half the problems; the JSON gives the worst errors over all problems, the number in which the chosen
pose is the planted one (direction of t within 0.2 rad) and the worst errors among those.

Every step is a process of its own under its own time limit, and the script stops at the first one that fails.  For
the kernel time, run `--step homography` once under `rocprofv3 --kernel-trace --stats --output-format csv` (a run of
its own, no other tracing), store its kernel_stats.csv as profiles/homography_batch_kernel_stats.csv and pass it to the
timing run with --kernel-stats: the JSON then holds the k_homography_ransac row.  Needs a GPU; there is no fallback.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
os.environ.setdefault("SIM3OPT_PRELOAD_TORCH", "1")

import essential_batch as EB  # noqa: E402  (the other stages' steps and the timing helpers)

GEN = dict(seed=20240613, plane_depth_in_baselines=[12.0, 16.0], plane_slope_x=[0.5, 1.0], plane_slope_y=[-0.3, 0.3],
           x_over_z=0.55, y_over_z=0.18, noise_px=0.3, outlier_fraction=0.25, outlier_px=40.0)
HOM_OPTS = dict(max_pixel_error=5.0, iterations=300, refine_rounds=5, min_points=10, seed=0)
STEPS = (("homography", 240), ("essential", 240), ("pnp", 120), ("two_view", 120), ("match", 240))


def make_problems(records, gen=GEN):
    """dict of point_ptr, uv0, uv1 and the planted cam1_true (n, 7): every problem's points on a plane of its own"""
    from sim3opt_amd import lib as L
    import two_view_batch as TV
    rng = np.random.default_rng(gen["seed"])
    f, cx, cy = L.KITTI_FOCAL, L.KITTI_CX, L.KITTI_CY

    def proj(R, t, p):
        X = p @ R.T + t
        return np.stack([f * X[:, 0] / X[:, 2] + cx, f * X[:, 1] / X[:, 2] + cy], axis=1)

    ptr, uv0, uv1, truth = [0], [], [], []
    for n, pose in records:
        base = float(np.linalg.norm(pose[4:]))
        z0 = base * rng.uniform(*gen["plane_depth_in_baselines"])
        sx = rng.uniform(*gen["plane_slope_x"]) * rng.choice([-1.0, 1.0])
        sy = rng.uniform(*gen["plane_slope_y"])
        xn, yn = rng.uniform(-gen["x_over_z"], gen["x_over_z"], n), rng.uniform(-gen["y_over_z"], gen["y_over_z"], n)
        z = z0 / (1.0 - sx * xn - sy * yn)  # the plane z = z0 + sx x + sy y: 6-40 baselines deep over the image
        p = np.stack([z * xn, z * yn, z], axis=1)
        a = proj(np.eye(3), np.zeros(3), p) + gen["noise_px"] * rng.standard_normal((n, 2))
        b = proj(TV.quat_to_R(pose[:4]), pose[4:], p) + gen["noise_px"] * rng.standard_normal((n, 2))
        bad, ang = rng.random(n) < gen["outlier_fraction"], rng.uniform(0.0, 2.0 * np.pi, n)
        b[bad] += gen["outlier_px"] * np.stack([np.cos(ang), np.sin(ang)], axis=1)[bad]
        ptr.append(ptr[-1] + n)
        uv0.append(a); uv1.append(b); truth.append(pose)
    return dict(point_ptr=np.array(ptr, dtype=np.int32), uv0=np.concatenate(uv0), uv1=np.concatenate(uv1),
                cam1_true=np.stack(truth))


def step_homography(args):
    from sim3opt_amd import lib as L
    import two_view_batch as TV
    P = make_problems(TV.read_records())
    counts = np.diff(P["point_ptr"])
    h = L.HomographyBatch(**HOM_OPTS)

    def call():
        h.set_problems(P["point_ptr"], P["uv0"], P["uv1"])
        return h.solve()

    t = EB.timed(call, args.runs, args.warmup)
    s, poses = h.summary(), h.poses()
    ok = s["status"] == 0
    truth = P["cam1_true"]
    dot = np.abs((poses[:, :4] * truth[:, :4]).sum(1)).clip(max=1.0)
    rot = 2 * np.arccos(dot)
    tdir = truth[:, 4:] / np.linalg.norm(truth[:, 4:], axis=1)[:, None]
    norm = np.linalg.norm(poses[:, 4:], axis=1)
    ang = np.arccos(np.clip((poses[:, 4:] * tdir).sum(1) / np.where(norm > 0, norm, 1.0), -1.0, 1.0))
    planted = ok & (ang < 0.2)
    return dict(problems=len(counts), points_min=int(counts.min()), points_max=int(counts.max()),
                points_total=int(counts.sum()), generator=GEN, homography_options=HOM_OPTS, homography_ms=t,
                result=dict(status_counts=[int((s["status"] == k).sum()) for k in range(5)],
                            inlier_share_min=float((s["n_inliers"] / counts)[ok].min()),
                            inlier_share_max=float((s["n_inliers"] / counts)[ok].max()),
                            ambiguity_branch=int(s["ambiguous"][ok].sum()),
                            rotation_rad_max=float(rot[ok].max()), direction_rad_max=float(ang[ok].max()),
                            chosen_is_planted=int(planted.sum()),
                            rotation_rad_max_where_planted=float(rot[planted].max()),
                            direction_rad_max_where_planted=float(ang[planted].max())))


def step_essential(args):
    r = EB.step_essential(args)
    rec = json.load(open(os.path.join(ROOT, "profiles", "essential_batch.json")))["essential_ms"]
    return dict(essential_ms=r["essential_ms"], essential_ms_recorded=rec)


step_pnp, step_two_view, step_match = EB.step_pnp, EB.step_two_view, EB.step_match


def kernel_trace(path):
    """the sim3opt_homography rows of a rocprofv3 kernel_stats.csv"""
    import csv
    with open(path) as f:
        rows = [r for r in csv.DictReader(f) if "sim3opt_homography::" in r["Name"]]
    return dict(source=os.path.relpath(os.path.abspath(path), ROOT),
                kernels={r["Name"].split("::")[1].split("(")[0]: dict(calls=int(r["Calls"]),
                                                                      average_us=float(r["AverageNs"]) / 1e3,
                                                                      min_us=float(r["MinNs"]) / 1e3,
                                                                      max_us=float(r["MaxNs"]) / 1e3) for r in rows},
                note="rocprofv3 --kernel-trace --stats, a run of its own of `--step homography` with no other tracing")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "homography_batch.json"))
    ap.add_argument("--kernel-stats", help="the kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of "
                                           "`--step homography` (a run of its own): its rows go into the JSON")
    ap.add_argument("--step", choices=[s for s, _ in STEPS], help="run one step in this process and print its JSON")
    args = ap.parse_args()
    if args.runs < 5:
        ap.error("--runs: at least 5")
    if args.step:
        print(json.dumps(globals()["step_" + args.step](args)))
        return 0
    res = dict(runs=args.runs, warmup=args.warmup,
               timing="host wall clock around calls that return after the device synchronise; warm; median of runs; "
                      "every run re-submits its problems; every step a process of its own",
               claim="none: nothing is known about this kernel's time, no target was set and no speed-up is claimed")
    for step, limit in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--runs", str(args.runs), "--warmup",
               str(args.warmup)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"step {step}: no result within {limit} s; stopping", file=sys.stderr)
            return 1
        if r.returncode != 0:
            print(f"step {step}: exit status {r.returncode}; stopping\n{r.stderr}", file=sys.stderr)
            return 1
        res.update(json.loads(r.stdout.strip().splitlines()[-1]))
    res["kernel_trace"] = kernel_trace(args.kernel_stats) if args.kernel_stats else \
        "not collected in this run (rocprofv3 --kernel-trace --stats, see the docstring)"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k.endswith("_ms") or k in ("problems", "points_total", "result", "kernel_trace")}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
