"""Times the batched two-view refinement (sim3opt_ba_batch: every loop candidate in one launch) against the same
problems run one after the other through the existing BundleAdjuster (2 cameras, camera 0 fixed, the same options),
and writes profiles/two_view_batch.json.

    python scripts/two_view_batch.py [--runs 11] [--out profiles/two_view_batch.json]

The 118 problems take their point counts (the match count that opens record line 4) and their start poses (record
line 3: Euler angles RPY of Rc12c2 and Tfins) from the 118 records of tests/golden/kitti00/loopConstraints.txt.
The detector's own inputs are not stored with the reference, so points and observations are synthetic: seeded, with
the generator's parameters recorded in the JSON.  Depths are drawn in units of the candidate's baseline |Tfins| (the
map is monocular: its unit is arbitrary), so the geometry is that of a metre-long baseline seen 6-40 m ahead.

Timing: host wall clock around calls that end in a device synchronise (both paths return only after their results
are on the host), after warm-up runs of the same shapes, the two paths alternating, median over the runs.  Each
timed run starts from the same start: the batch path re-submits its problems (set_problems + optimize), the
sequential path does set_problem + set_fixed_cameras + optimize per candidate.  Needs a GPU; there is no fallback.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("SIM3OPT_PRELOAD_TORCH", "1")

from sim3opt_amd import lib as L, sim3np as S3  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "kitti00", "loopConstraints.txt")
GEN = dict(seed=20240611, depth_in_baselines=[6.0, 40.0], x_over_z=0.55, y_over_z=0.18, noise_px=0.5,
           outlier_fraction=0.05, outlier_sigma_px=40.0, truth_rotation_sigma_rad=0.004,
           truth_translation_sigma_baselines=0.05, start_depth_sigma_rel=0.04)
OPTS = dict(max_iters=10, huber_delta=3.0, pixel_noise=1.0, tau=1e-5, user_lambda_init=50.0, max_trials=5)


def read_records(path=FIXTURE):
    """(matches of record line 4, start pose [q, t] of record line 3) of every record"""
    lines = [ln for ln in open(path).read().splitlines()[5:] if ln.strip()]
    out = []
    for k in range(0, len(lines) - 3, 4):
        c, d = lines[k + 2].split(), lines[k + 3].split()
        r, p, y, tx, ty, tz = [float(x) for x in c[2:8]]
        q = S3.R_to_quat(S3.euler_rpy_to_R(r, p, y)).reshape(4)
        out.append((int(d[0]), np.concatenate([q / np.linalg.norm(q), [tx, ty, tz]])))
    return out


def quat_to_R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def make_problems(records, gen=GEN):
    rng = np.random.default_rng(gen["seed"])
    f, cx, cy = L.KITTI_FOCAL, L.KITTI_CX, L.KITTI_CY
    proj = lambda R, t, p: np.stack([f * (p @ R.T + t)[:, 0] / (p @ R.T + t)[:, 2] + cx,
                                     f * (p @ R.T + t)[:, 1] / (p @ R.T + t)[:, 2] + cy], axis=1)
    ptr, cam1, pts, uv0, uv1 = [0], [], [], [], []
    for n, start in records:
        base = float(np.linalg.norm(start[4:]))
        z = base * rng.uniform(*gen["depth_in_baselines"], n)
        p = np.stack([z * rng.uniform(-gen["x_over_z"], gen["x_over_z"], n),
                      z * rng.uniform(-gen["y_over_z"], gen["y_over_z"], n), z], axis=1)
        w = gen["truth_rotation_sigma_rad"] * rng.standard_normal(3)
        dq = np.concatenate([0.5 * w, [1.0]])
        Rt = quat_to_R(dq / np.linalg.norm(dq)) @ quat_to_R(start[:4])
        tt = start[4:] + gen["truth_translation_sigma_baselines"] * base * rng.standard_normal(3)
        a = proj(np.eye(3), np.zeros(3), p) + gen["noise_px"] * rng.standard_normal((n, 2))
        b = proj(Rt, tt, p) + gen["noise_px"] * rng.standard_normal((n, 2))
        bad, view = rng.random(n) < gen["outlier_fraction"], rng.random(n) < 0.5
        gross = gen["outlier_sigma_px"] * rng.standard_normal((n, 2))
        a[bad & view] += gross[bad & view]
        b[bad & ~view] += gross[bad & ~view]
        ptr.append(ptr[-1] + n)
        cam1.append(start)
        pts.append(p * (1.0 + gen["start_depth_sigma_rel"] * rng.standard_normal(n))[:, None])
        uv0.append(a)
        uv1.append(b)
    n = len(records)
    cam0 = np.tile([0.0, 0, 0, 1, 0, 0, 0], (n, 1))
    return dict(point_ptr=np.array(ptr, dtype=np.int32), cam0=cam0, cam1=np.stack(cam1), points=np.concatenate(pts),
                uv0=np.concatenate(uv0), uv1=np.concatenate(uv1))


def run_batch(batch, P):
    batch.set_problems(**P)
    return batch.optimize()


def run_sequential(adjusters, P):
    ptr = P["point_ptr"]
    for k, b in enumerate(adjusters):
        lo, hi = int(ptr[k]), int(ptr[k + 1])
        n = hi - lo
        b.set_problem(np.stack([P["cam0"][k], P["cam1"][k]]), P["points"][lo:hi], np.tile([0, 1], n),
                      np.repeat(np.arange(n), 2), np.stack([P["uv0"][lo:hi], P["uv1"][lo:hi]], axis=1).reshape(-1, 2))
        b.set_fixed_cameras([1, 0])
        b.optimize(OPTS["max_iters"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "two_view_batch.json"))
    ap.add_argument("--no-sequential", action="store_true", help="time the batch alone")
    args = ap.parse_args()
    if args.runs < 5:
        ap.error("--runs: at least 5")
    records = read_records()
    P = make_problems(records)
    counts = np.diff(P["point_ptr"])
    res = dict(problems=len(records), points_min=int(counts.min()), points_max=int(counts.max()),
               points_total=int(counts.sum()), generator=GEN, options=OPTS, runs=args.runs, warmup=args.warmup,
               timing="host wall clock around calls that return after the device synchronise; median of runs; the two "
                      "paths alternate; every run starts from the same start (problems re-submitted)")
    batch = L.TwoViewBatch(**OPTS)
    seq_opts = {k: v for k, v in OPTS.items() if k != "max_iters"}
    adjusters = None
    if not args.no_sequential:
        try:
            adjusters = [L.BundleAdjuster(**seq_opts)]
            run_sequential(adjusters, dict(P, point_ptr=P["point_ptr"][:2]))
            adjusters = [L.BundleAdjuster(**seq_opts) for _ in records]
        except L.Sim3OptError as e:
            res["sequential"] = f"the sequential path could not run a 2-camera problem: {e}"
            adjusters = None
    for _ in range(args.warmup):
        run_batch(batch, P)
        if adjusters:
            run_sequential(adjusters, P)
    tb, ts = [], []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        run_batch(batch, P)
        tb.append(time.perf_counter() - t0)
        if adjusters:
            t0 = time.perf_counter()
            run_sequential(adjusters, P)
            ts.append(time.perf_counter() - t0)
    res["batch_ms"] = dict(median=1e3 * float(np.median(tb)), min=1e3 * min(tb), max=1e3 * max(tb))
    res["batch_iterations"] = [int(x) for x in batch.num_iterations()]
    if adjusters:
        res["sequential_ms"] = dict(median=1e3 * float(np.median(ts)), min=1e3 * min(ts), max=1e3 * max(ts))
        res["sequential_over_batch"] = float(np.median(ts) / np.median(tb))
        # per-problem agreement of the two paths (they sum in different orders: not bit for bit)
        c1, pts = batch.cameras()[1], batch.points()
        agree = dict(trials_equal=0, iterations_equal=0, chi2_rel=0.0, quaternion=0.0, translation_rel=0.0,
                     points_rel=0.0)
        for k, b in enumerate(adjusters):
            lo, hi = int(P["point_ptr"][k]), int(P["point_ptr"][k + 1])
            sb, ss = batch.stats(k), b.stats()
            agree["iterations_equal"] += len(sb) == len(ss)
            agree["trials_equal"] += [s["trials"] for s in sb] == [s["trials"] for s in ss]
            if sb and ss:
                agree["chi2_rel"] = max(agree["chi2_rel"], abs(sb[-1]["chi2_after"] - ss[-1]["chi2_after"]) /
                                        ss[-1]["chi2_after"])
            cs = b.cameras()[1]
            base = float(np.linalg.norm(cs[4:]))
            agree["quaternion"] = max(agree["quaternion"], float(min(np.abs(c1[k, :4] - cs[:4]).max(),
                                                                     np.abs(c1[k, :4] + cs[:4]).max())))
            agree["translation_rel"] = max(agree["translation_rel"], float(np.abs(c1[k, 4:] - cs[4:]).max() / base))
            agree["points_rel"] = max(agree["points_rel"], float(np.abs(pts[lo:hi] - b.points()).max() / base))
        agree["note"] = "worst over the problems; translation and points relative to the candidate's baseline"
        res["agreement"] = agree
    elif "sequential" not in res:
        res["sequential"] = "not timed (--no-sequential)"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: res[k] for k in ("problems", "points_total", "batch_ms", "sequential_ms",
                                          "sequential_over_batch", "agreement") if k in res}))


if __name__ == "__main__":
    main()
