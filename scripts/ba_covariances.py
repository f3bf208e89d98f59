"""Cost of the bundle-adjustment covariances (sim3opt_ba_covariances) on scripts/gpu_ba_scale.py's KITTI-sized problem
(771 cameras, 123 k points): all camera diagonal blocks, all consecutive camera pairs and all points in one call, next
to one LM iteration of the same handle.  Wall clock, warm, median of 11.  Reported only: nobody has measured this step
before, no target is set.

    python scripts/ba_covariances.py [--out profiles/ba_covariances.json] [--kernel-stats <kernel_stats.csv>]
    python scripts/ba_covariances.py --calls 5         (the workload alone: the target of a
                                                         `rocprofv3 --kernel-trace --stats -- python ...` run of its own)

Cameras 0 and 1 are fixed (the gauge).  Points the generator leaves with one observation and cameras it leaves without
any make H singular at lambda = 0, so lambda = 1 is used when any remain, else 0; which one is in the output.  The
consecutive pairs are those that share a point (the others are outside the factor's pattern)."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from gpu_ba_scale import kitti_like  # noqa: E402
from sim3opt_amd import lib as L  # noqa: E402


def median_ms(f, n=11):
    t = []
    for _ in range(n):
        t0 = time.perf_counter()
        f()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), [round(x, 3) for x in t]


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ba_covariances.json"))
    ap.add_argument("--calls", type=int, default=0, help="run that many covariance calls after a warm one and stop")
    ap.add_argument("--kernel-stats", help="kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of --calls")
    a = ap.parse_args()
    cams, pts, oc, op, uv = kitti_like()
    nc, npt = len(cams), len(pts)
    seen_once = int((np.bincount(op, minlength=npt) < 2).sum())
    unobserved = int((np.bincount(oc, minlength=nc) == 0).sum())
    lam = 1.0 if seen_once or unobserved else 0.0
    fixed = np.zeros(nc, dtype=np.uint8)
    fixed[:2] = 1
    b = L.BundleAdjuster()
    b.set_problem(cams, pts, oc, op, uv)
    b.set_fixed_cameras(fixed)
    b.optimize(2)  # uploads, plans, and a map an adjuster would ask about
    c = np.arange(nc, dtype=np.int32)
    first, last = np.full(npt, nc), np.full(npt, -1)  # (tracks are runs of consecutive cameras)
    np.minimum.at(first, op, oc)
    np.maximum.at(last, op, oc)
    shares_next = np.zeros(nc, dtype=bool)
    for p in np.flatnonzero(last > first):
        shares_next[first[p]:last[p]] = True
    nxt = c[:-1][shares_next[:-1]]
    cam_pairs = np.concatenate([np.stack([c, c], axis=1), np.stack([nxt, nxt + 1], axis=1)])
    points = np.arange(npt, dtype=np.int32)
    call = lambda: b.covariances(cam_pairs=cam_pairs, points=points, lam=lam)
    cc, pp, _ = call()  # the first call builds the context
    assert np.isfinite(cc).all() and np.isfinite(pp).all()
    if a.calls:
        for _ in range(a.calls):
            call()
        return
    cov_ms, cov_all = median_ms(call)
    st = b.covariance_stats()
    cams_ms, _ = median_ms(lambda: b.covariances(cam_pairs=cam_pairs, lam=lam))
    lm_ms, lm_all = median_ms(lambda: b.optimize(1))
    out = dict(problem=dict(n_cams=nc, n_points=npt, n_obs=len(oc), fixed_cameras=2, points_seen_once=seen_once,
                            cameras_without_observations=unobserved),
               lam=lam, request=dict(camera_blocks=int(len(cam_pairs)), point_blocks=int(npt)), stats=st,
               covariances_ms_median_of_11=round(cov_ms, 3), covariances_ms=cov_all,
               camera_blocks_only_ms_median_of_11=round(cams_ms, 3),
               lm_iteration_ms_median_of_11=round(lm_ms, 3), lm_iteration_ms=lm_all,
               lm_trials_last=[s["trials"] for s in b.stats()],
               note="wall clock of the Python call (host planning, launches, copies), warm; no target is set")
    if a.kernel_stats:
        rows = list(csv.DictReader(open(a.kernel_stats)))
        out["kernel_stats"] = dict(
            source="rocprofv3 --kernel-trace --stats, a run of its own of `--calls 5` (two LM iterations and six calls)",
            kernels=[{k: r[k] for k in ("Name", "Calls", "TotalDurationNs", "AverageNs", "Percentage") if k in r}
                     for r in rows[:14]])
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps({k: out[k] for k in ("lam", "covariances_ms_median_of_11", "camera_blocks_only_ms_median_of_11",
                                          "lm_iteration_ms_median_of_11", "stats")}))


if __name__ == "__main__":
    main()
