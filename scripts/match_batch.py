"""Times the batched descriptor matching and map-depth lookup (sim3opt_match_batch) alone and as the head of the chain
match -> PnP -> two-view refinement, and writes profiles/match_batch.json.

    python scripts/match_batch.py [--runs 11] [--out profiles/match_batch.json] [--numpy-reference]

KITTI-00's 118 loop candidates (tests/golden/kitti00/loopConstraints.txt: their planted poses and, as each keyframe's
number of map-point observations, the records' point counts) with 2000 keypoints a keyframe.  The reference stores
neither descriptors nor keypoints, so these are synthetic: seeded unit-norm Gaussian SURF-64 stand-ins, keyframe 1
holding keyframe 0's points in another order with descriptor noise; the generator's parameters are in the JSON.

Timing: host wall clock around calls that return after the device synchronise, warm, median over the runs; every run
hands frames and pairs over again (and, as a line of its own, only the pairs: the frames stay on the device).  No speed-up over the reference is claimed: OpenCV / FLANN cannot be built here and
there is no earlier number for this step.  k_match_nn is n_query x n_train x 64 subtract-multiply-adds per pair; its
achieved rate counts two FP32 operations for each (the subtraction is not counted) against the 157 TFLOP/s vector
peak.  --numpy-reference also times tests/match_ref.py's FP32 path on the CPU for a few pairs, as orientation only: it
is a test reference, not a competitor.  For kernel times run this script once under `rocprofv3 --kernel-trace
--stats --output-format csv` (a run of its own), store its kernel_stats.csv as profiles/match_batch_kernel_stats.csv
and pass it to the timing run with --kernel-stats: the JSON then holds k_match_nn's time and rate.  Needs a GPU; there is no fallback."""
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

GEN = dict(seed=20261019, keypoints=2000, descriptor_noise=0.02, depth_in_baselines=[6.0, 40.0], x_over_z=0.55,
           y_over_z=0.18)


def make_frames(records, gen=GEN):
    rng = np.random.default_rng(gen["seed"])
    f, cx, cy, n = L.KITTI_FOCAL, L.KITTI_CX, L.KITTI_CY, gen["keypoints"]
    fr = dict(kp=[], desc=[], obs_uv=[], obs_depth=[], kp_ptr=[0], obs_ptr=[0])
    for n_obs, pose in records:
        base = float(np.linalg.norm(pose[4:]))
        z = base * rng.uniform(*gen["depth_in_baselines"], n)
        p = np.stack([z * rng.uniform(-gen["x_over_z"], gen["x_over_z"], n),
                      z * rng.uniform(-gen["y_over_z"], gen["y_over_z"], n), z], axis=1)
        X1 = p @ TV.quat_to_R(pose[:4]).T + pose[4:]
        d = rng.standard_normal((n, 64))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        perm = rng.permutation(n)
        d1 = d[perm] + gen["descriptor_noise"] * rng.standard_normal((n, 64))
        for X, dd in ((p, d), (X1[perm], d1)):
            uv = np.stack([f * X[:, 0] / X[:, 2] + cx, f * X[:, 1] / X[:, 2] + cy], axis=1)
            m = min(max(int(n_obs), 1), n)  # the keyframe's observations: the first m keypoints, at their points' depths
            fr["kp"].append(uv); fr["desc"].append(dd); fr["obs_uv"].append(uv[:m]); fr["obs_depth"].append(X[:m, 2])
            fr["kp_ptr"].append(fr["kp_ptr"][-1] + n); fr["obs_ptr"].append(fr["obs_ptr"][-1] + m)
    cat = lambda k: np.concatenate(fr[k]).astype(np.float32)
    return dict(kp_ptr=np.array(fr["kp_ptr"], np.int32), obs_ptr=np.array(fr["obs_ptr"], np.int32), kp=cat("kp"),
                desc=cat("desc"), obs_uv=cat("obs_uv"), obs_depth=cat("obs_depth"))


def ms(t):
    return dict(median=1e3 * float(np.median(t)), min=1e3 * min(t), max=1e3 * max(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_batch.json"))
    ap.add_argument("--numpy-reference", action="store_true", help="also time tests/match_ref.py (orientation only)")
    ap.add_argument("--kernel-stats", help="the kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of this script "
                                           "(a run of its own): its sim3opt_match rows go into the JSON")
    args = ap.parse_args()
    records = TV.read_records()
    F = make_frames(records)
    n = len(records)
    pairs = np.arange(2 * n, dtype=np.int32).reshape(n, 2)
    cam0 = np.tile([0.0, 0, 0, 1, 0, 0, 0], (n, 1))
    m, pnp, ba = L.MatchBatch(), L.PnpBatch(), L.TwoViewBatch(**TV.OPTS)

    def run_match():
        m.set_frames(**F)
        m.set_pairs(pairs)
        return m.solve()

    def run_chain():
        run_match()
        ptr, mt = m.match_ptr(), m.matches()
        keep = np.diff(ptr) > 8  # point_count > 8, kittiDetector.h:1282
        sel = np.concatenate([np.arange(ptr[k], ptr[k + 1]) for k in np.nonzero(keep)[0]])
        p2 = np.concatenate([[0], np.cumsum(np.diff(ptr)[keep])]).astype(np.int32)
        pnp.set_problems(p2, mt["points0"][sel], mt["uv1"][sel])
        pnp.solve()
        ba.set_problems(point_ptr=p2, cam0=cam0[keep], cam1=pnp.poses(), points=mt["points0"][sel], uv0=mt["uv0"][sel],
                        uv1=mt["uv1"][sel])
        ba.optimize()
        return int(keep.sum())

    for _ in range(args.warmup):
        run_chain()
    tm, ts, tp, tc = [], [], [], []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        run_match()
        tm.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        m.solve()
        ts.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        m.set_pairs(pairs)  # another candidate list on frames that stay on the device
        m.solve()
        tp.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        fed = run_chain()
        tc.append(time.perf_counter() - t0)
    s, ptr = m.summary(), m.match_ptr()
    macs = float(n) * GEN["keypoints"] ** 2 * 64
    res = dict(pairs=n, frames=2 * n, generator=GEN, observations_total=int(F["obs_ptr"][-1]), runs=args.runs,
               warmup=args.warmup,
               timing="host wall clock around calls that return after the device synchronise; warm; median of runs",
               claim="none: OpenCV / FLANN cannot be built here and there is no earlier number for this step",
               set_frames_set_pairs_solve_ms=ms(tm), solve_only_ms=ms(ts), set_pairs_solve_ms=ms(tp), match_pnp_two_view_ms=ms(tc),
               k_match_nn_flop=2 * macs,
               result=dict(status_counts=[int((s["status"] == k).sum()) for k in range(3)],
                           matches_total=int(ptr[-1]), matches_min=int(np.diff(ptr).min()),
                           matches_max=int(np.diff(ptr).max()), after_filters_total=int(s["n_after_filters"].sum()),
                           candidates_fed_to_pnp=fed, pnp_status_counts=[int((pnp.summary()["status"] == k).sum())
                                                                         for k in range(4)]),
               kernel_trace="not collected in this run (rocprofv3 --kernel-trace --stats, see the docstring)")
    if args.kernel_stats:
        import csv
        with open(args.kernel_stats) as f:
            rows = [r for r in csv.DictReader(f) if "sim3opt_match::" in r["Name"]]
        kt = {r["Name"].split("::")[1].split("(")[0]: dict(calls=int(r["Calls"]), average_us=float(r["AverageNs"]) / 1e3,
                                                            min_us=float(r["MinNs"]) / 1e3, max_us=float(r["MaxNs"]) / 1e3)
              for r in rows}
        nn = kt["k_match_nn"]["average_us"] * 1e-6
        res["kernel_trace"] = dict(source=os.path.relpath(os.path.abspath(args.kernel_stats), ROOT), kernels=kt,
                                   k_match_nn_tflops=2 * macs / nn / 1e12,
                                   k_match_nn_share_of_157_tflops_vector_peak=2 * macs / nn / 157.3e12,
                                   note="rocprofv3 --kernel-trace --stats, a run of its own of this script with no other "
                                        "tracing; two FP32 operations per subtract-multiply-add, the subtraction not "
                                        "counted (with it: 1.5 times the rate)")
    if args.numpy_reference:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import match_ref as R
        fr = lambda k: dict(kp=F["kp"][F["kp_ptr"][k]:F["kp_ptr"][k + 1]], desc=F["desc"][F["kp_ptr"][k]:F["kp_ptr"][k + 1]],
                            obs_uv=F["obs_uv"][F["obs_ptr"][k]:F["obs_ptr"][k + 1]],
                            obs_depth=F["obs_depth"][F["obs_ptr"][k]:F["obs_ptr"][k + 1]])
        intr = dict(focal=L.KITTI_FOCAL, cx=L.KITTI_CX, cy=L.KITTI_CY, image_width=L.KITTI_WIDTH,
                    image_height=L.KITTI_HEIGHT)
        t0 = time.perf_counter()
        for k in range(3):
            R.match_pair(fr(2 * k), fr(2 * k + 1), intr)
        res["numpy_reference_ms"] = dict(per_pair=1e3 * (time.perf_counter() - t0) / 3,
                                         note="tests/match_ref.py's FP32 numpy path on the CPU, mean of 3 pairs: "
                                              "orientation only, a test reference and not a competitor")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: res[k] for k in ("pairs", "set_frames_set_pairs_solve_ms", "solve_only_ms", "set_pairs_solve_ms", "kernel_trace",
                                          "match_pnp_two_view_ms", "result") if k in res}))


if __name__ == "__main__":
    main()
