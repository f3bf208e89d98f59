"""Times the batched essential-matrix RANSAC (sim3opt_essential_batch: E and the depth-free relative pose of every loop
candidate in one launch) and writes profiles/essential_batch.json.

    python scripts/essential_batch.py [--runs 11] [--out profiles/essential_batch.json]

The 118 problems take their point counts and the poses they are planted with from the 118 records of
tests/golden/kitti00/loopConstraints.txt (scripts/two_view_batch.py reads them; scripts/pnp_batch.py's generator makes
the scenes).  The detector's matched pixels are not stored with the reference, so they are synthetic: seeded, 0.3 px
noise on both views, a quarter of camera 1's pixels moved by a gross error of 40 px; the generator's parameters are
recorded in the JSON.

Timing: host wall clock around calls that return after the device synchronise, warm, median over the runs; every run
re-submits its problems.  Nothing is known about this kernel's time: no target is set and NO SPEED-UP IS CLAIMED
(OpenCV cannot be built here, and there is no earlier number for this step).  The same run also times set_problems +
solve of PnpBatch, set_problems + optimize of TwoViewBatch and set_frames + set_pairs + solve of MatchBatch, each on
the problems of its own script (scripts/pnp_batch.py, two_view_batch.py, match_batch.py), next to the medians
profiles/pnp_batch.json, two_view_batch.json and match_batch.json hold: evidence that the other stages were left alone.

Every step is a process of its own under its own time limit, and the script stops at the first one that fails.  For
the kernel time, run `--step essential` once under `rocprofv3 --kernel-trace --stats --output-format csv` (a run of
its own, no other tracing), store its kernel_stats.csv as profiles/essential_batch_kernel_stats.csv and pass it to
the timing run with --kernel-stats: the JSON then holds the k_essential_ransac row.  Needs a GPU; there is no fallback.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
os.environ.setdefault("SIM3OPT_PRELOAD_TORCH", "1")

GEN = dict(seed=20240612, depth_in_baselines=[6.0, 40.0], x_over_z=0.55, y_over_z=0.18, noise_px=0.3,
           outlier_fraction=0.25, outlier_px=40.0)
ESS_OPTS = dict(threshold=1.0, distance_threshold=50.0, iterations=1000, min_points=9, seed=0)
STEPS = (("essential", 240), ("pnp", 120), ("two_view", 120), ("match", 240))  # (step, its time limit in seconds)


def ms(t):
    return dict(median=1e3 * float(np.median(t)), min=1e3 * min(t), max=1e3 * max(t))


def timed(call, runs, warmup):
    for _ in range(warmup):
        call()
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        call()
        t.append(time.perf_counter() - t0)
    return ms(t)


def step_essential(args):
    from sim3opt_amd import lib as L
    import pnp_batch as PB
    import two_view_batch as TV
    P = PB.make_problems(TV.read_records(), GEN)
    counts = np.diff(P["point_ptr"])
    e = L.EssentialBatch(**ESS_OPTS)

    def call():
        e.set_problems(P["point_ptr"], P["uv0"], P["uv1"])
        return e.solve()

    t = timed(call, args.runs, args.warmup)
    s, poses = e.summary(), e.poses()
    truth = P["cam1_true"]
    dot = np.abs((poses[:, :4] * truth[:, :4]).sum(1)).clip(max=1.0)
    tdir = truth[:, 4:] / np.linalg.norm(truth[:, 4:], axis=1)[:, None]
    ang = np.arccos(np.clip((poses[:, 4:] * tdir).sum(1), -1.0, 1.0))
    return dict(problems=len(counts), points_min=int(counts.min()), points_max=int(counts.max()),
                points_total=int(counts.sum()), generator=GEN, essential_options=ESS_OPTS, essential_ms=t,
                result=dict(status_counts=[int((s["status"] == k).sum()) for k in range(4)],
                            inlier_share_min=float((s["votes_winner"] / counts).min()),
                            inlier_share_max=float((s["votes_winner"] / counts).max()),
                            rotation_rad_max=float((2 * np.arccos(dot)).max()), direction_rad_max=float(ang.max())))


def step_pnp(args):
    from sim3opt_amd import lib as L
    import pnp_batch as PB
    import two_view_batch as TV
    P = PB.make_problems(TV.read_records())
    pnp = L.PnpBatch(**PB.PNP_OPTS)
    return dict(pnp_ms=timed(lambda: PB.run_pnp(pnp, P), args.runs, args.warmup),
                pnp_ms_recorded=json.load(open(os.path.join(ROOT, "profiles", "pnp_batch.json")))["pnp_ms"])


def step_two_view(args):
    from sim3opt_amd import lib as L
    import two_view_batch as TV
    P = TV.make_problems(TV.read_records())
    ba = L.TwoViewBatch(**TV.OPTS)
    rec = json.load(open(os.path.join(ROOT, "profiles", "two_view_batch.json")))["batch_ms"]
    return dict(two_view_ms=timed(lambda: TV.run_batch(ba, P), args.runs, args.warmup), two_view_ms_recorded=rec)


def step_match(args):
    from sim3opt_amd import lib as L
    import match_batch as MB
    import two_view_batch as TV
    records = TV.read_records()
    F = MB.make_frames(records)
    pairs = np.arange(2 * len(records), dtype=np.int32).reshape(len(records), 2)
    m = L.MatchBatch()

    def call():
        m.set_frames(**F)
        m.set_pairs(pairs)
        return m.solve()

    rec = json.load(open(os.path.join(ROOT, "profiles", "match_batch.json")))["set_frames_set_pairs_solve_ms"]
    return dict(match_ms=timed(call, args.runs, args.warmup), match_ms_recorded=rec)


def kernel_trace(path):
    """the sim3opt_essential rows of a rocprofv3 kernel_stats.csv"""
    import csv
    with open(path) as f:
        rows = [r for r in csv.DictReader(f) if "sim3opt_essential::" in r["Name"]]
    return dict(source=os.path.relpath(os.path.abspath(path), ROOT),
                kernels={r["Name"].split("::")[1].split("(")[0]: dict(calls=int(r["Calls"]),
                                                                      average_us=float(r["AverageNs"]) / 1e3,
                                                                      min_us=float(r["MinNs"]) / 1e3,
                                                                      max_us=float(r["MaxNs"]) / 1e3) for r in rows},
                note="rocprofv3 --kernel-trace --stats, a run of its own of `--step essential` with no other tracing")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "essential_batch.json"))
    ap.add_argument("--kernel-stats", help="the kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of "
                                           "`--step essential` (a run of its own): its rows go into the JSON")
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
               claim="none: nothing is known about this kernel's time, no target is set and no speed-up is claimed")
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
