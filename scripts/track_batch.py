"""Times the batched loop tracks (sim3opt_track_batch) and writes profiles/track_batch.json.

    python scripts/track_batch.py [--runs 11] [--out profiles/track_batch.json] [--kernel-stats kernel_stats.csv]

Workloads:
  (a) loop closing: 118 pairs over 221 frames.  The 29 pairs of tests/golden/kitti00/loop_tracks_29pairs.npy as they
      are (the reference's own matches; every frame that occurs in more than one pair is among them), and 89 pairs over
      frames of their own with the fixture's per-pair match counts (219 .. 1047) in turn and seeded distinct indices.
  (b) sequential matching: 771 frames of 2000 keypoints, every consecutive and second-neighbour pair, 1000 matches each
      between keypoints of the same index, so that tracks run over tens of frames.
Depths are seeded (2 .. 40, one in five absent) and the cameras near the identity: the arithmetic is the same whatever
they hold.

Timing: host wall clock around calls that return after the device synchronise, warm, median over the runs: set_matches
+ solve (the matches are checked on the host and uploaded again), solve alone on resident inputs, and next to them
sim3opt_track_reference, the serial restatement, on the same inputs on the host.  No target is set and no speed-up is
claimed: there is no earlier number for this step.  For kernel times run this script once under `rocprofv3
--kernel-trace --stats --output-format csv` (a run of its own), and pass its kernel_stats.csv to a timing run with
--kernel-stats.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("SIM3OPT_PRELOAD_TORCH", "1")

from sim3opt_amd import lib as L  # noqa: E402
import track_cases as TC  # noqa: E402

SEED = 20261021


def finish(name, n_kp, pairs, match_ptr, q, t, rng):
    kp_ptr = np.concatenate([[0], np.cumsum(n_kp)]).astype(np.int32)
    M = len(q)
    depth = [np.where(rng.random(M) < 0.2, np.nan, rng.uniform(2, 40, M)) for _ in range(2)]
    return dict(name=name, kp_ptr=kp_ptr, kp=TC.pixels(int(kp_ptr[-1]), SEED), pairs=np.asarray(pairs, np.int32),
                match_ptr=np.asarray(match_ptr, np.int32), query_idx=np.asarray(q, np.int32), train_idx=np.asarray(t, np.int32),
                mask=None, depth0=depth[0], depth1=depth[1], states=TC.random_states(len(n_kp), SEED))


def loop_closing():
    rng = np.random.default_rng(SEED)
    c = TC.fixture(False)
    counts = np.diff(c["match_ptr"])
    n_kp, pairs = list(np.diff(c["kp_ptr"])), c["pairs"].tolist()
    q, t, ptr = c["query_idx"].tolist(), c["train_idx"].tolist(), c["match_ptr"].tolist()
    for k in range(118 - len(pairs)):
        n = int(counts[k % len(counts)])
        pairs.append((len(n_kp), len(n_kp) + 1))
        n_kp += [2000, 2000]
        q += rng.permutation(2000)[:n].tolist()
        t += rng.permutation(2000)[:n].tolist()
        ptr.append(len(q))
    return finish("loop_closing_118_pairs", n_kp, pairs, ptr, q, t, rng)


def sequential(n_frames=771, n_kp=2000, n_matches=1000):
    rng = np.random.default_rng(SEED + 1)
    pairs = [(i, i + s) for i in range(n_frames) for s in (1, 2) if i + s < n_frames]
    idx = np.concatenate([np.sort(rng.permutation(n_kp)[:n_matches]) for _ in pairs])
    return finish("sequential_771_frames", [n_kp] * n_frames, pairs, np.arange(len(pairs) + 1) * n_matches, idx, idx, rng)


def ms(t):
    return dict(median=1e3 * float(np.median(t)), min=1e3 * min(t), max=1e3 * max(t))


def measure(c, runs, warmup):
    T = L.TrackBatch()
    T.set_frames(c["kp_ptr"], c["kp"])
    T.set_cameras(c["states"])
    mt = {k: c[k] for k in ("pairs", "match_ptr", "query_idx", "train_idx", "mask", "depth0", "depth1")}
    ref_kw = dict(kp_ptr=c["kp_ptr"], kp=c["kp"], states=c["states"], **mt)
    for _ in range(warmup):
        T.set_matches(**mt)
        T.solve()
    t_set, t_solve, t_ref = [], [], []
    for _ in range(runs):
        t0 = time.perf_counter()
        T.set_matches(**mt)
        kept = T.solve()
        t_set.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        T.solve()
        t_solve.append(time.perf_counter() - t0)
    for _ in range(max(3, runs // 3)):
        t0 = time.perf_counter()
        ref = L.TrackBatch.reference(**ref_kw)
        t_ref.append(time.perf_counter() - t0)
    d, tr = T.dims(), T.tracks()
    same = all(np.array_equal(tr[k], ref[k]) for k in tr) and T.points()[0].tobytes() == ref["points"].tobytes()
    lengths = np.diff(tr["track_ptr"])
    out = dict(frames=d["n_frames"], pairs=d["n_pairs"], matches=d["total_matches"], keypoints=int(c["kp_ptr"][-1]),
               tracks=d["n_tracks"], observations=d["n_observations"], kept_tracks=kept, rounds=d["rounds"],
               track_length=dict(max=int(lengths.max()), mean=float(lengths.mean()),
                                 over_wave_max=int((lengths > d["wave_max"]).sum()), over_lane_max=int((lengths > d["lane_max"]).sum())),
               status_counts=[int((tr["status"] == k).sum()) for k in range(5)],
               set_matches_solve_ms=ms(t_set), solve_resident_ms=ms(t_solve), host_reference_ms=ms(t_ref),
               device_equals_host_reference=bool(same))
    T.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_batch.json"))
    ap.add_argument("--kernel-stats", help="the kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of this script "
                                           "(a run of its own): its sim3opt_track rows go into the JSON")
    args = ap.parse_args()
    res = dict(runs=args.runs, warmup=args.warmup, seed=SEED,
               timing="host wall clock around calls that return after the device synchronise; warm; median of runs; "
                      "host_reference_ms is sim3opt_track_reference, the serial restatement, on the same inputs",
               claim="none: no target is set and there is no earlier number for this step",
               workloads={c["name"]: measure(c, args.runs, args.warmup) for c in (loop_closing(), sequential())},
               kernel_trace="not collected in this run (rocprofv3 --kernel-trace --stats, see the docstring)")
    if args.kernel_stats:
        import csv
        with open(args.kernel_stats) as f:
            rows = [r for r in csv.DictReader(f) if "sim3opt_track::" in r["Name"]]
        res["kernel_trace"] = dict(
            source=os.path.basename(args.kernel_stats),
            note="rocprofv3 --kernel-trace --stats, a run of its own of this script over both workloads and all their "
                 "warm-up and timed solves, with no other tracing; total_ms sums every call; the csv is kept as "
                 "profiles/track_batch_kernel_stats.csv",
            kernels={r["Name"].split("::")[1].split("(")[0]: dict(calls=int(r["Calls"]), total_ms=float(r["TotalDurationNs"]) / 1e6,
                                                                  average_us=float(r["AverageNs"]) / 1e3,
                                                                  min_us=float(r["MinNs"]) / 1e3, max_us=float(r["MaxNs"]) / 1e3)
                     for r in rows})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res["workloads"]))


if __name__ == "__main__":
    main()
