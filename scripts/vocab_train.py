"""Times the batched vocabulary training (sim3opt_vocabulary) and writes profiles/vocab_train.json.

    python scripts/vocab_train.py [--runs 11] [--levels 4 6] [--out profiles/vocab_train.json]

KITTI-00's 771 keyframes with 2000 synthetic descriptors each, from the generator of scripts/place_batch.py (the
descriptors of its 10-ary tree of as many levels as are trained); the tree is trained with k = 10 and L = 4 and 6.

Timing: host wall clock around calls that return after the device synchronise, warm, median over the runs, for train()
on resident frames and for set_frames + train().  Reported per level: the Lloyd passes, and for the whole tree
n_unconverged and the leaf-level distortion (the mean d2 of a training descriptor to the centre of the leaf it was
clustered into).  Then the run of scripts/place_batch.py with the trained tree in place of the synthetic one:
candidates, planted pairs found and candidates elsewhere, next to the numbers recorded for the synthetic tree.  These
are reported, not asserted.  No target is set and no speed-up is claimed: DBoW2 cannot be built here and there is no
earlier number for this step.  PARITY UNPINNED (include/sim3opt.h).  For kernel times run this script once under
`rocprofv3 --kernel-trace --stats --output-format csv` (a run of its own) and pass its kernel_stats.csv with
--kernel-stats.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("SIM3OPT_PRELOAD_TORCH", "1")

import place_batch as PB  # noqa: E402
from sim3opt_amd import lib as L  # noqa: E402

# profiles/place_batch.json: candidates / planted pairs found / candidates elsewhere with the synthetic trees
RECORDED = {4: (184, 101, 83), 6: (106, 101, 5)}
HBM_PEAK_TBS = 8.0  # MI355X, vendor figure


def run(levels, n_frames, loops, runs, warmup, max_iters):
    _, centre, _, _, first_leaf = PB.make_vocabulary(levels)
    kp_ptr, desc = PB.make_frames(n_frames, loops, centre, first_leaf)
    t = L.VocabularyTrainer(k=10, levels=levels, max_iters=max_iters, seed=1)

    def whole():
        t.set_frames(kp_ptr, desc)
        return t.train()

    for _ in range(warmup):
        whole()
    tw, tt = [], []
    for _ in range(runs):
        t0 = time.perf_counter()
        whole()
        tw.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        t.train()
        tt.append(time.perf_counter() - t0)
    dims = t.dims()
    voc = t.vocabulary()
    leaf = t.assignment()
    diff = desc.astype(np.float64) - voc[1][leaf].astype(np.float64)
    distortion = float((diff * diff).sum(axis=1).mean())
    held = L.device_memory_in_use()[1]
    t.close()
    # place recognition on the trained tree
    b = L.PlaceBatch()
    b.set_vocabulary(*voc)
    b.set_frames(kp_ptr, desc)
    n_cand = b.solve()
    match_of = {int(q): int(m) for q, m in b.pairs()}
    b.close()
    found = sum(1 for a, q in loops if q in match_of and abs(match_of[q] - a) <= 3)
    elsewhere = sum(1 for q in match_of if q not in {b_ for _, b_ in loops})
    passes = dims["passes"][:levels]
    n_desc = int(kp_ptr[-1])
    return dict(levels=levels, k=10, max_iters=max_iters, descriptors=n_desc, nodes=dims["n_nodes"], words=dims["n_words"],
                depth=dims["depth"], lloyd_passes_per_level=passes, n_unconverged=dims["n_unconverged"],
                leaf_level_distortion=distortion, train_ms=PB.ms(tt), set_frames_train_ms=PB.ms(tw),
                device_memory_bytes_held=held,
                assignment_pass_bytes=dict(descriptors_read=n_desc * 256, permutation_and_cluster=n_desc * 12,
                                           note="one pass over every member of the level: 64 floats, its index, its old and "
                                                "new cluster; the centres come from LDS"),
                place_recognition=dict(candidates=int(n_cand), planted_loop_pairs=len(loops), planted_loop_pairs_found=int(found),
                                       candidates_not_at_a_planted_keyframe=int(elsewhere),
                                       recorded_with_the_synthetic_tree=dict(zip(
                                           ("candidates", "planted_loop_pairs_found", "candidates_not_at_a_planted_keyframe"),
                                           RECORDED.get(levels, (None, None, None))))))


def add_kernel_trace(res, path):
    import csv
    with open(path) as f:
        rows = [r for r in csv.DictReader(f) if "sim3opt_vocab::" in r["Name"]]
    kernels = {r["Name"].split("::")[1].split("(")[0]: dict(calls=int(r["Calls"]), average_us=float(r["AverageNs"]) / 1e3,
                                                           min_us=float(r["MinNs"]) / 1e3, max_us=float(r["MaxNs"]) / 1e3)
               for r in rows}
    res["kernel_trace"] = dict(
        source=os.path.relpath(os.path.abspath(path), ROOT), kernels=kernels,
        note="rocprofv3 --kernel-trace --stats, a run of its own of this script (--runs 1 --warmup 0) with no other "
             "tracing; the calls of every training of that run together")
    if "k_vt_assign" in kernels:
        b = res["trainings"][0]["assignment_pass_bytes"]
        per_pass = b["descriptors_read"] + b["permutation_and_cluster"]
        res["kernel_trace"]["assignment_pass"] = dict(
            bytes_per_full_pass=per_pass, slowest_call_us=kernels["k_vt_assign"]["max_us"],
            tb_per_s_at_the_slowest_call=per_pass / (kernels["k_vt_assign"]["max_us"] * 1e-6) / 1e12,
            hbm_peak_tb_per_s=HBM_PEAK_TBS,
            note="the slowest call is taken for a pass in which every member of a level is assigned (the byte count above); "
                 "later passes of a level skip the nodes that have converged, so their calls move fewer bytes and the "
                 "average says nothing of the rate.  A lower bound of the rate: a slower call that moved fewer bytes "
                 "would be counted with the full byte count only if it were the slowest")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--levels", type=int, nargs="+", default=[4, 6])
    ap.add_argument("--max-iters", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vocab_train.json"))
    ap.add_argument("--kernel-stats", help="the kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of this script "
                                           "(a run of its own): its sim3opt_vocab rows go into the JSON")
    ap.add_argument("--merge", help="no run: read this result JSON, add --kernel-stats to it, write it to --out")
    args = ap.parse_args()
    if args.merge:
        res = json.load(open(args.merge))
        add_kernel_trace(res, args.kernel_stats)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        return
    n_frames, loops = PB.keyframes_and_loops()
    res = dict(keyframes=n_frames, generator=PB.GEN, runs=args.runs, warmup=args.warmup,
               timing="host wall clock around calls that return after the device synchronise; warm; median of runs",
               claim="none: DBoW2 cannot be built here and there is no earlier number for this step",
               parity="unpinned: synthetic descriptors; see include/sim3opt.h",
               trainings=[run(l, n_frames, loops, args.runs, args.warmup, args.max_iters) for l in args.levels],
               kernel_trace="not collected in this run (rocprofv3 --kernel-trace --stats, see the docstring)")
    if args.kernel_stats:
        add_kernel_trace(res, args.kernel_stats)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(keyframes=n_frames, trainings=res["trainings"])))


if __name__ == "__main__":
    main()
