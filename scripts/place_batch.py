"""Times the batched bag-of-words place recognition (sim3opt_place_batch) and writes profiles/place_batch.json.

    python scripts/place_batch.py [--runs 11] [--levels 4 6] [--out profiles/place_batch.json]

KITTI-00's 771 keyframes (tests/golden/kitti00/framePoses_kf.txt) with 2000 descriptors a keyframe, and revisits planted
at the fixture's 118 loop pairs (tests/golden/kitti00/loopConstraints.txt).  The reference stores neither descriptors
nor a vocabulary, so both are synthetic and seeded: the vocabulary a 10-ary tree of 4 (and 6) levels whose centres
spread less from level to level, a keyframe's descriptors the centres of its words with a little noise; a keyframe
shares words with the one before it, and the later keyframe of a loop pair with the earlier one.  The generator's
parameters are in the JSON.

Timing: host wall clock around calls that return after the device synchronise, warm, median over the runs, for
set_frames + solve and for solve alone on resident frames.  Counted: the candidates, how many of the planted loop pairs
come back (a candidate at the later keyframe whose match is within 3 keyframes of the earlier one), and the statuses.
No target is set and no speed-up is claimed: DBoW2 and DLoopDetector cannot be built here and there is no earlier
number for this step.  PARITY UNPINNED (include/sim3opt.h).  For kernel times run this script once under
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
os.environ.setdefault("SIM3OPT_PRELOAD_TORCH", "1")

from sim3opt_amd import lib as L  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "kitti00")
GEN = dict(seed=20261020, descriptors=2000, arity=10, level_spread=0.45, descriptor_noise_in_leaf_spreads=0.1,
           shared_with_previous=600, shared_with_revisited=900, weight_range=[1.0, 8.0])


def keyframes_and_loops():
    """(n_keyframes, [(earlier keyframe, later keyframe)]) of the fixture"""
    ids = [int(ln.split(",")[0]) for ln in open(os.path.join(GOLDEN, "framePoses_kf.txt")) if not ln.startswith("%")]
    index = {f: k for k, f in enumerate(ids)}
    lines = [ln for ln in open(os.path.join(GOLDEN, "loopConstraints.txt")).read().splitlines()[5:] if ln.strip()]
    loops = []
    for k in range(0, len(lines) - 3, 4):
        a, b = (index[int(x)] for x in lines[k].split()[:2])
        loops.append((min(a, b), max(a, b)))
    return len(ids), loops


def make_vocabulary(levels, gen=GEN):
    """A balanced tree in breadth-first order: (parent, centre, weight, word_id, index of the first leaf)"""
    rng = np.random.default_rng(gen["seed"] + levels)
    a = gen["arity"]
    counts = [a ** l for l in range(levels + 1)]
    n = sum(counts)
    parent = np.full(n, -1, dtype=np.int32)
    centre = np.zeros((n, 64), dtype=np.float32)
    lo = 0
    for l in range(1, levels + 1):
        first, m = lo + counts[l - 1], counts[l]
        parent[first:first + m] = lo + np.arange(m) // a
        centre[first:first + m] = centre[parent[first:first + m]] + \
            (gen["level_spread"] ** l) * rng.standard_normal((m, 64)).astype(np.float32)
        lo = first
    word_id = np.full(n, -1, dtype=np.int32)
    word_id[lo:] = rng.permutation(counts[-1]).astype(np.int32)
    weight = np.zeros(n)
    weight[lo:] = rng.uniform(*gen["weight_range"], counts[-1])
    return parent, centre, weight, word_id, lo


def make_frames(n_frames, loops, centre, first_leaf, gen=GEN):
    """(kp_ptr, desc): every keyframe's leaves are chosen first (shared with the keyframe before, with the revisited
    keyframe, the rest at random), then the descriptors are those leaves' centres with noise"""
    rng = np.random.default_rng(gen["seed"] + 1)
    n_leaves, d = len(centre) - first_leaf, gen["descriptors"]
    revisited = {}
    for a, b in loops:
        revisited.setdefault(b, a)
    leaves = []
    for f in range(n_frames):
        parts = []
        if f:
            parts.append(rng.choice(leaves[f - 1], gen["shared_with_previous"], replace=False))
        if f in revisited:
            parts.append(rng.choice(leaves[revisited[f]], gen["shared_with_revisited"], replace=False))
        have = sum(len(p) for p in parts)
        parts.append(rng.integers(n_leaves, size=d - have))
        leaves.append(np.concatenate(parts))
    desc = np.empty((n_frames * d, 64), dtype=np.float32)
    levels = int(round(np.log(n_leaves) / np.log(gen["arity"])))
    noise = gen["descriptor_noise_in_leaf_spreads"] * gen["level_spread"] ** levels
    for f in range(n_frames):
        desc[f * d:(f + 1) * d] = centre[first_leaf + leaves[f]] + \
            noise * rng.standard_normal((d, 64)).astype(np.float32)
    return np.arange(n_frames + 1, dtype=np.int32) * d, desc


def ms(t):
    return dict(median=1e3 * float(np.median(t)), min=1e3 * min(t), max=1e3 * max(t))


def run(levels, n_frames, loops, runs, warmup):
    t0 = time.perf_counter()
    parent, centre, weight, word_id, first_leaf = make_vocabulary(levels)
    kp_ptr, desc = make_frames(n_frames, loops, centre, first_leaf)
    t_gen = time.perf_counter() - t0
    b = L.PlaceBatch()
    t0 = time.perf_counter()
    b.set_vocabulary(parent, centre, weight, word_id)
    t_voc = time.perf_counter() - t0

    def whole():
        b.set_frames(kp_ptr, desc)
        return b.solve()

    for _ in range(warmup):
        whole()
    tw, ts = [], []
    for _ in range(runs):
        t0 = time.perf_counter()
        whole()
        tw.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        n_cand = b.solve()
        ts.append(time.perf_counter() - t0)
    r, pairs, (bow_ptr, _, _) = b.results(), b.pairs(), b.bow()
    match_of = {int(q): int(m) for q, m in pairs}
    found = sum(1 for a, q in loops if q in match_of and abs(match_of[q] - a) <= 3)
    out = dict(levels=levels, nodes=int(len(parent)), words=int(len(parent) - first_leaf),
               generation_s=t_gen, set_vocabulary_ms=1e3 * t_voc,
               set_frames_solve_ms=ms(tw), solve_only_ms=ms(ts), candidates=int(n_cand),
               planted_loop_pairs=len(loops), planted_loop_pairs_found=int(found),
               candidates_not_at_a_planted_keyframe=int(sum(1 for q in match_of if q not in {b_ for _, b_ in loops})),
               status_counts=[int((r["status"] == k).sum()) for k in range(7)],
               words_per_vector=dict(mean=float(np.diff(bow_ptr).mean()), min=int(np.diff(bow_ptr).min()),
                                     max=int(np.diff(bow_ptr).max())),
               device_memory_bytes=L.device_memory_in_use()[1])
    b.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--levels", type=int, nargs="+", default=[4, 6])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "place_batch.json"))
    ap.add_argument("--kernel-stats", help="the kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of this script "
                                           "(a run of its own): its sim3opt_place rows go into the JSON")
    args = ap.parse_args()
    n_frames, loops = keyframes_and_loops()
    res = dict(keyframes=n_frames, generator=GEN, runs=args.runs, warmup=args.warmup,
               timing="host wall clock around calls that return after the device synchronise; warm; median of runs",
               claim="none: DBoW2 and DLoopDetector cannot be built here and there is no earlier number for this step",
               parity="unpinned: synthetic vocabulary and descriptors; see include/sim3opt.h",
               status_order=["CANDIDATE", "CLOSE_MATCHES_ONLY", "NO_DB_RESULTS", "LOW_NSS_FACTOR", "LOW_SCORES",
                             "NO_GROUPS", "NO_TEMPORAL_CONSISTENCY"],
               vocabularies=[run(l, n_frames, loops, args.runs, args.warmup) for l in args.levels],
               kernel_trace="not collected in this run (rocprofv3 --kernel-trace --stats, see the docstring)")
    if args.kernel_stats:
        import csv
        with open(args.kernel_stats) as f:
            rows = [r for r in csv.DictReader(f) if "sim3opt_place::" in r["Name"]]
        res["kernel_trace"] = dict(
            source=os.path.relpath(os.path.abspath(args.kernel_stats), ROOT),
            kernels={r["Name"].split("::")[1].split("(")[0]: dict(calls=int(r["Calls"]), average_us=float(r["AverageNs"]) / 1e3,
                                                                 min_us=float(r["MinNs"]) / 1e3, max_us=float(r["MaxNs"]) / 1e3)
                     for r in rows},
            note="rocprofv3 --kernel-trace --stats, a run of its own of this script with no other tracing; the calls of "
                 "every vocabulary of that run together")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(keyframes=n_frames, vocabularies=res["vocabularies"])))


if __name__ == "__main__":
    main()
