"""Profiling target of sim3opt_covariances on KITTI-00 (run under rocprofv3 --kernel-trace --stats, one
configuration per run; scripts/prof_covariances.sh): 3 + 20 calls of one request, wall median of the 20.

    gpu_cov_prof.py one|all pairs|column|marginals      the target
    gpu_cov_prof.py summarise DIR OUT.csv               per-kernel medians over the calls (a call's dispatches of
                                                        one kernel summed; the 3 warm-up calls left out) of every
                                                        <tag>_kernel_trace.csv under DIR
"""
import csv, glob, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
WARM, CALLS = 3, 20


def target(which, what):
    from sim3opt_amd import lib as L
    import kitti_graph as K
    g = K.build_direct_graph(which == "one")
    G = L.Graph()
    G.add_vertices(g["states"], g["fixed"]); G.add_edges(g["v0"], g["v1"], g["meas"]); G.initialize()
    ids = np.flatnonzero(g["fixed"] == 0).astype(np.int32)
    if what == "pairs":  # 1000 random pairs of free vertices
        rng = np.random.default_rng(1)
        pairs = np.stack([rng.choice(ids, 1000), rng.choice(ids, 1000)], axis=1)
    else:  # one full block column: every free vertex against the deepest vertex of the elimination tree
        P = G.marginal_plan()
        depth = np.zeros(P["nb"], dtype=np.int64)
        for j in range(P["nb"] - 1, -1, -1):
            if P["colptr"][j + 1] - P["colptr"][j] > 1:
                depth[j] = depth[P["lrow"][P["colptr"][j] + 1]] + 1
        pairs = np.stack([ids, np.full(ids.size, ids[P["perm"][int(np.argmax(depth))]])], axis=1)
    call = (lambda: G.marginal_covariances(1e-2)) if what == "marginals" else (lambda: G.covariances(pairs, 1e-2))
    ts = []
    for k in range(WARM + CALLS):
        t = time.perf_counter()
        call()
        ts.append(time.perf_counter() - t)
    st = G.covariance_stats()
    print(f"{which} {what}: wall median {1e3 * np.median(ts[WARM:]):.3f} ms over {CALLS} calls; {st}", flush=True)


def summarise(d, out):
    rows = []
    for path in sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)):
        tag = os.path.basename(path).replace("_kernel_trace.csv", "")
        by = {}
        for r in csv.DictReader(open(path)):
            by.setdefault(r["Kernel_Name"], []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
        for name, v in sorted(by.items()):
            v.sort()
            per_call = max(1, round(len(v) / (WARM + CALLS)))
            if len(v) > WARM * per_call:
                v = v[WARM * per_call:]
            # a kernel launched several times per call (bottom and top groups): the call's sum
            dur = np.array([sum(b - a for a, b in v[i:i + per_call]) for i in range(0, len(v) - per_call + 1, per_call)])
            rows.append((tag, name, len(v), per_call, int(np.median(dur)), int(dur.min()), int(dur.max())))
    with open(out, "w", newline="") as f:
        w = csv.writer(f, quoting=csv.QUOTE_NONNUMERIC)
        w.writerow(["Run", "Name", "Dispatches", "PerCall", "MedianNsPerCall", "MinNsPerCall", "MaxNsPerCall"])
        w.writerows(rows)
    for r in rows:
        print("%-18s %5d (%2d per call)  median %8.1f us  %s" % (r[0], r[2], r[3], r[4] / 1e3, r[1][:90]))


if __name__ == "__main__":
    if sys.argv[1] == "summarise":
        summarise(sys.argv[2], sys.argv[3])
    else:
        target(sys.argv[1], sys.argv[2])
