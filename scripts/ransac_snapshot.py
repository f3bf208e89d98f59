"""Everything the two batched RANSAC stages (PnpBatch, EssentialBatch) return, dumped so that two builds of the library
can be compared byte for byte: the check of a change that must leave their results alone.

    SIM3OPT_LIB=/path/to/libsim3opt.so python scripts/ransac_snapshot.py dump parent.npz
    python scripts/ransac_snapshot.py dump head.npz
    python scripts/ransac_snapshot.py compare parent.npz head.npz

dump solves tests/pnp_cases.SIZE_CASES and tests/essential_cases.SIZE_CASES (around 64 lanes, the 256-thread stride and
the LDS staging cap: the staged and the global path) as one batch each, with iterations in ITERATIONS -- one
hypothesis, and a full chunk and one more of each stage, so that the best carried from chunk to chunk and the partial
last chunk are both run.  Per setting: poses, models, masks and inlier counts, every summary field, every
debug_hypotheses field of every problem; and once per stage debug_score on the matrices the tests' scoring operator
is given (the restatement's hypotheses among them).
compare prints the first differing field with its problem and index, and a verdict line; exit status 1 if any differs.
dump needs a GPU; there is no fallback.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("SIM3OPT_PRELOAD_TORCH", "1")

ITERATIONS = (1, 16, 17, 100, 256, 257)


def stages():
    from sim3opt_amd import lib as L
    import essential_cases as EC
    import pnp_cases as PC
    return (("pnp", L.PnpBatch, PC, dict(min_points=4), PC.score_poses, ()),
            ("essential", L.EssentialBatch, EC, dict(min_points=6), EC.score_matrices, ("essentials",)))


def dump(out):
    res = {}
    for name, Batch, cases, opts, score_input, extra in stages():
        arrays = cases.batch_arrays(cases.SIZE_CASES)
        for H in ITERATIONS:
            b = Batch(iterations=H, **opts)
            b.set_problems(**arrays)
            key = f"{name}/iterations={H}/"
            res[key + "solved"] = np.array(b.solve())
            res[key + "poses"] = b.poses()
            res[key + "mask"], res[key + "n_inliers"] = b.inliers()
            for f in extra:
                res[key + f] = getattr(b, f)()
            for f, v in b.summary().items():
                res[key + "summary." + f] = v
            for k in range(len(cases.SIZE_CASES)):
                for f, v in b.debug_hypotheses(k).items():
                    res[key + f"problem={k}/hypotheses." + f] = v
            b.close()
        b = Batch(**opts)
        b.set_problems(**arrays)
        given = np.stack([score_input(*c) for c in cases.SIZE_CASES])
        res[name + "/score.count"], res[name + "/score.cost"] = b.debug_score(given)
        b.close()
    np.savez(out, **res)
    print(f"{out}: {len(res)} arrays, {sum(v.nbytes for v in res.values())} bytes")
    return 0


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    if sorted(a.files) != sorted(b.files):
        print(f"DIFFERENT: the dumps hold different fields: {sorted(set(a.files) ^ set(b.files))[:5]} ...")
        return 1
    nbytes = 0
    for f in a.files:
        x, y = a[f], b[f]
        if x.shape != y.shape or x.dtype != y.dtype:
            print(f"DIFFERENT: {f}: {x.dtype}{x.shape} against {y.dtype}{y.shape}")
            return 1
        if x.tobytes() != y.tobytes():
            bad = np.flatnonzero(x.reshape(-1).view(np.uint8) != y.reshape(-1).view(np.uint8))[0] // x.dtype.itemsize
            idx = np.unravel_index(bad, x.shape) if x.shape else ()
            print(f"DIFFERENT: {f}{list(map(int, idx))}: {x.reshape(-1)[bad]!r} against {y.reshape(-1)[bad]!r}")
            return 1
        nbytes += x.nbytes
    print(f"IDENTICAL: {len(a.files)} arrays, {nbytes} bytes, every byte equal ({os.path.basename(pa)} against "
          f"{os.path.basename(pb)}; iterations {list(ITERATIONS)})")
    return 0


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="mode", required=True)
    d = sub.add_parser("dump")
    d.add_argument("out")
    c = sub.add_parser("compare")
    c.add_argument("a")
    c.add_argument("b")
    args = ap.parse_args()
    return dump(args.out) if args.mode == "dump" else compare(args.a, args.b)


if __name__ == "__main__":
    sys.exit(main())
