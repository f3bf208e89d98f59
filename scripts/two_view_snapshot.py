"""Digests of everything TwoViewBatch.optimize() returns on the tests' cases, so that two builds of the library can be
compared: the check of a change that must leave the batched two-view refinement's results alone
(profiles/two_view_readout_parity.md).

    SIM3OPT_LIB=/path/to/libsim3opt.so python scripts/two_view_snapshot.py > parent.txt
    python scripts/two_view_snapshot.py > head.txt
    diff parent.txt head.txt

One line per run and field -- cameras, points, stats, summary (iterations, activeChi2 before / after, outlier edges,
lambda_0) and edge_chi2 -- with the SHA-256 of its bytes, and a last line with the digest of all of them.  The runs:
tests/two_view_cases.WHOLE_RUN_CASES under its four OPTION_SETS, and MANY_CASES x 10 (300 workgroups).
Needs a GPU; there is no fallback.
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("SIM3OPT_PRELOAD_TORCH", "1")


def fields(b):
    n = b.dims()[0]
    c0, c1 = b.cameras()
    stats = np.array([[s[k] for k in ("chi2_before", "chi2_after", "lambda_", "rho", "trials")]
                      for p in range(n) for s in b.stats(p)])
    chi = b.chi2()
    summary = np.stack([b.num_iterations().astype(np.float64), chi["active_before"], chi["active_after"],
                        chi["n_outlier_edges"].astype(np.float64), b.lambda_init()], axis=1)
    return dict(cam0=c0, cam1=c1, points=b.points(), stats=stats, summary=summary, edge_chi2=chi["edge_chi2"])


def main():
    from sim3opt_amd import lib as L
    import two_view_cases as TC
    # a build older than this tree's lib.py may lack exports this script never calls
    L.load(tolerant=bool(os.environ.get("SIM3OPT_LIB")))
    for name in L.MISSING_SYMBOLS:
        print(f"not in this build, not bound: {name}", file=sys.stderr)
    runs = [("whole_run " + (",".join(f"{k}={v}" for k, v in o.items()) or "defaults"), TC.WHOLE_RUN_CASES, o)
            for o in TC.OPTION_SETS] + [("many x 10", TC.MANY_CASES * 10, {})]
    total = hashlib.sha256()
    print(f"library: {os.path.basename(os.path.dirname(L.LIB_PATH))}/{os.path.basename(L.LIB_PATH)}")
    for name, cases, opts in runs:
        b = L.TwoViewBatch(**opts)
        b.set_problems(**TC.batch_arrays(cases))
        assert b.optimize() == len(cases)
        for f, v in fields(b).items():
            raw = np.ascontiguousarray(v).tobytes()
            total.update(raw)
            print(f"{name:32s} {f:10s} {len(raw):8d} bytes  {hashlib.sha256(raw).hexdigest()[:32]}")
        b.close()
    print(f"all: {total.hexdigest()}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
