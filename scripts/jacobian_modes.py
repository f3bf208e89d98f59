"""Numeric against closed-form Jacobians (options.jacobians 0 / 1) on bench.py's headline graph.

    python scripts/jacobian_modes.py [--out FILE]            # the A/B record (JSON)
    python scripts/jacobian_modes.py --linearize-only N      # N linearisations per mode, for rocprofv3

The graph is bench.py's (synth.manhattan(100000, 1000000), drift 0.05, fix_small_angle_b = 1, pcg_rel_tol 1e-8,
time_kernels 1).  One handle; the mode is switched with set_options between legs, and every leg starts from the
initial estimates:
  window   : bench's window -- 5 warm-up LM iterations, estimates put back, 20 timed LM iterations -- for numeric
             (fd_delta = 1e-9, bench's setting) and analytic, alternately A/B/A/B in this process
  optimize : optimize(100) to g2o's Terminate rule for both modes: iterations, trials, wall time, final chi2
Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of --linearize-only (k_linearize_*).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = {"numeric": dict(jacobians=0, fd_delta=1e-9), "analytic": dict(jacobians=1)}


def run_lm(G, k):
    done, stats = 0, []
    while done < k:
        it = G.optimize(k - done)
        if it <= 0:
            raise SystemExit("optimize returned %d" % it)
        done += it
        stats += G.stats()
    return stats


def window(G, states, torch, warmup=5, steps=20):
    G.set_vertices(states)
    run_lm(G, warmup)
    G.set_vertices(states)
    G.kernel_times(reset=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    st = run_lm(G, steps)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    kt = G.kernel_times()
    return {"lm_iters_per_s": steps / dt, "seconds": dt,
            "trials_per_iter": sum(s.trials for s in st) / steps,
            "pcg_iters": int(sum(s.pcg_iters for s in st)),
            "n_linearize": int(kt.n_linearize),
            "ms_per_linearize": kt.ms_linearize / max(kt.n_linearize, 1),
            "chi2_final": st[-1].chi2_after, "trials": [int(s.trials) for s in st]}


def optimize100(G, states, torch):
    G.set_vertices(states)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = G.optimize(100)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    st = G.stats()
    return {"iterations": int(n), "seconds": dt, "trials": int(sum(s.trials for s in st)),
            "pcg_iters": int(sum(s.pcg_iters for s in st)), "chi2_final": st[-1].chi2_after,
            "terminated_by": "iteration limit" if n >= 100 else "Terminate rule (ten rejected trials / rho == 0)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vertices", type=int, default=100000)
    ap.add_argument("--edges", type=int, default=1000000)
    ap.add_argument("--linearize-only", type=int, default=0)
    ap.add_argument("--no-optimize100", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch  # (its HIP runtime first: sim3opt_amd.lib.load)
    from sim3opt_amd import lib as L, synth

    synth.DRIFT_TARGET = 0.05
    g = synth.manhattan(args.vertices, args.edges)
    G = L.Graph(device=0, time_kernels=1, pcg_rel_tol=1e-8, fix_small_angle_b=1, preconditioner=-1)
    G.add_vertices(g["states"], g["fixed"])
    G.add_edges(g["v0"], g["v1"], g["meas"])
    G.initialize()
    if args.linearize_only:
        for mode, o in MODES.items():
            G.set_options(**o)
            for _ in range(args.linearize_only):
                G.linearize()
            print(mode, "linearised", args.linearize_only, "times", flush=True)
        return
    rec = {"graph": {"vertices": args.vertices, "edges": args.edges, "fix_small_angle_b": 1, "pcg_rel_tol": 1e-8,
                     "preconditioner_in_use": G.preconditioner_in_use()},
           "window": {"warmup": 5, "steps": 20, "order": [], "numeric": [], "analytic": []}}
    for mode in ("numeric", "analytic", "numeric", "analytic"):
        G.set_options(**MODES[mode])
        w = window(G, g["states"], torch)
        rec["window"]["order"].append(mode)
        rec["window"][mode].append(w)
        print(mode, json.dumps({k: v for k, v in w.items() if k != "trials"}), flush=True)
    if not args.no_optimize100:
        rec["optimize100"] = {}
        for mode in ("numeric", "analytic"):
            G.set_options(**MODES[mode])
            rec["optimize100"][mode] = optimize100(G, g["states"], torch)
            print(mode, "optimize(100)", json.dumps(rec["optimize100"][mode]), flush=True)
    G.close()
    txt = json.dumps(rec, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
