"""Levenberg-Marquardt, Gauss-Newton and Powell's dogleg (options.algorithm 0 / 1 / 2) on optimize(100).

    python scripts/algorithms.py [--out FILE] [--skip-config3]

Graphs:
  config3 : bench.py's headline graph (synth.manhattan(100000, 1000000), drift 0.05, fix_small_angle_b = 1,
            pcg_rel_tol 1e-8, automatic preconditioner -- the multigrid PCG)
  kitti00 : the KITTI-00 one-loop graph of tests/golden/kitti00 (fix_small_angle_b = 1, automatic linear solver --
            the exact block Cholesky)
One handle per graph; the algorithm is switched with set_options between legs, every leg starts from the initial
estimates and is run twice (the first run warms up launches and caches; the second is recorded).  time_kernels = 1,
so every iteration records its device time split into linearisation, linear solve(s) (for dogleg: with the two SpMVs
and the dots of its model) and trial work (update + chi2).  Per leg: wall time, iterations, trials, PCG iterations
(exact path: linear solves), final chi2, how the run ended.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ALGS = {"lm": 0, "gauss_newton": 1, "dogleg": 2}


def leg(G, states, torch, L, alg, iters):
    G.set_options(algorithm=ALGS[alg])
    G.set_vertices(states)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    err = None
    try:
        n = G.optimize(iters)
    except L.Sim3OptError as e:  # g2o's Fail (a GN solve that failed): optimize() returned 0
        n, err = 0, str(e)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    st = G.stats()
    rec = {"iterations": int(n), "iterations_recorded": len(st), "seconds": dt,
           "trials": int(sum(s.trials for s in st)), "pcg_iters": int(sum(s.pcg_iters for s in st)),
           "pcg_capped": int(sum(s.pcg_capped for s in st)),
           "chi2_initial": st[0].chi2_before if st else None, "chi2_final": st[-1].chi2_after if st else None,
           "device_ms": {"linearize": sum(s.ms_linearize for s in st), "solve": sum(s.ms_solve for s in st),
                         "trials": sum(s.ms_update for s in st)}}
    if G.linear_solver_in_use() == 1:
        rec["linear_solves"] = rec["trials"] if alg == "lm" else len(st)  # (dogleg: plus damped re-solves, if any)
    if alg == "dogleg":
        tr = G.trust_region_stats()
        rec["steps"] = {name: sum(1 for t in tr if t.step == k) for k, name in ((1, "SD"), (2, "GN"), (3, "DL"))}
        rec["was_pd"] = bool(tr[-1].was_pd) if tr else None
        rec["delta_final"] = tr[-1].delta_after if tr else None
    if err:
        rec["ended"] = "Fail: " + err
    elif n < iters:
        rec["ended"] = "Terminate rule"
    else:
        rec["ended"] = "iteration limit"
    return rec


def run_graph(name, g, opts, torch, L, iters):
    G = L.Graph(device=0, time_kernels=1, **opts)
    G.add_vertices(g["states"], g["fixed"])
    G.add_edges(g["v0"], g["v1"], g["meas"])
    G.initialize()
    out = {"options": opts, "linear_solver_in_use": G.linear_solver_in_use(),
           "preconditioner_in_use": G.preconditioner_in_use()}
    for alg in ALGS:
        leg(G, g["states"], torch, L, alg, iters)  # warm-up
        out[alg] = leg(G, g["states"], torch, L, alg, iters)
        print(name, alg, json.dumps(out[alg]), flush=True)
    G.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--skip-config3", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch  # (its HIP runtime first: sim3opt_amd.lib.load)
    from sim3opt_amd import lib as L, synth
    import kitti_graph as K

    rec = {"optimize": args.iters, "device": torch.cuda.get_device_name(0)}
    rec["kitti00_one_loop"] = run_graph("kitti00", K.build_direct_graph(True), dict(fix_small_angle_b=1), torch, L,
                                        args.iters)
    if not args.skip_config3:
        synth.DRIFT_TARGET = 0.05
        g = synth.manhattan(100000, 1000000)
        rec["config3"] = run_graph("config3", g, dict(fix_small_angle_b=1, pcg_rel_tol=1e-8, preconditioner=-1),
                                   torch, L, args.iters)
    txt = json.dumps(rec, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
