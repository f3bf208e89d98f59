"""Bit parity of a dogleg run between two builds (profiles/dogleg_readout_parity.md): 11 dogleg iterations on
chain_graph() of tests/test_gpu_algorithms.py with the exact and the PCG solver, run by the sim3opt_amd package found
under a given tree -- a built checkout of the commit to compare with, or `.` -- and written as hex floats.

    python scripts/dogleg_parity.py <tree> out.json          one side (a process of its own per side)
    python scripts/dogleg_parity.py compare a.json b.json    one table row per solver, then PARITY OK / FAILED
"""
import hashlib
import json
import sys


def run(root, out):
    import os
    root = os.path.abspath(root)
    sys.path.insert(0, root)
    import numpy as np
    from sim3opt_amd import lib as L, synth
    assert L.__file__.startswith(root), L.__file__
    synth.DRIFT_TARGET = 0.6
    g = synth.chain_loop(240, 720, seed_graph=7101, seed_noise=7102, min_gap=5)
    rng = np.random.default_rng(31)
    M = rng.standard_normal((len(g["v0"]), 7, 7)) * 0.3
    g["info"] = np.einsum("kij,klj->kil", M, M) + np.eye(7)
    res = {}
    solvers = {"exact": dict(linear_solver=1),
               "pcg": dict(linear_solver=0, preconditioner=0, pcg_rel_tol=1e-12, pcg_max_iters=20000)}
    for name, so in solvers.items():
        G = L.Graph(algorithm=L.ALGORITHM_DOGLEG, dl_delta_init=0.1, fix_small_angle_b=1, fd_delta=1e-4, **so)
        G.add_vertices(g["states"], g["fixed"])
        G.add_edges(g["v0"], g["v1"], g["meas"], info=g["info"])
        G.initialize()
        n = G.optimize(11)
        st, ts = G.stats(), G.trust_region_stats()
        rows = []
        for s, t in zip(st, ts):
            rows.append(dict(chi2_before=float(s.chi2_before).hex(), chi2_after=float(s.chi2_after).hex(),
                             trials=int(s.trials), step=int(t.step), delta_before=float(t.delta_before).hex(),
                             delta_after=float(t.delta_after).hex(), alpha=float(t.alpha).hex(),
                             norm_sd=float(t.norm_sd).hex(), norm_gn=float(t.norm_gn).hex(),
                             norm_dl=float(t.norm_dl).hex()))
        v = np.ascontiguousarray(G.get_vertices())
        res[name] = dict(iterations=int(n), rows=rows, estimates_sha256=hashlib.sha256(v.tobytes()).hexdigest(),
                         chi2_final=float(st[-1].chi2_after))
        G.close()
    json.dump(res, open(out, "w"), indent=1)
    print("wrote", out)


def compare(a, b):
    A, B = json.load(open(a)), json.load(open(b))
    ok = True
    for name in A:
        ra, rb = A[name], B[name]
        same_est = ra["estimates_sha256"] == rb["estimates_sha256"]
        diff = [(k, f) for k, (x, y) in enumerate(zip(ra["rows"], rb["rows"])) for f in x if x[f] != y[f]]
        same = same_est and not diff and ra["iterations"] == rb["iterations"] == 11
        ok = ok and same
        print(f"| {name} | {ra['iterations']} / {rb['iterations']} | {ra['estimates_sha256'][:16]} | "
              f"{rb['estimates_sha256'][:16]} | {sum(len(x) for x in ra['rows'])} | {len(diff)} | {ra['chi2_final']!r} | "
              f"{[r['step'] for r in ra['rows']]} | {'equal' if same else 'DIFFERENT'} |")
    print("PARITY", "OK" if ok else "FAILED")
    return 0 if ok else 1


if __name__ == "__main__":
    if sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    run(sys.argv[1], sys.argv[2])
