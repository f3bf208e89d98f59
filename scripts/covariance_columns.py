"""The gate of candidate edges and one block column by columns of the inverse (options.cov_solver = 1), timed on an
MI355X: config 3 (Manhattan 100k / 1M, the benchmark's graph and options) after optimize(10), gate_edges of 1, 8 and 64
seeded non-adjacent candidates at lambda = 0 and 1e-2, and one full block column on Manhattan 3000 / 30000.

    python scripts/covariance_columns.py [OUT.json]        (default profiles/covariance_columns.json)

Per call: wall time (host clock around the call, which ends in a device synchronise; median of CALLS after WARM
warm-up calls), vertices and columns solved, PCG iterations per column, batches, refinement rounds, the worst true
residual, and whether cov_rel_tol was reached (a call that fails reports the residual it got to).  For scale, the
same number of sequential sim3opt_solve calls (one system each, right-hand side b) is timed next to each gate."""
import json, os, socket, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sim3opt_amd import lib as L, synth
WARM, CALLS = 1, 3


def graph(g, **opts):
    G = L.Graph(fix_small_angle_b=1, cov_solver=1, **opts)
    G.add_vertices(g["states"], g["fixed"])
    G.add_edges(g["v0"], g["v1"], g["meas"])
    G.initialize()
    return G


def timed(call):
    ts, err = [], None
    for _ in range(WARM + CALLS):
        t = time.perf_counter()
        try:
            call()
        except L.Sim3OptError as e:
            err = str(e)
        ts.append(time.perf_counter() - t)
    return 1e3 * float(np.median(ts[WARM:])), err


def record(G, what, lam, call):
    ms, err = timed(call)
    st = G.covariance_columns_stats()
    cols = max(st["columns"], 1)
    row = dict(what=what, lam=lam, wall_ms=ms, vertices=st["vertices"], columns=st["columns"],
               pcg_iters=st["pcg_iters"], pcg_iters_per_column=st["pcg_iters"] / cols, batches=st["batches"],
               refinement_rounds=st["refinements"], worst_rel_residual=st["max_rel_residual"],
               cov_rel_tol=st["cov_rel_tol"], reached=err is None, error=err)
    print(json.dumps(row), flush=True)
    return row


def candidates(g, n, seed=41):
    """n seeded pairs of free vertices no edge joins, the measurement an identity-like closure"""
    rng = np.random.default_rng(seed)
    V = g["states"].shape[0]
    joined = set(zip(g["v0"].tolist(), g["v1"].tolist())) | set(zip(g["v1"].tolist(), g["v0"].tolist()))
    free = np.flatnonzero(np.asarray(g["fixed"]) == 0)
    out = []
    while len(out) < n:
        a, b = (int(x) for x in rng.choice(free, 2))
        if a != b and (a, b) not in joined and (a, b) not in out:
            out.append((a, b))
    v0, v1 = (np.array(x, dtype=np.int32) for x in zip(*out))
    meas = np.tile(np.array([0, 0, 0, 1, 0.5, 0, 0, 1.0]), (n, 1))
    return v0, v1, meas


def main(out_path):
    rows = []
    g = synth.manhattan()  # config 3
    # the benchmark's options (central differences, delta = 1e-9), then the closed-form Jacobians at lambda = 0: H from
    # delta = 1e-9 differences carries eps |e| / delta of noise per entry and may not be positive definite there
    for tag, opts, cases in (("numeric Jacobians, delta = 1e-9", {}, [(l, n) for l in (0.0, 1e-2) for n in (1, 8, 64)]),
                             ("analytic Jacobians", dict(jacobians=1), [(0.0, 1), (0.0, 8)])):
        G = graph(g, **opts)
        assert G.linear_solver_in_use() == 0
        G.optimize(10)
        for lam, n in cases:
            v0, v1, meas = candidates(g, n)
            r = record(G, f"config 3, {tag}: gate_edges of {n}", lam, lambda: G.gate_edges(v0, v1, meas, lam=lam))
            if n == 1:  # the same number of one-system solves, sequentially (the parent commit's only solve)
                G.linearize()
                k = 14
                ms, err = timed(lambda: [G.solve(lam) for _ in range(k)])
                r["sequential_solves"] = k
                r["sequential_solves_ms"] = ms
                r["sequential_solves_error"] = err
                try:
                    r["sequential_solve_iters"] = G.solve(lam)[1]
                except L.Sim3OptError:
                    r["sequential_solve_iters"] = None
                print(json.dumps({k2: r[k2] for k2 in r if k2.startswith("sequential")}), flush=True)
            rows.append(r)
        G.close()
    g = synth.manhattan(3000, 30000, dims=(17, 17, 10))
    G = graph(g, fd_delta=1e-6, linear_solver=0, preconditioner=2)
    free = np.flatnonzero(np.asarray(g["fixed"]) == 0).astype(np.int32)
    pairs = np.stack([free, np.full(free.size, free[free.size // 2])], axis=1)
    for lam in (0.0, 1e-2):
        rows.append(record(G, "Manhattan 3000 / 30000: one block column", lam, lambda: G.covariances(pairs, lam)))
    G.close()
    doc = dict(box=socket.gethostname(), warmup_calls=WARM, timed_calls=CALLS, statistic="median wall ms per call", rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "covariance_columns.json"))
