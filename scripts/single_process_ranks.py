"""What the in-process transport costs: config 3 (100k vertices / 1M edges, fix_small_angle_b = 1) on ONE GPU as
   one rank,
   Graph.set_devices([0] * N)            -- the library's rank threads, peer-memory collectives (comm_local.hip),
   tests/dist_helpers.ThreadGroup(N)     -- thread-ranks over the host-staged callback transport (the baseline),
for N = 2, 4, 8: LM iterations per second of optimize(20) after 5 warm-up iterations (median of 5 repetitions from the
same start) and, from a further run with time_kernels = 1, milliseconds and count per kind of collective (rank 0).
Ranks that share a device do not speed anything up over one rank: the figures are costs of the transport, not a
scaling curve.
Usage: python scripts/single_process_ranks.py [--sizes 2,4,8] [--reps 5] [--steps 20] [--warmup 5] [--vertices V --edges E]
   -> $OUT/single_process_ranks.json   (OUT defaults to <repo>/profiles)"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dist_helpers as H  # noqa: E402
from sim3opt_amd import lib as L, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="2,4,8")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--vertices", type=int, default=100000)
ap.add_argument("--edges", type=int, default=1000000)
A = ap.parse_args()
OUT = os.environ.get("OUT", os.path.join(ROOT, "profiles"))
synth.DRIFT_TARGET = 0.05
if A.vertices == 100000:
    g = synth.manhattan(A.vertices, A.edges)
else:
    g = synth.manhattan(A.vertices, A.edges, dims=(int(round((A.vertices / 10) ** 0.5)),) * 2 + (10,))
OPTS = dict(fix_small_angle_b=1)


def measure(G):
    """on every rank of a variant alike (the calls are collective)"""
    rates, last = [], None
    for _ in range(A.reps):
        G.set_vertices(g["states"])
        G.optimize(A.warmup)
        t0 = time.perf_counter()
        n = G.optimize(A.steps)
        dt = time.perf_counter() - t0
        rates.append(n / dt)
        last = G.stats()
    G.set_options(time_kernels=1)
    G.set_vertices(g["states"])
    G.optimize(A.warmup)
    G.kernel_times(reset=True)
    n = G.optimize(A.steps)
    ct = G.comm_times()
    G.set_options(time_kernels=0)
    return dict(lm_iterations_per_s=statistics.median(rates), all_repetitions=rates, lm_iterations=int(n),
                pcg_iterations=int(sum(s.pcg_iters for s in last)), chi2_after=float(last[-1].chi2_after),
                collectives={k: dict(ms=float(ct["ms_" + k]), count=int(ct["n_" + k]), bytes=int(ct["bytes_" + k]))
                             for k in ("allreduce", "allgather", "exchange")})


def fill(G):
    G.add_vertices(g["states"], g["fixed"])
    G.add_edges(g["v0"], g["v1"], g["meas"])


def one_rank():
    G = L.Graph(device=0, **OPTS)
    fill(G)
    G.initialize()
    out = measure(G)
    G.close()
    return out


def in_process(n):
    G = L.Graph(**OPTS)
    fill(G)
    G.set_devices([0] * n)
    G.initialize()
    out = measure(G)
    G.close()
    return out


def thread_ranks(n):
    tg = H.ThreadGroup(n, timeout=1800.0)

    def body(rank):
        G = L.Graph(device=0, **OPTS)
        fill(G)
        tg.attach(G, rank)
        G.initialize()
        out = measure(G)
        G.close()
        return out

    return tg.run(body)[0]


res = dict(vertices=A.vertices, edges=A.edges, steps=A.steps, warmup=A.warmup, repetitions=A.reps,
           note="all ranks share one GPU: costs of the transport, not a scaling curve", one_rank=one_rank(),
           set_devices={}, thread_group={})
print(json.dumps(dict(one_rank=res["one_rank"]["lm_iterations_per_s"])), flush=True)
os.makedirs(OUT, exist_ok=True)


def save():
    with open(os.path.join(OUT, "single_process_ranks.json"), "w") as f:
        json.dump(res, f, indent=1)


for n in [int(x) for x in A.sizes.split(",")]:
    res["set_devices"][str(n)] = in_process(n)
    print(json.dumps({"ranks": n, "set_devices": res["set_devices"][str(n)]["lm_iterations_per_s"]}), flush=True)
    save()
    res["thread_group"][str(n)] = thread_ranks(n)
    print(json.dumps({"ranks": n, "thread_group": res["thread_group"][str(n)]["lm_iterations_per_s"]}), flush=True)
    # same partition, same reductions: the two transports must land on the same bits
    res["set_devices"][str(n)]["same_chi2_as_thread_group"] = \
        res["set_devices"][str(n)]["chi2_after"] == res["thread_group"][str(n)]["chi2_after"]
    save()
print("wrote", os.path.join(OUT, "single_process_ranks.json"))
