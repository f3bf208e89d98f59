#!/usr/bin/env python3
"""bench.py -- LM iterations/s of the Sim(3) pose-graph hot path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

One "step" = one Levenberg-Marquardt iteration (chi2, per-edge residual + numeric Jacobians,
block-CSR assembly, preconditioned CG solve, oplus update, chi2 again, lambda policy) on
BASELINE.json configs[2]: the synthetic Manhattan-grid Sim(3) graph, 100k vertices / 1M edges,
inputs resident in HBM before the timed region.  N > 1: the same graph, block rows partitioned
across the ranks (strong scaling), RCCL all-gather of the PCG direction + fused scalar all-reduce.

A plain run sets up, warms up, times the K steps, writes --dump-outputs and prints rank 0's ONE
JSON line: the headline (metric, value, unit, higher_is_better, dtype, ms_per_step) and what the
timed steps measured anyway, among it
  roofline      dominant kernel (k_spmv: block-CSR SpMV of the PCG) against the 8 TB/s HBM peak,
                duration measured live with HIP events on the library's stream in the timed region
--full adds everything that takes runs of its own, after the timed region:
  roofline.box_stream / box_clocks   a bare stream of the block array and the clocks under load
  block_jacobi_pcg, reference_arithmetic, optimize100_to_terminate   comparison legs (--main-only
                skips them)
  cpu_baseline  the CPU oracle (port of the reference's g2o configuration) timed on rank 0 on the
                phases of the same workload a CPU can run at full size; plus the KITTI-00 table
                (reference configuration) where both sides run the whole optimisation and ba_demo
                (--no-cpu-baseline skips the three)
  partition     at N > 1, the row partition the collectives serve
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E peak 8.0 TB/s


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # default window: LM iterations 1..8 from the initial state, the ones in which chi2 still moves;
    # from the 12th on LM sits at the noise floor of the numeric Jacobians and an "iteration" is up
    # to 10 rejected trials -- still measurable with --steps, but not the default headline
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--vertices", type=int, default=100000)
    ap.add_argument("--edges", type=int, default=1000000)
    ap.add_argument("--fix-small-angle-b", type=int, default=1,
                    help="1 (default) = exact small-angle B coefficient: LM converges on this graph; "
                         "0 = reference arithmetic as written (sim3_rv.h:166): LM stalls at "
                         "lambda ~1e8, reported separately as reference_arithmetic")
    ap.add_argument("--pcg-rel-tol", type=float, default=1e-8)
    ap.add_argument("--preconditioner", type=int, default=-1,
                    help="-1 automatic (multigrid on this workload at 1 GPU), 0 block-Jacobi, 2 multigrid")
    ap.add_argument("--time-kernels", type=int, default=1,
                    help="1: HIP-event pair around every SpMV launch of the PCG (roofline figure; "
                         "disables hipGraph replay), 0: untimed launches")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also run what takes runs of its own: the box's bare stream "
                         "and clocks (roofline), the comparison legs, the CPU baselines and the N > 1 "
                         "partition figures; a plain run does only what the headline needs")
    ap.add_argument("--main-only", action="store_true",
                    help="with --full: skip the comparison legs (block-Jacobi PCG, reference arithmetic, "
                         "optimize(100))")
    ap.add_argument("--no-cpu-baseline", action="store_true",
                    help="with --full: skip the CPU baselines (cpu_baseline, KITTI-00 table, ba_demo)")
    ap.add_argument("--transport", choices=["rccl", "gloo"], default="rccl",
                    help="multi-rank collectives: rccl (default; ncclAllReduce / grouped ncclBroadcast "
                         "on the library's stream) or gloo (host-staged callbacks; lets N ranks share "
                         "one GPU for dry runs)")
    ap.add_argument("--cpu-sample-vertices", type=int, default=1000)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one returned to a caller (the vertex "
                         "estimates, chi2 and lambda) as DIR/<name>.npy, float64, at most 64 MB in all")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


DUMP_MAX_BYTES = 64_000_000


def dump_outputs(directory, G, stats):
    """What the timed path handed its caller after the last timed step: every vertex estimate
    (sim3opt_get_vertices, n x 8: qx qy qz qw tx ty tz s) and that step's chi2 before /
    after and lambda.  Above the size cap a fixed, seeded sample of rows is written together with
    its row indices, so two builds given the same arguments can be compared output for output."""
    os.makedirs(directory, exist_ok=True)
    states = G.get_vertices()
    last = stats[-1]
    out = {"lm_last_step": np.array([last.chi2_before, last.chi2_after, last.lambda_], dtype=np.float64)}
    max_rows = (DUMP_MAX_BYTES - 4096) // (states.shape[1] * 8 + 8)
    if states.shape[0] > max_rows:
        rows = np.sort(np.random.default_rng(20240613).choice(states.shape[0], max_rows, replace=False))
        out["vertices_sample_rows"] = rows.astype(np.float64)
        out["vertices_sample"] = states[rows]
    else:
        out["vertices"] = states
    for name, a in out.items():
        np.save(os.path.join(directory, name + ".npy"), np.ascontiguousarray(a, dtype=np.float64))


def cpu_baseline(args, g, gpu_ms_linearize, gpu_value, threads=1):
    """The CPU oracle (restatement of the reference's g2o configuration, single thread like the
    reference: no OpenMP in its build, CMakeLists.txt:17-18) on the SAME graph the GPU just ran:
    the phases a CPU can run at full size in bounded time -- numeric-Jacobian linearisation of every
    edge (EdgeSim3::linearizeOplus) and one chi2 evaluation.  The exact sparse Cholesky of the
    100k/1M Manhattan graph is out of reach (fill), so the CPU's linear solve is left out ENTIRELY:
    `value` is an upper bound on the CPU's LM iterations/s and the quoted speed-up a lower bound.
    What the solve costs on a graph small enough to factor is reported under `solve_sample`."""
    from oracle import oracle as O
    o = O.default_options(fix_small_angle_b=args.fix_small_angle_b, threads=threads)
    G = O.Graph(g["states"], g["fixed"], g["v0"], g["v1"], g["meas"])
    t0 = time.perf_counter()
    chi = G.chi2(o)
    t_chi = time.perf_counter() - t0
    t0 = time.perf_counter()
    G.jacobians(o)
    t_lin = time.perf_counter() - t0
    # the same two phases with every core the box gives this process (OpenMP over edges)
    # (a one-GPU box of the pool gives a job 16 CPUs although it shows the whole host's 256)
    ncores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    ncores = min(ncores, 16)
    all_cores = None
    if ncores > threads:
        oa = O.default_options(fix_small_angle_b=args.fix_small_angle_b, threads=ncores)
        t0 = time.perf_counter()
        G.chi2(oa)
        ta_chi = time.perf_counter() - t0
        t0 = time.perf_counter()
        G.jacobians(oa)
        ta_lin = time.perf_counter() - t0
        all_cores = {"cores": ncores, "seconds": {"linearize": ta_lin, "chi2": ta_chi},
                     "value": 1.0 / (ta_lin + ta_chi), "unit": "LM iter/s (upper bound, solve excluded)",
                     "speedup_lm_iters_lower_bound": gpu_value * (ta_lin + ta_chi)}
    # solve phase: the largest sample the oracle's LDL^T factors in about ten seconds
    from sim3opt_amd import lib as L, synth
    Vs = args.cpu_sample_vertices
    side = max(4, int(round((Vs / 10.0) ** 0.5)))
    gs = synth.manhattan(Vs, 10 * Vs, dims=(side, side, 10), per_cell=4)
    Gs = O.Graph(gs["states"], gs["fixed"], gs["v0"], gs["v1"], gs["meas"])
    it, tr = Gs.optimize(2, o)
    solves = sum(t.trials for t in tr)
    t_solve = sum(t.t_solve for t in tr) / max(solves, 1)
    lnz = int(O.lib().or_last_lnz())
    # is the oracle's ordering a strawman?  fill of a nested-dissection order of the same sample
    P = L.Graph()
    P.add_vertices(gs["states"], gs["fixed"])
    P.add_edges(gs["v0"], gs["v1"], gs["meas"])
    nd = P.direct_plan(max_pairs=200_000_000)
    P.close()
    value = 1.0 / (t_lin + t_chi)
    return {
        "value": value, "unit": "LM iter/s", "cores": threads, "kind": "port",
        "sample": (f"configs[2] itself, {args.vertices} vertices / {args.edges} edges, full size: one "
                   f"numeric-Jacobian linearisation of all edges ({t_lin:.2f} s) + one chi2 evaluation "
                   f"({t_chi:.2f} s), {threads} thread; the CPU's sparse Cholesky is EXCLUDED (fill makes "
                   f"it impractical at this size), so value is an upper bound on the CPU rate"),
        "seconds": {"linearize": t_lin, "chi2": t_chi}, "chi2": chi,
        "gpu_same_phase_ms": {"linearize_plus_chi2": gpu_ms_linearize},
        "speedup_linearize_phase": (t_lin + t_chi) / (gpu_ms_linearize * 1e-3) if gpu_ms_linearize else None,
        "speedup_lm_iters_lower_bound": gpu_value / value,
        "all_cores": all_cores,
        "solve_sample": {
            "graph": f"Manhattan graph of the same generator, {Vs} vertices / {10 * Vs} edges",
            "seconds_per_factor_and_solve": t_solve, "solves": solves,
            "fill_nonzeros_min_degree": lnz,
            "fill_nonzeros_nested_dissection": int(nd["nL"]) * 49,
            "note": "the oracle's block-minimum-degree fill against a nested-dissection order of the "
                    "same sample (sim3opt_direct_plan): the CPU factorisation is not handicapped by "
                    "its ordering"},
    }


def solver_options(G):
    o = G.options()
    names = ("amg_cycle", "amg_passes", "amg_additive", "amg_fp32", "amg_pivot", "amg_coarsest", "adaptive_prec",
             "row_order", "halo_exchange", "span_grid", "amg_shard_rows", "amg_virtual_ranks", "pcg_batch",
             "amg_omega", "amg_over", "pcg_check_every", "pcg_graph", "pcg_max_iters")
    out = {}
    for n in names:
        v = getattr(o, n)
        out[n] = list(v) if hasattr(v, "__len__") else v
    return out


def optimize100_leg(args, g, device):
    """The reference's own call on the benchmark graph: initializeOptimization(); optimize(100)
    (kitti_surf.cpp:674-675) from the initial state until g2o's Terminate rule (ten rejected trials,
    rho == 0 or a non-finite lambda) or 100 iterations.  Not part of `value`."""
    import torch
    from sim3opt_amd import lib as L
    G = L.Graph(device=device, pcg_rel_tol=args.pcg_rel_tol, fix_small_angle_b=args.fix_small_angle_b,
                preconditioner=args.preconditioner)
    G.add_vertices(g["states"], g["fixed"])
    G.add_edges(g["v0"], g["v1"], g["meas"])
    G.initialize()
    chi0 = G.chi2()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = G.optimize(100)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    st = G.stats()
    out = {"call": "optimize(100), kitti_surf.cpp:675", "iterations": int(n), "seconds": dt,
           "lm_iters_per_s": n / dt if dt > 0 else None,
           "terminated_by": ("iteration limit" if n >= 100 else "g2o Terminate rule (ten rejected trials / rho == 0)"),
           "trials": int(sum(int(s.trials) for s in st)), "pcg_iterations": int(sum(int(s.pcg_iters) for s in st)),
           "unconverged_solves": int(sum(int(s.pcg_capped) for s in st)),
           "chi2_initial": chi0, "chi2_final": st[-1].chi2_after if st else chi0,
           "chi2_after_10": st[9].chi2_after if len(st) > 9 else None,
           "lm_trials": [int(s.trials) for s in st]}
    G.close()
    return out


def kitti_table(device):
    """BASELINE.json configs[0] (and its all-loops variant) in the reference's OWN configuration
    (delta = 1e-9, B as written, optimize(100), kitti_surf.cpp:674-675): both sides actually run."""
    from oracle import oracle as O
    from sim3opt_amd import lib as L, synth
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import kitti_graph as K
    out = {}
    for name, one in (("one_loop", True), ("all_118_loops", False)):
        g = K.build_direct_graph(one)
        G = L.Graph(device=device)
        G.add_vertices(g["states"], g["fixed"])
        G.add_edges(g["v0"], g["v1"], g["meas"])
        G.initialize()
        G.optimize(2)
        G.set_vertices(g["states"])
        t0 = time.perf_counter()
        n = G.optimize(100)
        t_gpu = time.perf_counter() - t0
        chi_gpu = G.stats()[-1].chi2_after
        OG = O.Graph(g["states"], g["fixed"], g["v0"], g["v1"], g["meas"])
        t0 = time.perf_counter()
        it, tr = OG.optimize(100)
        t_cpu = time.perf_counter() - t0
        out[name] = {"gpu_iters": n, "gpu_seconds": t_gpu, "gpu_chi2": chi_gpu,
                     "cpu_iters": it, "cpu_seconds": t_cpu, "cpu_chi2": tr[-1].chi2_after,
                     "cpu_cores": 1, "speedup": t_cpu / t_gpu,
                     "gpu_lm_iters_per_s": n / t_gpu, "cpu_lm_iters_per_s": it / t_cpu,
                     "rmse_gpu_vs_cpu_m": synth.rmse(G.get_vertices(), OG.states),
                     "linear_solver": "exact block Cholesky" if G.linear_solver_in_use() else "PCG"}
        G.close()
    # BASELINE.json configs[4] in the reference's meaning (kitti_surf.cpp:887-1047): scales from the
    # null vector (host), scale + translation LM with the rotations frozen (100 it), Sim(3) LM
    # warm-started from it (100 it); both sides start from the same scale initialisation.
    gt = np.loadtxt(os.path.join(K.FIXTURE, "gt_kf.txt"), comments="%")[:, [4, 8, 12]]
    for name, one in (("stepwise_one_loop", True), ("stepwise_all_118_loops", False)):
        g = K.build_direct_graph(one)
        G = L.Graph(device=device)
        G.add_vertices(g["states"], g["fixed"])
        G.add_edges(g["v0"], g["v1"], g["meas"])
        G.stepwise_scale_init()
        st0 = G.get_vertices().copy()
        t0 = time.perf_counter()
        G.set_options(dof_mask=0x78)
        G.initialize()
        n2 = max(G.optimize(100), 0)
        chi_st = G.stats()[-1].chi2_after if n2 else float("nan")
        G.set_options(dof_mask=127)
        n3 = max(G.optimize(100), 0)
        t_gpu = time.perf_counter() - t0
        chi_gpu = G.stats()[-1].chi2_after if n3 else float("nan")
        OG = O.Graph(st0, g["fixed"], g["v0"], g["v1"], g["meas"])
        t0 = time.perf_counter()
        i2, tr2 = OG.optimize(100, O.default_options(dof_mask=0x78))
        i3, tr3 = OG.optimize(100)
        t_cpu = time.perf_counter() - t0
        out[name] = {"gpu_iters": [n2, n3], "cpu_iters": [i2, i3], "gpu_seconds": t_gpu, "cpu_seconds": t_cpu,
                     "speedup": t_cpu / t_gpu, "cpu_cores": 1,
                     "scale_trans_chi2_gpu": chi_st, "scale_trans_chi2_cpu": tr2[-1].chi2_after if i2 > 0 else None,
                     "gpu_chi2": chi_gpu, "cpu_chi2": tr3[-1].chi2_after if i3 > 0 else None,
                     "rmse_gpu_vs_cpu_m": synth.rmse(G.get_vertices(), OG.states),
                     "rmse_vs_ground_truth_m": {"gpu": L.align_trajectory(synth.positions(G.get_vertices()), gt)[1],
                                                "cpu": L.align_trajectory(synth.positions(OG.states), gt)[1]}}
        G.close()
    return out


def ba_demo_leg(device, cpu=True):
    """the reference's ba_demo (bal_example.cpp:44-243, 5 LM iterations by default)
    on a synthetic problem of the KITTI-00 map's shape -- 771 cameras, 123 000 points, ~369 k
    observations (the real map is not in the repo) -- GPU path and numpy/scipy restatement side by side."""
    from sim3opt_amd import lib as L
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import gpu_ba_scale as S
    cams, pts, oc, op, uv = S.kitti_like()
    b = L.BundleAdjuster(device=device)
    b.set_problem(cams, pts, oc, op, uv)
    c0 = b.chi2()  # (includes the one-time structure build and upload)
    t0 = time.perf_counter()
    n = b.optimize(5)
    t_gpu = time.perf_counter() - t0
    st = b.stats()
    out = {"workload": "synthetic BA problem of the KITTI-00 map's shape", "cameras": len(cams), "points": len(pts),
           "observations": len(oc), "lm_iterations": n, "gpu_seconds": t_gpu, "chi2_initial": c0,
           "gpu_chi2": [s["chi2_after"] for s in st], "gpu_trials": [s["trials"] for s in st],
           "reduced_system": "exact block Cholesky" if all(s["pcg_iters"] == 0 for s in st) else "PCG"}
    if cpu:
        from oracle import ba_oracle as BO  # checker / baseline only
        P = BO.Problem(cams, pts, oc, op, uv)
        t0 = time.perf_counter()
        tr = P.optimize(5, schur=True)
        t_cpu = time.perf_counter() - t0
        out.update({"cpu_seconds": t_cpu, "cpu_cores": 1, "cpu_kind": "port (numpy/scipy, Schur complement)",
                    "cpu_chi2": [t["chi2"] for t in tr], "speedup": t_cpu / t_gpu,
                    "max_rel_chi2_diff": max(abs(s["chi2_after"] - t["chi2"]) / t["chi2"] for s, t in zip(st, tr))})
    b.close()
    return out


def main():
    args = parse()
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus and world > 1:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # launched without torch.distributed.run: start the N ranks ourselves (before anything here
        # has touched the GPU) and exit with their code -- never a silent 1-GPU number
        import subprocess
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
               f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1", "--master-port",
               str(29500 + os.getpid() % 2000), os.path.abspath(__file__)] + sys.argv[1:]
        raise SystemExit(subprocess.call(cmd))

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device (no CPU fallback exists)")
    if args.transport == "gloo" or os.environ.get("SIM3OPT_BENCH_SHARE_GPU"):
        local_rank = local_rank % torch.cuda.device_count()  # dry runs: several ranks on one GPU
    torch.cuda.set_device(local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.transport == "gloo":
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))

    from sim3opt_amd import build as B, lib as L, synth
    if rank == 0:
        B.build()  # one writer; the other ranks load the finished file
    if dist is not None:
        dist.barrier()

    # ---- workload (identical on every rank: same seeds) ----
    synth.DRIFT_TARGET = 0.05
    g = synth.manhattan(args.vertices, args.edges)
    G = L.Graph(device=local_rank, time_kernels=args.time_kernels, pcg_rel_tol=args.pcg_rel_tol,
                fix_small_angle_b=args.fix_small_angle_b, preconditioner=args.preconditioner)
    G.add_vertices(g["states"], g["fixed"])
    G.add_edges(g["v0"], g["v1"], g["meas"])
    transport_used = None
    if world > 1:
        gloo_group = None

        def _ar(arr, op):
            dist.all_reduce(torch.from_numpy(arr), group=gloo_group,
                            op=dist.ReduceOp.MAX if op == 1 else dist.ReduceOp.SUM)

        def _ag(arr, offs, rk):
            t = torch.from_numpy(arr)
            for r in range(len(offs) - 1):
                if offs[r + 1] > offs[r]:
                    dist.broadcast(t[int(offs[r]):int(offs[r + 1])], src=r, group=gloo_group)

        def _aa(send, soffs, recv, roffs, rk):
            ts, tr = torch.from_numpy(send), torch.from_numpy(recv)
            reqs = [dist.irecv(tr[int(roffs[p]):int(roffs[p + 1])], src=p, group=gloo_group)
                    for p in range(len(roffs) - 1) if roffs[p + 1] > roffs[p]]
            reqs += [dist.isend(ts[int(soffs[p]):int(soffs[p + 1])].clone(), dst=p, group=gloo_group)
                     for p in range(len(soffs) - 1) if soffs[p + 1] > soffs[p]]
            for q in reqs:
                q.wait()

        ok = 0
        if args.transport == "rccl":
            # the library builds its own RCCL communicator from an id broadcast over torch's group
            uid = np.zeros(128, dtype=np.uint8)
            if rank == 0 and L.load().sim3opt_comm_unique_id(uid.ctypes.data_as(L._up)) != L.OK:
                uid[:] = 0  # (an all-zero id tells every rank that rank 0 has none: nobody may block in init)
            t = torch.from_numpy(uid).cuda()
            dist.broadcast(t, 0)
            uid = np.ascontiguousarray(t.cpu().numpy())
            ok = 1 if uid.any() else 0
            if ok and L.load().sim3opt_comm_init(G._g, rank, world,
                                                 uid.ctypes.data_as(L._up)) != L.OK:
                sys.stderr.write("sim3opt_comm_init: " + L.load().sim3opt_last_error(G._g).decode() + "\n")
                ok = 0
            flag = torch.tensor([ok], dtype=torch.int32, device="cuda")
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)  # every rank must have its communicator
            ok = int(flag.item())
            transport_used = "rccl" if ok else None
        if not ok:
            # host-staged collectives over gloo: the dry-run transport, and the fallback should the
            # library's RCCL communicator not come up on some rank (same partitioned kernels)
            if args.transport != "gloo":
                gloo_group = dist.new_group(backend="gloo")
            G.comm_init_callbacks(rank, world, _ar, _ag, _aa)
            transport_used = "gloo"
    G.initialize()  # uploads everything to HBM
    chi2_0 = G.chi2()
    nb, nnzb = G.system_dims()

    def run(k):
        done = 0
        while done < k:
            it = G._L.sim3opt_optimize(G._g, k - done)
            if it <= 0:
                raise SystemExit("optimize failed: " + G._L.sim3opt_last_error(G._g).decode())
            done += it
        return G.stats()

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    if args.warmup > 0:
        # warm-up = W LM iterations (caches, hipGraph capture, hierarchy set-up), then the estimates
        # are put back: the K timed iterations are LM iterations 1..K from the initial state.  Timing
        # a second optimize() call on the warmed-up states instead would make `value` depend on luck:
        # like g2o, every optimize() call starts from lambda = tau * max|H_dd|, and with delta = 1e-9
        # Jacobians that maximum is an outlier entry (1.2e3 or 7.0e4 for states that differ by 1e-8)
        run(args.warmup)
        G.set_vertices(g["states"])
    G.kernel_times(reset=True)
    barrier()
    t0 = time.perf_counter()
    stats = []
    done = 0
    while done < args.steps:  # exactly K LM iterations
        it = G._L.sim3opt_optimize(G._g, args.steps - done)
        if it <= 0:
            raise SystemExit("optimize failed: " + G._L.sim3opt_last_error(G._g).decode())
        done += it
        stats += G.stats()
    barrier()
    dt = time.perf_counter() - t0
    if dist is not None:
        tt = torch.tensor([dt], dtype=torch.float64,
                          device="cpu" if args.transport == "gloo" else "cuda")
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
    kt = G.kernel_times()
    ct = G.comm_times() if world > 1 else None  # (before the chi2 below adds its own all-reduce)
    chi2_final = G.chi2()
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, G, stats)

    if rank == 0:
        K = args.steps
        # algorithmic bytes of one SpMV launch: blocks + column indices + row
        # pointers, the input vector read once, q written once; per rank when row-partitioned
        lo, hi = G.local_rows()  # rank 0's share (ranks are balanced by stored blocks)
        rows_local = hi - lo
        blocks_local = nnzb if world == 1 else (nnzb + world - 1) // world
        # (vectors: the input read once, q written once; with block-Jacobi / chain preconditioning the
        # SpMV also reads r for the fused r.z reduction -- with the multigrid cycle r.z comes from the
        # cycle's last pass and the SpMV does not load r)
        n_vec = 2 if G.preconditioner_in_use() == 2 else 3
        spmv_bytes = blocks_local * (392 + 4) + (rows_local + 1) * 4 + n_vec * 7 * rows_local * 8
        # HBM bytes per SpMV launch from the last rocprofv3 --pmc collection (separate passes;
        # TCC_EA0_RDREQ x 128 B + WRITE_SIZE, gfx950 correction applied): profiles/r4_pmc_spmv.json
        traffic = None
        try:
            if world == 1 and args.vertices == 100000 and args.edges == 1000000:
                pm = json.load(open(os.path.join(ROOT, "profiles", "r4_pmc_spmv.json")))
                traffic = pm["hbm_read_bytes_corrected"] + pm["hbm_write_bytes"]
        except Exception:
            traffic = None
        prec_name = {0: "block-Jacobi", 1: "chain-segment",
                     2: "aggregation-multigrid" + ("; solves whose damping is of the order of the diagonal of H "
                                                   "start with block-Jacobi (same tolerance)"
                                                   if args.preconditioner < 0 else "")}[
            G.preconditioner_in_use()]
        roof = None
        if kt.n_spmv > 0:
            avg_ms = kt.ms_spmv / kt.n_spmv
            ach = spmv_bytes / (avg_ms * 1e-3) / 1e9
            roof = {"bound": "hbm", "kernel": "k_spmv_span", "achieved": ach, "peak": HBM_PEAK_GBS,
                    "unit": "GB/s", "frac": ach / HBM_PEAK_GBS, "traffic": traffic,
                    "traffic_source": ("profiles/r4_pmc_spmv.json: separate rocprofv3 --pmc passes of the same "
                                       "kernel on the same graph, not a counter read in this run")
                    if traffic is not None else None,
                    "avg_launch_ms": avg_ms, "launches": int(kt.n_spmv),
                    "algorithmic_bytes_per_launch": int(spmv_bytes)}
            if world == 1 and args.full:
                # what THIS box delivers for a bare stream of the same block array (16 B per lane, non-temporal,
                # after the timed region): the pool's boxes differ by up to 12 % (profiles/README.md)
                try:
                    # (mode 0: 16 B per lane; mode 2: one 392-B block per wave-instruction, the SpMV's own shape)
                    sms = {m: G.bench_stream(m, 20) for m in (0, 2)}
                    sgb = {m: 392.0 * nnzb / (t * 1e-3) / 1e9 for m, t in sms.items()}
                    roof["box_stream"] = {"GBs_16B_per_lane": sgb[0], "GBs_block_shaped": sgb[2],
                                          "ms_16B_per_lane": sms[0], "ms_block_shaped": sms[2], "bytes": int(392 * nnzb),
                                          "spmv_fraction_of_best_stream": ach / max(sgb.values())}
                except Exception as ex:  # (a measurement aid, never a reason to lose the line)
                    roof["box_stream"] = {"error": str(ex)}
                # ... and its clocks while the SpMV runs back to back for ~2 s (rocm-smi from a thread; the pool's slow
                # boxes stream as fast as the fast ones but run this kernel 12 % slower)
                try:
                    import re, subprocess, threading
                    smi = {}

                    def _smi():
                        time.sleep(0.6)
                        r = subprocess.run(["rocm-smi", "--showclocks", "--showpower"], capture_output=True, text=True, timeout=20)
                        for key in ("sclk", "mclk", "fclk"):
                            m = re.search(key + r" clock level: \S+ \((\d+)Mhz\)", r.stdout)
                            if m:
                                smi[key + "_mhz_under_load"] = int(m.group(1))
                        m = re.search(r"Power \(W\): ([0-9.]+)", r.stdout)
                        if m:
                            smi["power_w_under_load"] = float(m.group(1))

                    th = threading.Thread(target=_smi)
                    th.start()
                    G.bench_spmv(int(2.5 / max(avg_ms * 1e-3, 1e-5)))
                    th.join()
                    roof["box_clocks"] = smi
                except Exception as ex:
                    roof["box_clocks"] = {"error": str(ex)}
        out = {
            "metric": "LM iterations/s", "value": K / dt, "unit": "LM iter/s",
            "n_gpus": world, "steps": K, "warmup": args.warmup, "ms_per_step": 1e3 * dt / K,
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
            "dtype": "f64", "data": "synthetic",
            "config": {"workload": "configs[2]: synthetic Manhattan-grid Sim3 pose graph "
                                   f"{args.vertices} vertices / {args.edges} edges, information I7, "
                                   f"vertex 0 fixed, numeric Jacobians delta=1e-9, {prec_name} PCG "
                                   f"rel tol {args.pcg_rel_tol:g}",
                       "vertices": args.vertices, "edges": args.edges,
                       "fix_small_angle_b": args.fix_small_angle_b,
                       "arithmetic": ("exact small-angle B coefficient -- NOT the reference's as-written "
                                      "sim3_rv.h:166/:290 (with it LM stalls on this graph: see "
                                      "reference_arithmetic; the reference's own arithmetic is run where the "
                                      "reference runs it: kitti00_reference_configuration)")
                                     if args.fix_small_angle_b else "reference (B as written)",
                       "preconditioner": prec_name,
                       "parallelism": "single GPU" if world == 1 else f"row-partition x{world}",
                       "transport": transport_used,
                       # the tuning options the run used (sim3opt_get_options after initialize: environment
                       # overrides included) and the SIM3OPT_* variables that were set
                       "solver_options": solver_options(G),
                       # what the automatic choices resolved to (levels, levels partitioned over the ranks, cycle)
                       "multigrid_in_use": G.amg_in_use(),
                       "env_overrides": {k: v for k, v in os.environ.items() if k.startswith("SIM3OPT_")}},
            "edges_iters_per_s": args.edges * K / dt,
            "chi2_initial": chi2_0, "chi2_final": chi2_final,
            "lm_trials": [int(s.trials) for s in stats],
            "pcg_iters": [int(s.pcg_iters) for s in stats],
            "pcg_rel_res": [float("%.2e" % s.pcg_rel_res) for s in stats],
            # solves that stopped at the iteration cap short of the tolerance (an inexact LM step; 0 here)
            "unconverged_solves": int(sum(int(s.pcg_capped) for s in stats)),
            # device time of every LM iteration's solves (all its trials): the bursts of rejected trials show here
            "ms_solve": [float("%.2f" % s.ms_solve) for s in stats],
            "ms_linearize_mean": float(np.mean([s.ms_linearize for s in stats])),
            "ms_solve_mean": float(np.mean([s.ms_solve for s in stats])),
            "ms_update_mean": float(np.mean([s.ms_update for s in stats])),
            "roofline": roof,
        }
        if ct is not None:
            # rank 0's collectives inside the timed region: device time (includes waiting for the
            # slowest rank), count, payload -- what the next scaling decision needs
            npcg = max(sum(int(s.pcg_iters) for s in stats), 1)
            ms_all = ct["ms_allreduce"] + ct["ms_allgather"] + ct["ms_exchange"]
            n_all = ct["n_allreduce"] + ct["n_allgather"] + ct["n_exchange"]
            by_all = ct["bytes_allreduce"] + ct["bytes_allgather"] + ct["bytes_exchange"]
            out["collectives_rank0"] = dict(ct, ms_per_lm_iteration=ms_all / K, ms_per_pcg_iteration=ms_all / npcg,
                                            fraction_of_step=ms_all / (dt * 1e3),
                                            collectives_per_pcg_iteration=n_all / npcg,
                                            # payload: whole buffer of an all-reduce / all-gather (a rank receives
                                            # (N - 1) / N of an all-gather); sent + received bytes of this rank
                                            # for the neighbour exchanges; per PCG iteration
                                            bytes_per_pcg_iteration=by_all / npcg)
        if ct is not None and args.full:
            # the partition the collectives serve: rows in breadth-first locality order, equal spans
            _, _, bnd, cut = G.partition_plan(world)
            out["partition"] = {"row_order": "breadth-first locality order", "rows": int(nb),
                                "boundary_rows_per_rank": [int(x) for x in bnd],
                                "halo_fraction_of_vector": float(bnd.sum()) / max(1, int(nb)),
                                "cut_edges": int(cut), "cut_edge_fraction": float(cut) / max(1, len(g["v0"])),
                                # block arrays (H, FP32 copy, partitioned coarse levels, assembly scratch) as
                                # allocated on rank 0 / what one rank holding the whole graph allocates
                                "block_array_MB_rank0": G.device_bytes()[0] / 1e6,
                                "block_array_MB_one_rank": G.device_bytes()[1] / 1e6}
        if args.full and world == 1 and G.preconditioner_in_use() != 0 and not args.main_only:
            # same K steps with plain block-Jacobi PCG, for comparison (not part of `value`)
            J = L.Graph(device=local_rank, pcg_rel_tol=args.pcg_rel_tol, preconditioner=0,
                        fix_small_angle_b=args.fix_small_angle_b)
            J.add_vertices(g["states"], g["fixed"])
            J.add_edges(g["v0"], g["v1"], g["meas"])
            J.initialize()
            if args.warmup > 0:
                J.optimize(args.warmup)
                J.set_vertices(g["states"])
            torch.cuda.synchronize()
            tj0 = time.perf_counter()
            jdone, jstats = 0, []
            while jdone < K:
                it = J._L.sim3opt_optimize(J._g, K - jdone)
                if it <= 0:
                    break
                jdone += it
                jstats += J.stats()
            torch.cuda.synchronize()
            jdt = time.perf_counter() - tj0
            out["block_jacobi_pcg"] = {
                "steps": jdone, "value": jdone / jdt, "unit": "LM iter/s", "chi2_final": J.chi2(),
                "pcg_iters": [int(s.pcg_iters) for s in jstats],
                "pcg_rel_res": [float("%.2e" % s.pcg_rel_res) for s in jstats],
                "unconverged_solves": int(sum(int(s.pcg_capped) for s in jstats)),
                "note": "preconditioner = 0: solves stop at the 1000-iteration cap (truncated, i.e. inexact LM steps)"}
            J.close()
        if args.full and world == 1 and args.fix_small_angle_b == 1 and not args.main_only:
            # same K steps in the reference's as-written arithmetic (not part of `value`)
            R = L.Graph(device=local_rank, pcg_rel_tol=args.pcg_rel_tol, fix_small_angle_b=0)
            R.add_vertices(g["states"], g["fixed"])
            R.add_edges(g["v0"], g["v1"], g["meas"])
            R.initialize()
            r0 = R.chi2()
            torch.cuda.synchronize()
            tr0 = time.perf_counter()
            rdone, rstats = 0, []
            while rdone < K:
                it = R._L.sim3opt_optimize(R._g, K - rdone)
                if it <= 0:
                    break
                rdone += it
                rstats += R.stats()
            torch.cuda.synchronize()
            rdt = time.perf_counter() - tr0
            out["reference_arithmetic"] = {
                "fix_small_angle_b": 0, "steps": rdone, "value": rdone / rdt, "unit": "LM iter/s",
                "chi2_initial": r0, "chi2_final": R.chi2(),
                "pcg_iters": [int(s.pcg_iters) for s in rstats],
                "lm_trials": [int(s.trials) for s in rstats],
                "pcg_rel_res": [float("%.2e" % s.pcg_rel_res) for s in rstats],
                "preconditioner": {0: "block-Jacobi", 1: "chain-segment", 2: "aggregation-multigrid"}[R.preconditioner_in_use()],
                "lambda_last": rstats[-1].lambda_ if rstats else None,
                "unconverged_solves": int(sum(int(s.pcg_capped) for s in rstats)),
                "solves": int(sum(int(s.trials) for s in rstats)),
                "note": "B coefficient as written in sim3_rv.h:166/:290: lambda_0 = 1e-5 * max|H_dd| "
                        "is ~1e8 and LM barely moves (DESIGN.md); the multigrid hierarchy is automatic here "
                        "too.  `unconverged_solves` of `solves` stop at the 1000-iteration cap short of the "
                        "tolerance (a system that is numerically indefinite without a detectable breakdown; "
                        "it stops at 4000 as well): such a step is an inexact LM step whose fate g2o's gain "
                        "ratio decides, all others converge to pcg_rel_tol (pcg_rel_res: last trial of each "
                        "iteration).  A trial whose system breaks the PCG down (p.Ap <= 0) is rejected like "
                        "g2o's failed Cholesky"}
            R.close()
        if args.full and world == 1 and not args.main_only:
            out["optimize100_to_terminate"] = optimize100_leg(args, g, local_rank)
        if args.full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(args, g, out["ms_linearize_mean"], out["value"])
            # configs both sides actually ran, in the reference's own configuration
            out["kitti00_reference_configuration"] = kitti_table(local_rank)
            out["ba_demo"] = ba_demo_leg(local_rank)
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
