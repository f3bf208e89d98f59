"""GPU tests (-m gpu) of the PCG loop's SCHEDULE: how many iterations the host enqueues between two looks at the
solver's scalars, and whether a look drains the queue (Engine::pcg_run, engine_pcg.hip: one system or a batch).  The
stopping iteration is decided on the device, so the schedule must not show in any result: every case is compared, bit
for bit, with pcg_check_every = 1 -- one iteration per look, no prediction -- and the read-out
sim3opt_pcg_schedule_stats says whether the schedule does what it is for: few iterations enqueued after `done`, few
looks that drain the queue.

Graphs and options as in test_gpu_preconditioners.py; dampings relative to max diag(H): 1e-7, 1e-3, 1.
"""
import numpy as np
import pytest

from sim3opt_amd import lib as L, synth

pytestmark = pytest.mark.gpu

LAMS = (1e-7, 1e-3, 1.0)
# (graph, preconditioner, options): the multigrid cases come first (test 3 reads exactly these)
CASES = [("m400", 2, dict(amg_coarsest=16)), ("m1500", 2, dict(amg_coarsest=16)), ("m400", 0, {}), ("m1500", 0, {}),
         ("chain_150", 1, {}), ("chain_150", 0, {})]
MG = [c for c in range(len(CASES)) if CASES[c][1] == 2]
# the anchors poll every iteration; the three others are the default schedule on the replayed-graph path (the
# default), on the eager path and on the timed eager path (what the benchmark runs)
VARIANTS = {"anchor": dict(pcg_check_every=1), "anchor_timed": dict(pcg_check_every=1, time_kernels=1),
            "graph": dict(pcg_graph=1), "eager": dict(pcg_graph=0), "timed": dict(time_kernels=1)}


def graph_of(name):
    synth.DRIFT_TARGET = 0.05
    if name == "m400":
        return synth.manhattan(400, 4000, dims=(6, 6, 10))
    if name == "m1500":
        return synth.manhattan(1500, 15000, dims=(14, 14, 8))
    if name == "chain_150":
        return synth.chain_loop(150, 300)
    raise KeyError(name)


def mk(g, **opts):
    o = dict(fix_small_angle_b=1, fd_delta=1e-6, linear_solver=0)
    o.update(opts)
    G = L.Graph(**o)
    G.add_vertices(g["states"], g["fixed"])
    G.add_edges(g["v0"], g["v1"], g["meas"])
    G.initialize()
    return G


def stats_tuple(G, timed):
    """The full tuples, as test_readouts_change_nothing compares them -- but for the three phase times of a timed
    run, which are measurements (they are zero on graphs this small otherwise)."""
    return [tuple(getattr(s, f) for f, _ in s._fields_ if not (timed and f.startswith("ms_"))) for s in G.stats()]


_runs = {}


def run(case, variant):
    """Three solves at the initial linearisation, then optimize(6); computed once per (case, variant)."""
    key = (case, variant)
    if key in _runs:
        return _runs[key]
    name, prec, opts = CASES[case]
    vo = VARIANTS[variant]
    G = mk(graph_of(name), preconditioner=prec, **opts, **vo)
    assert G.preconditioner_in_use() == prec
    G.linearize()
    rp, ci, blk, b = G.get_system()
    maxdiag = float(np.abs(blk[rp[:-1]].diagonal(0, 1, 2)).max())
    G.kernel_times(reset=True)
    G.pcg_schedule_stats(reset=True)
    solves = [G.solve(lam * maxdiag) for lam in LAMS]
    sched, n_spmv = G.pcg_schedule_stats(), int(G.kernel_times().n_spmv)
    assert G.optimize(6) == 6
    r = dict(solves=solves, sched=sched, n_spmv=n_spmv, verts=G.get_vertices(),
             stats=stats_tuple(G, "time_kernels" in vo), sched_all=G.pcg_schedule_stats())
    G.close()
    _runs[key] = r
    return r


@pytest.mark.parametrize("variant", ["graph", "eager", "timed"])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_schedule_changes_no_result(case, variant):
    """x, the iteration count and the relative residual of G.solve at the three dampings, and the estimates and
    stats() of optimize(6): identical to polling every iteration."""
    timed = variant == "timed"
    a, r = run(case, "anchor_timed" if timed else "anchor"), run(case, variant)
    for lam, (xa, ia, ra), (xr, ir, rr) in zip(LAMS, a["solves"], r["solves"]):
        assert np.array_equal(xa, xr), lam
        assert ia == ir and ra == rr, (lam, ia, ir, ra, rr)
    assert np.array_equal(a["verts"], r["verts"])
    assert a["stats"] == r["stats"]
    print(f"[schedule] {CASES[case][0]} prec {CASES[case][1]} {variant}: PCG iterations "
          f"{[s[1] for s in r['solves']]}, solves {r['sched']}, with optimize(6) {r['sched_all']}")


def test_batched_solve_is_scheduled_the_same_way():
    """LM with bursts of rejected trials (delta = 1e-9, as test_batched_rejected_trials_equal_sequential_solves), the
    trial systems solved together (pcg_batch = 4): trial counts, dampings, chi2, PCG iteration counts and capped flags
    of every iteration and the estimates equal those with pcg_check_every = 1 -- every solution a batch hands out is
    evaluated by its trial."""
    synth.DRIFT_TARGET = 0.05
    g = synth.manhattan(3000, 30000, dims=(17, 17, 10))
    out = []
    for o in (dict(pcg_check_every=1), {}):
        G = L.Graph(fix_small_angle_b=1, pcg_rel_tol=1e-8, preconditioner=2, pcg_batch=4, **o)
        G.add_vertices(g["states"], g["fixed"])
        G.add_edges(g["v0"], g["v1"], g["meas"])
        G.initialize()
        G.pcg_schedule_stats(reset=True)
        n = G.optimize(30)
        kt = G.kernel_times()
        out.append((n, stats_tuple(G, False), int(kt.n_batches), int(kt.n_batched_solves), G.get_vertices(),
                    G.pcg_schedule_stats()))
        G.close()
    a, r = out
    print(f"[schedule] batch: {r[2]} batches of {r[3]} systems; anchor {a[5]}, default {r[5]}")
    assert a[2] >= 2 and a[3] >= 2 * a[2]  # (the case reaches pcg_batch)
    assert a[:4] == r[:4]
    assert np.array_equal(a[4], r[4])
    assert a[5]["past_done"] == 0 and a[5]["overlapped_polls"] == 0
    # the default run did predict: solves of twenty and more iterations cannot all have gone by without one look
    # that had the next chunk queued behind it, and the chunks were not the anchor's
    assert r[5]["overlapped_polls"] > 0 and r[5]["sync_polls"] < a[5]["sync_polls"]


def test_batch_view_of_one_system_equals_batch_view_of_four():
    """The two widths of the batch's view against each other through the one driver: the columns of the inverse of three
    vertices (21 columns) on the smallest multigrid case, solved four to a batch (five batches of four and a last one of
    ONE system: every launch of it carries live == 1, the K = 1 kernels on the batch's buffers) and one to a batch
    (pcg_batch = 1: 21 batches of one).  A column's bits do not depend on its batch partners
    (test_gpu_covariance_columns.py asserts that for one block), so every returned block and the PCG iterations summed
    over the columns are equal, bit for bit.  The column call puts kernel_times() back as it found it, so the batch
    counts are read from its own stats."""
    name, prec, opts = CASES[0]
    assert (name, prec, opts) == ("m400", 2, dict(amg_coarsest=16))
    pairs, lam, out = [(250, 250), (11, 11), (120, 120)], 1e-2, []
    for width in (4, 1):
        G = mk(graph_of(name), preconditioner=prec, cov_solver=1, pcg_batch=width, **opts)
        assert G.preconditioner_in_use() == prec
        kt0 = G.kernel_times()
        Z = G.covariances(pairs, lam)
        st, kt = G.covariance_columns_stats(), G.kernel_times()
        assert (int(kt.n_batches), int(kt.n_batched_solves)) == (int(kt0.n_batches), int(kt0.n_batched_solves))
        print(f"[schedule] columns, {width} to a batch: {st}")
        assert st["columns"] == 21 and st["vertices"] == 3
        assert 21 % width == (1 if width == 4 else 0)  # width 4: the last batch is one system
        assert st["batches"] == -(-21 // width)  # (the first passes; a refinement solve is not counted as a batch)
        out.append((Z, st["pcg_iters"], st["refinements"], st["max_rel_residual"]))
        G.close()
    assert np.abs(out[0][0]).max() > 1e-3 and out[0][1] >= 21
    assert np.array_equal(out[0][0], out[1][0])
    assert out[0][1:] == out[1][1:]


@pytest.mark.parametrize("variant", ["graph", "eager", "timed"])
def test_schedule_wastes_little(variant):
    """Over the multigrid solves above, with N_i their iteration counts: fixed chunks of four enqueue
    D4 = sum(4 ceil(N_i / 4) - N_i) iterations past convergence and drain the queue sum(ceil(N_i / 4) + 1) times.  The
    schedule enqueues at most D4 / 2 iterations after `done` and drains the queue no more often."""
    N = [s[1] for c in MG for s in run(c, variant)["solves"]]
    d4 = sum(4 * -(-n // 4) - n for n in N)
    polls4 = sum(-(-n // 4) + 1 for n in N)
    assert d4 >= 8, N  # (a change of the generators must not empty this test)
    past = sum(run(c, variant)["sched"]["past_done"] for c in MG)
    sync = sum(run(c, variant)["sched"]["sync_polls"] for c in MG)
    over = sum(run(c, variant)["sched"]["overlapped_polls"] for c in MG)
    enq = sum(run(c, variant)["sched"]["enqueued"] for c in MG)
    print(f"[schedule] {variant}: N {N}, enqueued {enq}, past done {past} (D4 {d4}), synchronising polls {sync} "
          f"(fixed chunks: {polls4}), overlapped {over}")
    assert 2 * past <= d4
    assert sync <= polls4


@pytest.mark.parametrize("anchor", ["anchor", "anchor_timed"])
def test_one_iteration_per_poll_enqueues_nothing_past_done(anchor):
    for c in range(len(CASES)):
        s = run(c, anchor)["sched_all"]
        assert s["past_done"] == 0 and s["overlapped_polls"] == 0 and s["enqueued"] > 0, (CASES[c], s)


def test_working_spmv_launches_are_counted_as_before():
    """kernel_times().n_spmv (timed runs) counts the launches that did their work, whatever was enqueued behind
    them: the same as with one iteration per poll, where every launch works."""
    for c in range(len(CASES)):
        a, r = run(c, "anchor_timed"), run(c, "timed")
        assert a["n_spmv"] == r["n_spmv"] == a["sched"]["enqueued"], (CASES[c], a["n_spmv"], r["n_spmv"], a["sched"])
        assert r["n_spmv"] >= sum(s[1] for s in r["solves"])
