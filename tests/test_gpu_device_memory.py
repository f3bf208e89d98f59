"""Who owns device memory, and what a read-out leaves behind.  sim3opt_device_memory_in_use counts the blocks the
library has handed out and not got back; the three tests hold it, and the solver's state, against every diagnostic
read-out at once, on one small graph per solver configuration:

  exact       factor_cases chain_40 (40 block rows with three loops: a small one with pairs outside the factor's pattern)
  multigrid   pcg_cases m400, the smallest multigrid case (batch capacity 4), covariances by columns of the inverse
  jacobi      pcg_cases tiny3, block-Jacobi PCG, covariances by columns one at a time

1. no read-out keeps a block, whether it succeeds or refuses;
2. a graph, a bundle adjuster and the three batch handles give back everything when they are destroyed, and the batch
   handles when a change of options.device releases them -- after which they solve again to the same bytes;
3. optimize(3), every read-out, optimize(3) is bit for bit optimize(3), optimize(3): the per-family "change nothing" tests
   guard each family, this one their combination under the one SolverSnapshot."""
import functools
import gc

import numpy as np
import pytest

from conftest import gpu_available
from sim3opt_amd import lib as L
import ba_cases as BC
import factor_cases as FC
import match_cases as MC
import pcg_cases as PC
import pnp_cases as PNC
import two_view_cases as TC

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

BASE = dict(fix_small_angle_b=1, fd_delta=1e-6)
CONFIGS = {
    "exact": (lambda: FC.CASES["chain_40"](), dict(linear_solver=1)),
    "multigrid": (lambda: PC.graph_of("m400"), dict(linear_solver=0, preconditioner=2, amg_coarsest=16, cov_solver=1)),
    "jacobi": (lambda: PC.graph_of("tiny3"), dict(linear_solver=0, preconditioner=0, cov_solver=1)),
}
KB = 4      # engine_impl.hpp: systems of a batch
LAM = 1e-2


@functools.lru_cache(maxsize=None)
def graph(cfg):
    return CONFIGS[cfg][0]()


def make(cfg):
    g = graph(cfg)
    G = L.Graph(**BASE, **CONFIGS[cfg][1])
    G.add_vertices(g["states"], g["fixed"])
    G.add_edges(g["v0"], g["v1"], g["meas"])
    G.initialize()
    assert G.linear_solver_in_use() == (1 if cfg == "exact" else 0)
    assert cfg == "exact" or G.preconditioner_in_use() == CONFIGS[cfg][1]["preconditioner"]
    return G


@functools.lru_cache(maxsize=None)
def inputs(cfg):
    """Everything the read-outs are called with, from the graph alone (seeded; shared, left unchanged)."""
    g = graph(cfg)
    G = make(cfg)
    rp, ci = G.system_pattern()
    levels = G.amg_structure() if cfg == "multigrid" else []
    free = np.flatnonzero(np.asarray(g["fixed"]) == 0)
    off = None  # a pair outside the pattern of the marginals' factor, if the graph has one: marginals() refuses it
    for j in range(len(free) - 1, 0, -1):
        try:
            G.marginals([(int(free[0]), int(free[j]))], LAM)
        except L.Sim3OptError as e:
            assert "outside the pattern" in str(e)
            off = (int(free[0]), int(free[j]))
            break
    G.close()
    assert off is not None or cfg == "jacobi"  # (four vertices: the factor is full)
    nb = rp.shape[0] - 1
    rng = np.random.default_rng(5)
    both = [(a, b) for a, b in zip(g["v0"], g["v1"]) if not g["fixed"][a] and not g["fixed"][b]]
    vals, b = FC.injected(g, rp, ci)
    a, z = off if off else (int(free[0]), int(free[-1]))
    return dict(nb=nb, vals=vals, b=b, levels=levels, step=1e-3 * rng.standard_normal(7 * nb),
                vecs=rng.standard_normal((KB, 7 * nb)),
                on_pattern=[(a, a), (int(both[0][0]), int(both[0][1]))],     # a vertex with itself, an edge
                any_pairs=[(a, z), (z, a), (z, z)],                           # (first, last): outside the pattern
                off=off, gate=(np.array([a, 0], dtype=np.int32), np.array([z, a], dtype=np.int32), g["meas"][:2]))


def readouts(cfg, G):
    """[(name, call)]: every read-out that applies to the configuration, in the fixed order of the three tests."""
    I = inputs(cfg)
    prec = dict(exact=0, multigrid=2, jacobi=0)[cfg]
    out = [
        ("edge_errors", G.edge_errors),
        ("preconditioner_apply", lambda: G.preconditioner_apply(prec, LAM, I["vecs"][:2])),
        ("marginals", lambda: G.marginals(I["on_pattern"], LAM)),
        ("debug_update", lambda: G.debug_update(I["step"], 0.3)),
        ("operator_apply_1", lambda: G.operator_apply(LAM, I["vecs"][0], I["vecs"][1])),
        ("edge_chi2", G.edge_chi2),
        ("debug_factor_1", lambda: G.debug_factor(1, LAM, selinv=True)),
        ("covariances", lambda: G.covariances(I["any_pairs"], LAM)),
        ("debug_linearization", G.debug_linearization),
        ("debug_factor_1_injected", lambda: G.debug_factor(1, LAM, I["vals"], I["b"], selinv=True)),
        ("gate_edges", lambda: G.gate_edges(*I["gate"], lam=LAM)),
        ("edge_jacobians", G.edge_jacobians),
        ("spmv_spans", G.spmv_spans),
        ("debug_update_grid", lambda: G.debug_update(I["step"], 0.1, grid=3)),
    ]
    if cfg == "exact":
        out += [("debug_factor_0", lambda: G.debug_factor(0, LAM)),
                ("debug_update_fail", lambda: G.debug_update(I["step"], 0.1, fail=True)),
                ("debug_factor_0_injected", lambda: G.debug_factor(0, LAM, I["vals"], I["b"]))]
    if cfg == "multigrid":
        top, last = I["levels"][0], I["levels"][-1]
        out += [("operator_apply_KB", lambda: G.operator_apply([LAM, 0.0, 1.0, 10.0], I["vecs"], I["vecs"][::-1])),
                ("amg_level_numbers_0", lambda: G.amg_level_numbers(LAM, 0, top["nb"], top["nnzb"])),
                ("amg_coarsest_inverse", lambda: G.amg_coarsest_inverse(LAM, last["nb"])),
                ("amg_level_numbers_last", lambda: G.amg_level_numbers(LAM, len(I["levels"]) - 1, last["nb"], last["nnzb"])),
                ("preconditioner_apply_0", lambda: G.preconditioner_apply(0, LAM, I["vecs"][0]))]
    return out


def refusals(cfg, G):
    """[(name, call)]: arguments the read-outs refuse -- some before they touch the device, some after their set-up."""
    I = inputs(cfg)
    nan = float("nan")
    out = [
        ("marginals_nan", lambda: G.marginals(I["on_pattern"], nan)),
        ("covariances_inf", lambda: G.covariances(I["any_pairs"], float("inf"))),
        ("gate_edges_nan", lambda: G.gate_edges(*I["gate"], lam=nan)),
        ("debug_factor_nan", lambda: G.debug_factor(1, nan, selinv=True)),
        ("debug_factor_0_selinv", lambda: G.debug_factor(0, LAM, selinv=True)),
        ("preconditioner_apply_chain", lambda: G.preconditioner_apply(1, LAM, I["vecs"][0])),
    ]
    if I["off"]:
        out += [("marginals_off_pattern", lambda: G.marginals([I["off"]], LAM))]
    if cfg != "exact":
        out += [("debug_update_fail", lambda: G.debug_update(I["step"], 0.1, fail=True)),
                ("debug_factor_0", lambda: G.debug_factor(0, LAM))]
    if cfg == "multigrid":  # (the set-up for lambda runs, then the level is refused)
        top = I["levels"][0]
        out += [("amg_unknown_level", lambda: G.amg_level_numbers(LAM, 99, top["nb"], top["nnzb"]))]
    else:
        out += [("amg_level_numbers", lambda: G.amg_level_numbers(LAM, 0, I["nb"], 1)),
                ("amg_coarsest_inverse", lambda: G.amg_coarsest_inverse(LAM, 1)),
                ("operator_apply_KB", lambda: G.operator_apply([LAM] * KB, I["vecs"]))]
    return out


@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_no_read_out_keeps_a_block(cfg):
    inputs(cfg)
    gc.collect()  # (handles other tests dropped go now, not in the middle of the count)
    G = make(cfg)
    G.linearize()
    for name, call in readouts(cfg, G):  # the first calls build what is built lazily: the batch's buffers, the columns',
        call()                           # the marginal context
    held = L.device_memory_in_use()
    assert held[0] > 0 and held[1] >= 256 * held[0]
    for name, call in readouts(cfg, G):
        call()
        assert L.device_memory_in_use() == held, name
    for name, call in refusals(cfg, G):
        with pytest.raises(L.Sim3OptError):
            call()
        assert L.device_memory_in_use() == held, name
    for name, call in readouts(cfg, G):  # ... and a refusal leaves nothing half-built behind
        call()
        assert L.device_memory_in_use() == held, name
    G.close()
    assert L.device_memory_in_use()[0] < held[0]


def test_handles_give_everything_back():
    for cfg in CONFIGS:
        inputs(cfg)
    gc.collect()
    start = L.device_memory_in_use()
    for cfg in sorted(CONFIGS):
        G = make(cfg)
        during = L.device_memory_in_use()
        assert during[0] > start[0] and during[1] > start[1]
        assert G.optimize(1) == 1
        G.covariances(inputs(cfg)["any_pairs"], LAM)  # (the lazily built owners too: marginal context or column buffers)
        G.close()
        assert L.device_memory_in_use() == start, cfg
    P = BC.problem("tiny")
    for solver in (0, 1):  # PCG on the reduced system, the exact factorisation of it
        b = L.BundleAdjuster(linear_solver=solver)
        b.set_problem(P.cams, P.points, P.oc, P.op, P.uv, P.f, P.cx, P.cy)
        assert b.optimize(1) == 1
        assert L.device_memory_in_use()[0] > start[0]
        b.close()
        assert L.device_memory_in_use() == start, f"ba, linear_solver {solver}"
    t = L.TwoViewBatch()
    t.set_problems(**TC.batch_arrays(TC.ONE_ITERATION_CASES[:1]))
    assert t.optimize() == 1
    assert not t.debug_trial(50.0)["fail"].any()  # (the read-out's blocks are gone when it returns)
    assert L.device_memory_in_use()[0] == start[0] + 4  # (its four blocks)
    t.close()
    assert L.device_memory_in_use() == start, "two-view batch"
    pnp_batch_gives_everything_back(start)
    match_batch_gives_everything_back(start)
    two_view_batch_survives_a_release(start)


def as_bytes(x):
    """A getter's output -- an array, a tuple or a dict of them, a list of per-iteration dicts -- as comparable bytes."""
    if isinstance(x, dict):
        return tuple((k, as_bytes(v)) for k, v in sorted(x.items()))
    if isinstance(x, (tuple, list)):
        return tuple(as_bytes(v) for v in x)
    return np.asarray(x).tobytes()


def pnp_getters(b):
    return as_bytes([b.poses(), b.inliers(), b.summary()])


def pnp_batch_gives_everything_back(start):
    two, three = PNC.batch_arrays(PNC.MANY_CASES[:2]), PNC.batch_arrays(PNC.MANY_CASES[:3])
    b = L.PnpBatch()  # (device = -1; MANY_CASES hold the nine points the defaults ask for)
    b.set_problems(**two)
    b.solve()
    first = pnp_getters(b)
    assert L.device_memory_in_use()[0] == start[0] + 8  # pointers, input, three hypothesis blocks, two outputs, the mask
    b.solve()
    assert L.device_memory_in_use()[0] == start[0] + 8
    b.set_problems(**three)  # another size: every block goes and comes again
    b.solve()
    assert L.device_memory_in_use()[0] == start[0] + 8
    b.set_problems(**two)
    b.solve()
    assert pnp_getters(b) == first
    b.set_options(device=0)  # the option changes: release()
    assert L.device_memory_in_use() == start, "pnp batch, released by set_options"
    assert pnp_getters(b) == first  # (the results of the last solve stay on the host)
    b.solve()
    assert L.device_memory_in_use()[0] == start[0] + 8
    assert pnp_getters(b) == first
    b.close()
    assert L.device_memory_in_use() == start, "pnp batch"


def match_getters(b):
    return as_bytes([b.match_ptr(), b.matches(), b.summary()])


def match_batch_gives_everything_back(start):
    rng = np.random.default_rng(19)
    w, h = MC.KITTI["image_width"], MC.KITTI["image_height"]
    pool, homes = MC._pool(rng, 30, w, h)
    frames = [MC._quantised_frame(rng, pool, homes, n_kp, n_obs, w, h) for n_kp, n_obs in ((40, 30), (37, 45))]
    b = L.MatchBatch()  # (device = -1)
    b.set_frames(**MC.frame_arrays(frames), **MC.KITTI)
    b.set_pairs([(0, 1)])
    assert b.solve() == 1 and b.match_ptr()[-1] > 0
    first = match_getters(b)
    nn = as_bytes(b.debug_nn(0))
    assert L.device_memory_in_use()[0] == start[0] + 22  # 6 blocks of the frames, 16 of the pairs
    b.solve()
    assert L.device_memory_in_use()[0] == start[0] + 22
    b.set_pairs([(0, 1), (1, 0)])  # another size: the pairs' blocks go at the next solve, the frames' stay
    assert L.device_memory_in_use()[0] == start[0] + 22
    assert b.solve() == 2
    assert L.device_memory_in_use()[0] == start[0] + 22
    b.debug_depth(0, frames[0]["kp"][:5])  # (the frames' blocks alone, and temporaries that go)
    assert L.device_memory_in_use()[0] == start[0] + 22
    b.set_pairs([(0, 1)])
    b.solve()
    assert match_getters(b) == first and as_bytes(b.debug_nn(0)) == nn
    b.set_options(device=0)  # the option changes: release()
    assert L.device_memory_in_use() == start, "match batch, released by set_options"
    assert match_getters(b) == first  # (the results of the last solve stay on the host)
    with pytest.raises(L.Sim3OptError, match="the device blocks of the last solve were released; solve again"):
        b.debug_nn(0)
    assert L.device_memory_in_use() == start
    assert b.solve() == 1
    assert L.device_memory_in_use()[0] == start[0] + 22
    assert match_getters(b) == first and as_bytes(b.debug_nn(0)) == nn
    b.close()
    assert L.device_memory_in_use() == start, "match batch"


def two_view_getters(t):
    return as_bytes([t.cameras(), t.points(), t.num_iterations(), [t.stats(k) for k in range(t.dims()[0])],
                     t.lambda_init(), t.chi2()])


def two_view_batch_survives_a_release(start):
    a = TC.batch_arrays(TC.ONE_ITERATION_CASES[1:3])
    t = L.TwoViewBatch()  # (device = -1)
    t.set_problems(**a)
    assert t.optimize() == 2
    first = two_view_getters(t)
    assert L.device_memory_in_use()[0] == start[0] + 4
    t.set_options(device=0)  # the option changes: release()
    assert L.device_memory_in_use() == start, "two-view batch, released by set_options"
    assert two_view_getters(t) == first  # (the results of the last run stay on the host)
    t.set_problems(**a)  # (optimize() goes on from the estimate it left: the same start again)
    assert t.optimize() == 2
    assert L.device_memory_in_use()[0] == start[0] + 4
    assert two_view_getters(t) == first
    t.close()
    assert L.device_memory_in_use() == start, "two-view batch"


def outcome(G):
    """What two optimize() calls left, as bytes: estimates, per-iteration statistics without the three phase times (they
    are measurements), the PCG schedule's counters and the launch counters."""
    st = [tuple(getattr(t, k) for k, _ in L.IterStats._fields_ if not k.startswith("ms_")) for t in G.stats()]
    kt = G.kernel_times()
    counts = {k: getattr(kt, k) for k, _ in L.KernelTimes._fields_ if k.startswith("n_")}
    return dict(states=G.get_vertices().tobytes(), stats=np.array(st, dtype=np.float64).tobytes(),
                schedule=G.pcg_schedule_stats(), counts=counts)


@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_the_read_outs_together_change_nothing(cfg):
    """Run A: optimize(3), every read-out of the configuration in the fixed interleaved order of readouts() -- refusals
    included --, optimize(3).  Run B: the two optimize() calls on a fresh graph.  Estimates, statistics and counters
    are equal bit for bit, after the first call and after the second; so is a covariance request made at the end of
    both, with its covariance_stats (run B's first and only one)."""
    I = inputs(cfg)
    A, B = make(cfg), make(cfg)
    assert A.optimize(3) == B.optimize(3) >= 1
    first = outcome(B)
    assert outcome(A) == first
    for name, call in readouts(cfg, A):
        call()
    for name, call in refusals(cfg, A):
        with pytest.raises(L.Sim3OptError):
            call()
    assert outcome(A) == first  # (the counters and the estimates, before anything else runs)
    na, nb = A.optimize(3), B.optimize(3)
    assert na == nb and na >= 1
    got, want = outcome(A), outcome(B)
    for k in want:
        assert got[k] == want[k], k
    za, zb = A.covariances(I["any_pairs"], LAM), B.covariances(I["any_pairs"], LAM)
    assert za.tobytes() == zb.tobytes()
    assert A.covariance_stats() == B.covariance_stats()
    if cfg != "exact":
        assert A.covariance_columns_stats() == B.covariance_columns_stats()
    A.close()
    B.close()
