"""Who owns device memory, and what a read-out leaves behind.  sim3opt_device_memory_in_use counts the blocks the
library has handed out and not got back; the three tests hold it, and the solver's state, against every diagnostic
read-out at once, on one small graph per solver configuration:

  exact       factor_cases chain_40 (40 block rows with three loops: a small one with pairs outside the factor's pattern)
  multigrid   pcg_cases m400, the smallest multigrid case (batch capacity 4), covariances by columns of the inverse
  jacobi      pcg_cases tiny3, block-Jacobi PCG, covariances by columns one at a time

1. no read-out keeps a block, whether it succeeds or refuses;
2. a graph, a bundle adjuster and a two-view batch give back everything when they are destroyed;
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
import pcg_cases as PC
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
    assert L.device_memory_in_use()[0] == start[0] + 4  # (its four blocks)
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
