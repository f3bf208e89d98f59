"""One process drives N ranks (Graph.set_devices, sim3opt_set_devices): the library's own worker threads and the
in-process transport -- k_comm_put into the peers' device mailboxes, a host barrier, k_comm_reduce / k_comm_unpack --
against the same graph run as thread-ranks over the host-staged callback transport (dist_helpers.ThreadGroup, which is
the reference and is not changed).

Every comparison is np.array_equal / ==, not a tolerance.  That is derivable: the two runs launch the same kernels
on the same partition; what differs is how an operand travels.  The copies are copies, and the all-reduce folds the
ranks' operands left to right in rank order in both (ThreadGroup.allreduce: slots[0] + slots[1] + ..., k_comm_reduce:
((s0 + s1) + s2) + ..., no contraction), so every rank gets the same bits in both, and every decision that follows
-- PCG stopping, LM trials -- is the same.  All ranks share device 0: a repeated ordinal is how one GPU runs N ranks."""
import os
import sys

import numpy as np
import pytest
import torch

import dist_helpers as H
from sim3opt_amd import lib as L, synth

pytestmark = pytest.mark.gpu

BASE = dict(fix_small_angle_b=1, fd_delta=1e-6, pcg_rel_tol=1e-12)


def small_graph():
    synth.DRIFT_TARGET = 0.05
    return synth.manhattan(300, 2500, dims=(7, 7, 4), per_cell=4)


def big_graph():
    synth.DRIFT_TARGET = 0.05
    return synth.manhattan(1500, 15000, dims=(12, 12, 10))


def chain_graph():
    synth.DRIFT_TARGET = 0.05
    return synth.chain_loop(200, 239, seed_graph=911, seed_noise=912, min_gap=10)  # 199 odometry edges + 40 loops


def fill(G, g, **edge_kw):
    G.add_vertices(g["states"], g["fixed"])
    G.add_edges(g["v0"], g["v1"], g["meas"], **edge_kw)


def read(G, n):
    st = G.stats()
    return dict(n=n, states=G.get_vertices(), chi=[s.chi2_after for s in st], trials=[s.trials for s in st],
                pcg=[s.pcg_iters for s in st])


def same(a, b):
    """bit for bit: estimates, every chi2_after, trial counts, PCG iterations per LM iteration"""
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], (k, a[k], b[k])


def both(world, g, opts, drive, edge_kw=None, neighbour=True):
    """drive(G) -> dict on a set_devices([0] * world) graph from this thread, and on `world` thread-ranks; returns
    (single-process result, thread-rank results)."""
    edge_kw = edge_kw or {}
    S = L.Graph(**opts)
    fill(S, g, **edge_kw)
    S.set_devices([0] * world)
    assert S.rank_count() == world
    S.initialize()
    one = drive(S)
    S.close()
    tg = H.ThreadGroup(world)

    def rank_body(rank):
        G = L.Graph(device=0, **opts)
        fill(G, g, **edge_kw)
        tg.attach(G, rank, neighbour)
        G.initialize()
        out = drive(G)
        G.close()
        return out

    return one, tg.run(rank_body)


def check_both(world, g, opts, drive, **kw):
    one, ranks = both(world, g, opts, drive, **kw)
    for r in ranks:
        same(one, r)
    return one


def optimize4(G):
    return read(G, G.optimize(4))


def test_two_ranks_block_jacobi():
    """one neighbour per rank: 2-double and 1-double all-reduces, the exchange, the all-gather of the step"""
    one = check_both(2, chain_graph(), dict(preconditioner=0, **BASE), optimize4)
    assert one["n"] == 4


@pytest.mark.parametrize("world,verts,shard", [(4, 300, 1), (6, 300, 1), (8, 1500, 10)])
def test_partitioned_coarse_levels(monkeypatch, world, verts, shard):
    """Coarse levels partitioned at about 10 rows per rank: short and one-sided neighbour lists, ranks with an empty
    coarse span (8 ranks: the full pointer table), the mailbox growing from a 1-double all-reduce to the Galerkin
    all-gather."""
    monkeypatch.setenv("SIM3OPT_AMG_COARSEST", "16")
    monkeypatch.setenv("SIM3OPT_AMG_SHARD_ROWS", str(shard))

    def drive(G):
        mg = G.amg_in_use()
        assert mg["partitioned_levels"] >= 2, mg
        out = optimize4(G)
        out["mg"] = mg
        return out

    one = check_both(world, big_graph() if verts == 1500 else small_graph(), dict(preconditioner=2, **BASE), drive)
    assert one["n"] == 4


def test_three_ranks_dense_information_and_huber(monkeypatch):
    """The set-up of test_partitioned_multigrid_with_information_and_huber_matches_oracle.  The oracle's side of it --
    a minute of CPU time -- is read from its record, tests/golden/single_process_ranks_huber_oracle.npz
    (tests/golden/make_single_process_golden.py; the fingerprint says that the record is of these inputs)."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_single_process_golden as MG
    monkeypatch.setenv("SIM3OPT_AMG_COARSEST", "64")
    monkeypatch.setenv("SIM3OPT_AMG_SHARD_ROWS", "10")
    g, inf = MG.inputs()
    rec = np.load(os.path.join(MG.HERE, "single_process_ranks_huber_oracle.npz"))
    assert np.allclose(rec["inputs_sum"], MG.fingerprint(g, inf), rtol=1e-12, atol=0.0)
    one = check_both(3, g, dict(preconditioner=2, **BASE), optimize4,
                     edge_kw=dict(info=inf, kernel=L.KERNEL_HUBER, kernel_delta=0.5))
    assert one["n"] == int(rec["iterations"]) == 4 and one["trials"] == [int(t) for t in rec["trials"]]
    assert np.allclose(one["chi"], rec["chi2_after"], rtol=1e-7)
    assert synth.rmse(one["states"], rec["states"]) < 1e-4


def test_two_ranks_dogleg():
    """the 6-double all-reduce of the dogleg's scalars and the all-gather of b"""
    synth.DRIFT_TARGET = 0.6
    g = synth.chain_loop(240, 720, seed_graph=7101, seed_noise=7102, min_gap=5)
    rng = np.random.default_rng(31)
    M = rng.standard_normal((len(g["v0"]), 7, 7)) * 0.3
    inf = np.einsum("kij,klj->kil", M, M) + np.eye(7)
    opts = dict(algorithm=L.ALGORITHM_DOGLEG, dl_delta_init=0.1, fix_small_angle_b=1, fd_delta=1e-4, linear_solver=0,
                preconditioner=0, pcg_rel_tol=1e-12, pcg_max_iters=20000)

    def drive(G):
        out = read(G, G.optimize(11))
        out["steps"] = [t.step for t in G.trust_region_stats()]
        out["delta"] = [t.delta_after for t in G.trust_region_stats()]
        return out

    one = check_both(2, g, opts, drive, edge_kw=dict(info=inf))
    assert one["n"] == 11


def test_four_ranks_whole_vector_all_gathers():
    """halo_exchange = 0: whole-vector all-gathers in the place of the neighbour exchanges"""
    one = check_both(4, small_graph(), dict(preconditioner=0, halo_exchange=0, **BASE), optimize4)
    assert one["n"] == 4


def test_three_ranks_graph_that_changes():
    g = small_graph()

    def drive(G):
        out = {}
        for k, v in read(G, G.optimize(2)).items():
            out["a_" + k] = v
        a, b, m = G.get_edge(len(g["v0"]) - 1)
        G.add_edge(a, b, m)  # one more loop edge: re-initialise, the graph stays partitioned
        G.initialize()
        for k, v in read(G, G.optimize(2)).items():
            out["b_" + k] = v
        pert = out["b_states"].copy()
        pert[:, 4:7] += 1e-3 * np.random.default_rng(6).standard_normal((pert.shape[0], 3))
        pert[g["fixed"] != 0] = out["b_states"][g["fixed"] != 0]
        G.set_vertices(pert)
        out["c_chi2"] = G.chi2()
        out["c_states"] = G.get_vertices()
        G.set_edge_kernels([3, 50, 700, 1500, 2400], L.KERNEL_CAUCHY, 0.7)
        for k, v in read(G, G.optimize(1)).items():
            out["d_" + k] = v
        out["d_edge_chi2"] = G.edge_chi2()[0]
        return out

    one = check_both(3, g, dict(preconditioner=0, **BASE), drive)
    assert one["a_n"] == 2 and one["b_n"] == 2 and one["d_n"] == 1
    assert not np.array_equal(one["c_states"], one["b_states"])  # (the perturbed state went in)


def test_one_device_is_the_plain_graph():
    g = small_graph()
    A = L.Graph(preconditioner=0, **BASE)
    fill(A, g)
    A.set_devices([0])
    assert A.rank_count() == 1
    A.initialize()
    B = L.Graph(preconditioner=0, **BASE)
    fill(B, g)
    assert B.rank_count() == 1
    B.initialize()
    same(read(A, A.optimize(4)), read(B, B.optimize(4)))
    assert A.local_rows() == A.local_rows_of_rank(0) == B.local_rows()
    A.close()
    B.close()


def code_of(call):
    with pytest.raises(L.Sim3OptError) as e:
        call()
    return e.value.code


def test_refusals_leave_the_graph_usable():
    g = small_graph()
    ndev = torch.cuda.device_count()
    G = L.Graph(preconditioner=0, **BASE)
    fill(G, g)
    assert code_of(lambda: G.set_devices([])) == L.ERR_ARG
    assert code_of(lambda: G.set_devices([0] * 9)) == L.ERR_ARG
    assert code_of(lambda: G.set_devices([0, ndev])) == L.ERR_ARG
    assert code_of(lambda: G.set_devices([0, -1])) == L.ERR_ARG
    assert G.rank_count() == 1
    G.initialize()
    assert code_of(lambda: G.set_devices([0, 0])) == L.ERR_STATE  # after initialize
    assert G.optimize(1) == 1 and G.rank_count() == 1
    G.close()

    tg = H.ThreadGroup(1)
    G = L.Graph(preconditioner=0, **BASE)
    fill(G, g)
    tg.attach(G, 0)
    assert code_of(lambda: G.set_devices([0, 0])) == L.ERR_STATE  # the ranks come from outside
    G.initialize()
    assert G.optimize(1) == 1
    G.close()

    G = L.Graph(preconditioner=0, **BASE)
    fill(G, g)
    G.set_devices([0, 0])
    assert code_of(lambda: tg.attach(G, 0)) == L.ERR_STATE  # comm_init_callbacks after set_devices
    G.initialize()
    # what a partitioned graph refuses, it refuses here
    free = [int(v) for v in np.flatnonzero(g["fixed"] == 0)[:2]]
    nb = G.system_dims()[0]
    for call in (lambda: G.marginals([(free[0], free[0])]), lambda: G.covariances([(free[0], free[1])]),
                 lambda: G.gate_edges([free[0]], [free[1]], g["meas"][:1]), lambda: G.solve(1e-3),
                 lambda: G.operator_apply(1e-3, np.ones(7 * nb)), lambda: G.debug_factor()):
        assert code_of(call) == L.ERR_STATE
    G.linearize()
    assert code_of(lambda: G.solve(1e-3)) == L.ERR_STATE
    assert code_of(lambda: G.operator_apply(1e-3, np.ones(7 * nb))) == L.ERR_STATE
    assert G.optimize(2) == 2 and np.isfinite(G.chi2())
    G.close()


def test_ownership_of_device_memory():
    g = small_graph()
    before = L.device_memory_in_use()

    def run():
        G = L.Graph(preconditioner=0, **BASE)
        fill(G, g)
        G.set_devices([0] * 4)
        G.initialize()
        assert L.device_memory_in_use()[0] > before[0]
        out = read(G, G.optimize(3))
        G.close()
        return out

    first = run()
    assert L.device_memory_in_use() == before
    same(first, run())
    assert L.device_memory_in_use() == before


def test_per_rank_read_outs():
    g = small_graph()
    world = 4

    def drive(G):
        return dict(rows=G.local_rows(), bytes=G.device_bytes())

    S = L.Graph(preconditioner=0, **BASE)
    fill(S, g)
    S.set_devices([0] * world)
    S.initialize()
    nb = S.system_dims()[0]
    rows = [S.local_rows_of_rank(r) for r in range(world)]
    byts = [S.device_bytes_of_rank(r) for r in range(world)]
    assert S.local_rows() == rows[0] and S.device_bytes() == byts[0]
    assert code_of(lambda: S.local_rows_of_rank(world)) == L.ERR_ARG
    S.close()
    _, ranks = both(world, g, dict(preconditioner=0, **BASE), drive)
    assert rows[0][0] == 0 and rows[-1][1] == nb
    assert all(a[1] == b[0] for a, b in zip(rows[:-1], rows[1:]))
    assert rows == [r["rows"] for r in ranks]
    assert sum(b[0] for b in byts) == sum(r["bytes"][0] for r in ranks)
    assert sum(b[1] for b in byts) == sum(r["bytes"][1] for r in ranks)


def test_a_failed_rank_finishes_the_handle():
    """A rank whose engine call fails aborts the group's barrier: the call returns that rank's code, the handle then
    answers ERR_STATE, and destroying it does not hang.  (The failure is a refusal on the host -- the exact
    factorisation is not partitioned -- which every rank meets before its first collective.)"""
    g = small_graph()
    G = L.Graph(linear_solver=1, **BASE)
    fill(G, g)
    G.set_devices([0, 0], timeout_s=5.0)
    assert code_of(G.initialize) == L.ERR_ARG
    assert code_of(G.initialize) == L.ERR_STATE
    assert code_of(G.chi2) == L.ERR_STATE
    assert code_of(G.get_vertices) == L.ERR_STATE
    assert code_of(lambda: G.set_options(linear_solver=0)) == L.ERR_STATE
    with pytest.raises(L.Sim3OptError, match="finished"):
        G.optimize(1)
    G.close()
    # ... and the next handle is none the worse for it
    H2 = L.Graph(preconditioner=0, **BASE)
    fill(H2, g)
    H2.set_devices([0, 0])
    H2.initialize()
    assert H2.optimize(1) == 1
    H2.close()
