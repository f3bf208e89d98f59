"""The collectives of the in-process transport (csrc/comm_local.hip, csrc/comm_kernels.hpp: k_comm_put, k_comm_unpack,
k_comm_reduce, two alternating mailboxes per rank, a host barrier, the exchange's second round) as OPERATORS: one
collective at a time on chosen operands through sim3opt_comm_apply_*, read off the device, against the numpy
restatement tests/comm_ref.py on the cases of tests/comm_cases.py.  tests/test_comm_ref.py shows without a GPU that
these cases see every defect of comm_ref.DEFECTS.

Every comparison is on bits (np.array_equal on .view(np.uint64): NaN payloads and -0.0 count).  No tolerance is
needed: copies are copies, the reduce is a fixed-order fold with contraction off, and float64 addition and comparison
are the same on host and device.  A guard double next to an operand that changes fails the call itself
(Sim3OptError).  Next to every result the mailbox capacity and the collective count are compared with what
comm_ref.Transport predicts from the state read before the call (Graph.comm_local_state), which is how a case's path
through growth, rounds and parity is asserted rather than assumed.  All ranks run on device 0 (a repeated ordinal)."""
import ctypes as C_

import numpy as np
import pytest
import torch

import comm_cases as C
import comm_ref as R
from sim3opt_amd import lib as L, synth

pytestmark = pytest.mark.gpu

BASE = dict(preconditioner=0, fix_small_angle_b=1, fd_delta=1e-6, pcg_rel_tol=1e-12)
I64P = C_.POINTER(C_.c_int64)
DP = C_.POINTER(C_.c_double)


def tiny_graph():
    synth.DRIFT_TARGET = 0.05
    return synth.chain_loop(40, 52, seed_graph=411, seed_noise=412, min_gap=5)


def make(world, devices=None, initialize=True, **opts):
    g = tiny_graph()
    G = L.Graph(**dict(BASE, **opts))
    G.add_vertices(g["states"], g["fixed"])
    G.add_edges(g["v0"], g["v1"], g["meas"])
    G.set_devices(devices if devices is not None else [0] * world)
    if initialize:
        G.initialize()
    return G


@pytest.fixture(scope="module")
def handles():
    """one handle per world for the whole file"""
    made = {}

    def get(world):
        if world not in made:
            made[world] = make(world)
        return made[world]

    yield get
    for G in made.values():
        G.close()


def code_of(call):
    with pytest.raises(L.Sim3OptError) as e:
        call()
    return e.value.code


def check_step(G, step, name=""):
    """one collective on the device against the restatement; the state after it against the model's"""
    world = G.rank_count()
    cap0, seq0 = G.comm_local_state()
    T = R.Transport(world, cap=cap0, seq=seq0)
    model = C.run_on_model(T, step)
    exp = C.expected(step)
    got = C.run_on_graph(G, step)
    assert len(got) == world
    for r in range(world):
        assert R.same_bits(model[r], exp[r])
        assert R.same_bits(got[r], exp[r]), (name, step["kind"], "rank", r,
                                             np.flatnonzero(R.bits(got[r]) != R.bits(exp[r]))[:8])
    assert G.comm_local_state() == (T.cap, T.seq), (name, cap0, seq0)
    if step["kind"] == "allgatherv":
        offs = step["offs"]
        for r in range(world):
            assert R.same_bits(got[r][offs[r]:offs[r + 1]], step["rows"][r][offs[r]:offs[r + 1]])  # its own span
            assert not (R.bits(got[r]) == R.bits(C.SENTINEL)).any()  # no sentinel survives outside it
    if step["kind"] == "exchange":
        for r in range(world):
            lead = step["roffs"][r][0]
            assert R.same_bits(got[r][:lead], step["recv"][r][:lead])  # what no segment covers keeps its pre-fill
    return T


def run_scenarios(G, scs):
    for sc in scs:
        for st in sc["steps"]:
            check_step(G, st, sc["name"])


# ------------------------------------------------------------------------------------------------------ all-reduce
@pytest.mark.parametrize("world", C.WORLDS)
def test_allreduce_small(handles, world):
    G = handles(world)
    scs = C.allreduce_small(world)
    assert len(scs) == len(C.ALLREDUCE_NS) * 4
    for sc in scs:
        st = sc["steps"][0]
        n = st["rows"].shape[1]
        p = R.span_path(0, R.GUARD_DOUBLES + st["phase"], n, R.copy_grid(n))  # the put: slot (even) <- operand
        assert p["same_phase"] == (st["phase"] == 0) and p["head"] == 0 and (st["phase"] or p["tail"] == n % 2)
    run_scenarios(G, scs)


def test_allreduce_long_wraps_the_reduce(handles):
    scs = C.allreduce_long(3)
    n = C.ALLREDUCE_LONG_N
    assert n > R.reduce_grid(n) * R.COMM_WG  # k_comm_reduce goes round again
    assert R.span_path(0, R.GUARD_DOUBLES + 1, n, R.copy_grid(n))["sweeps"] == 2  # ... and the put's scalar loop
    assert [s["steps"][0]["phase"] for s in scs] == [0, 1] and all(s["steps"][0]["rows"].shape == (3, n) for s in scs)
    run_scenarios(handles(3), scs)


# ------------------------------------------------------------------------------------------------------ all-gather
@pytest.mark.parametrize("world", C.WORLDS)
def test_allgather_small(handles, world):
    scs = C.allgather_small(world)
    heads = tails = 0
    for sc in scs:
        st = sc["steps"][0]
        for r in range(world):
            lo, n = st["offs"][r], st["offs"][r + 1] - st["offs"][r]
            p = R.span_path(lo, R.GUARD_DOUBLES + st["phase"] + lo, n, R.copy_grid(max(n, 1)))
            assert n == 0 or p["same_phase"] == (st["phase"] == 0)
            heads += p["head"]
            tails += p["tail"]
    assert heads and tails
    run_scenarios(handles(world), scs)


def test_allgather_long_wraps_the_copy(handles):
    scs = C.allgather_long(2)
    for sc, head in zip(scs, (0, 1)):
        st = sc["steps"][0]
        lo, n = max(((st["offs"][r], st["offs"][r + 1] - st["offs"][r]) for r in range(2)), key=lambda x: x[1])
        p = R.span_path(lo, R.GUARD_DOUBLES + st["phase"] + lo, n, R.copy_grid(n))
        assert p["same_phase"] and p["head"] == head and p["pairs"] > R.COMM_MAX_GRID_X * R.COMM_WG and p["sweeps"] == 2
    run_scenarios(handles(2), scs)


# -------------------------------------------------------------------------------------------------------- exchange
@pytest.mark.parametrize("world", C.WORLDS)
def test_exchange_small(handles, world):
    G = handles(world)
    scs = C.exchange_small(world)
    assert {(s["steps"][0]["send_phase"], s["steps"][0]["recv_phase"]) for s in scs} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    # the mailboxes hold every segment already (no second round here: that is test_exchange_growth's)
    G.comm_apply_allreduce(np.zeros((world, 16)))
    cap = G.comm_local_state()[0]
    for sc in scs:
        assert all(C.growth_facts(sc["steps"][0], world, cap)["fits"])
    run_scenarios(G, scs)


@pytest.mark.parametrize("world", [3, 8])
def test_exchange_growth(world):
    """One rank's segment is beyond the slot: the ranks that fit put in round 0, all grow, round 1 runs the collective
    again (three barriers); the same exchange once more is one barrier.  A fresh handle: the capacity is what
    initialisation left -- or, where that is no mailbox at all, what one 1-double all-reduce leaves."""
    G = make(world)
    try:
        if G.comm_local_state()[0] == 0:
            G.comm_apply_allreduce(np.ones((world, 1)))
        cap, seq = G.comm_local_state()
        assert cap > 0
        step = C.growth_step(world, cap)
        f = C.growth_facts(step, world, cap)
        counts = C.growth_counts(world, cap)
        assert counts.max() == cap // world + 2 > ((cap // world) & ~1) and (counts > 2).sum() == 1
        assert f["fits"].count(False) == 2 and f["fits"].count(True) == world - 2 and max(f["need"]) > cap
        check_step(G, step, "growth")
        cap1, seq1 = G.comm_local_state()
        assert cap1 > cap and cap1 >= max(f["need"]) and seq1 == seq + 3
        again = C.growth_step(world, cap, seed=4001)
        check_step(G, again, "after growth")
        assert G.comm_local_state() == (cap1, seq1 + 1)
        assert G.optimize(1) == 1
    finally:
        G.close()


# ------------------------------------------------------------------------------------------------------- sequences
@pytest.mark.parametrize("world", C.WORLDS)
@pytest.mark.parametrize("start", [0, 1])
def test_sequences_from_both_parities(handles, world, start):
    G = handles(world)
    sc = C.sequences(world)[start]
    G.comm_apply_allgatherv(sc["steps"][-5]["offs"], sc["steps"][-5]["rows"])  # (the mailboxes have their size)
    flip = C.allreduce_step(world, 1, 0, 0, 5556)
    if (G.comm_local_state()[1] & 1) != 0:
        check_step(G, flip, "to an even count")
    assert G.comm_local_state()[1] & 1 == 0
    first = len(sc["steps"]) - 5
    for k, st in enumerate(sc["steps"]):
        if k == first:
            assert G.comm_local_state()[1] & 1 == start == sc["start_parity"]
        T = check_step(G, st, sc["name"])
        assert T.seq == G.comm_local_state()[1]
    assert G.comm_local_state()[1] & 1 == (start + 5) & 1


# ------------------------------------------------------------------------------------------- the rest of the handle
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


def test_nothing_else_changes():
    world = 3
    A, B = make(world), make(world)
    try:
        assert A.comm_local_state() == B.comm_local_state()
        for st in C.sequences(world)[0]["steps"]:
            check_step(A, st, "before optimize")
        if (A.comm_local_state()[1] - B.comm_local_state()[1]) % 2 == 0:
            check_step(A, C.allreduce_step(world, 1, 0, 0, 5557), "an odd number in all")
        assert (A.comm_local_state()[1] - B.comm_local_state()[1]) % 2 == 1
        ra, rb = read(A, A.optimize(3)), read(B, B.optimize(3))
        assert ra["n"] == 3
        same(ra, rb)
    finally:
        A.close()
        B.close()


def test_timing_counters_count_the_applied_collectives():
    world = 3
    G = make(world, time_kernels=1)
    try:
        steps = C.sequences(world)[1]["steps"]
        t0 = G.comm_times()
        for st in steps:
            check_step(G, st, "timed")
        t1 = G.comm_times()
        kinds = [st["kind"] for st in steps]
        assert t1["n_allreduce"] - t0["n_allreduce"] == kinds.count("allreduce") == 3
        assert t1["n_allgather"] - t0["n_allgather"] == kinds.count("allgatherv") == 2
        assert t1["n_exchange"] - t0["n_exchange"] == kinds.count("exchange") == 1
        ex = [st for st in steps if st["kind"] == "exchange"][0]
        moved = ex["soffs"][0][-1] + ex["roffs"][0][-1]  # rank 0's buffers (they start at 0 here)
        assert ex["soffs"][0][0] == 0 and ex["roffs"][0][0] == 0 and moved > 0
        assert t1["bytes_exchange"] - t0["bytes_exchange"] == 8 * moved
    finally:
        G.close()


def test_applied_collectives_keep_no_device_memory():
    before = L.device_memory_in_use()
    world = 3
    G = make(world)
    steps = C.sequences(world)[0]["steps"]
    for st in steps:  # warm-up: the mailboxes grow to what these need
        check_step(G, st, "warm-up")
    for st in steps:
        held = L.device_memory_in_use()
        check_step(G, st, "steady")
        assert L.device_memory_in_use() == held
    G.close()
    assert L.device_memory_in_use() == before


# -------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_handle_in_step(handles):
    world = 3
    G = handles(world)
    lib, g = G._L, G._g
    n = 4
    a, out = np.arange(world * n, dtype=np.float64), np.zeros(world * n)
    pa, po = a.ctypes.data_as(DP), out.ctypes.data_as(DP)
    offs = np.array([0, 2, 3, 4], dtype=np.int64)
    bad_offs = np.array([0, 3, 2, 4], dtype=np.int64)
    late_offs = np.array([1, 2, 3, 4], dtype=np.int64)
    po64 = lambda v: v.ctypes.data_as(I64P)
    st = C.exchange_small(world)[0]["steps"][0]
    so, ro = np.array(st["soffs"], dtype=np.int64), np.array(st["roffs"], dtype=np.int64)
    send, recv = np.concatenate(st["send"]), np.concatenate(st["recv"])
    ps, pr = send.ctypes.data_as(DP), recv.ctypes.data_as(DP)
    ro_bad = ro.copy()
    ro_bad[2, 1:] += 1  # rank 2 expects one more double from rank 0 than rank 0 sends
    so_down = so.copy()
    so_down[1, 2] = so_down[1, 1] - 1
    state = G.comm_local_state()
    recv0 = recv.copy()
    arg = [
        lambda: lib.sim3opt_comm_apply_allreduce(g, -1, 0, 0, pa, po),
        lambda: lib.sim3opt_comm_apply_allreduce(g, n, 0, 2, pa, po),
        lambda: lib.sim3opt_comm_apply_allreduce(g, n, 0, -1, pa, po),
        lambda: lib.sim3opt_comm_apply_allreduce(g, n, 2, 0, pa, po),
        lambda: lib.sim3opt_comm_apply_allreduce(g, n, 0, 0, None, po),
        lambda: lib.sim3opt_comm_apply_allreduce(g, n, 0, 0, pa, None),
        lambda: lib.sim3opt_comm_apply_allgatherv(g, po64(bad_offs), 0, pa, po),
        lambda: lib.sim3opt_comm_apply_allgatherv(g, po64(late_offs), 0, pa, po),
        lambda: lib.sim3opt_comm_apply_allgatherv(g, po64(offs), 3, pa, po),
        lambda: lib.sim3opt_comm_apply_allgatherv(g, None, 0, pa, po),
        lambda: lib.sim3opt_comm_apply_allgatherv(g, po64(offs), 0, None, po),
        lambda: lib.sim3opt_comm_apply_exchange(g, po64(so), po64(ro_bad), 0, 0, ps, pr),
        lambda: lib.sim3opt_comm_apply_exchange(g, po64(so_down), po64(ro), 0, 0, ps, pr),
        lambda: lib.sim3opt_comm_apply_exchange(g, po64(so), po64(ro), 2, 0, ps, pr),
        lambda: lib.sim3opt_comm_apply_exchange(g, po64(so), po64(ro), 0, -1, ps, pr),
        lambda: lib.sim3opt_comm_apply_exchange(g, None, po64(ro), 0, 0, ps, pr),
        lambda: lib.sim3opt_comm_apply_exchange(g, po64(so), po64(ro), 0, 0, ps, None),
    ]
    for k, call in enumerate(arg):
        assert call() == L.ERR_ARG, k
        assert G.comm_local_state() == state, k  # nobody entered a collective
    assert lib.sim3opt_comm_apply_exchange(g, po64(so), po64(ro_bad), 0, 0, ps, pr) == L.ERR_ARG
    assert b"disagree" in lib.sim3opt_last_error(g)
    assert lib.sim3opt_comm_local_state(g, None) == L.ERR_ARG
    assert G.comm_local_state() == state and np.array_equal(recv, recv0)
    # ... and the handle is none the worse: empty operands are valid, a real collective is right, an optimisation runs
    for empty in (dict(kind="allreduce", rows=np.zeros((world, 0)), op=0, phase=1),
                  dict(kind="allgatherv", offs=[0] * (world + 1), rows=np.zeros((world, 0)), phase=0)):
        check_step(G, empty, "empty")
    assert G.comm_local_state() == (state[0], state[1] + 2)
    run_scenarios(G, C.exchange_small(world)[:2])
    assert G.optimize(1) == 1

    # handles that have no ranks of their own, or are not initialised, or are finished
    row = np.ones((1, 3))
    P = L.Graph(**BASE)
    t = tiny_graph()
    P.add_vertices(t["states"], t["fixed"])
    P.add_edges(t["v0"], t["v1"], t["meas"])
    assert code_of(lambda: P.comm_apply_allreduce(row)) == L.ERR_STATE  # not initialised, one rank
    P.initialize()
    assert code_of(lambda: P.comm_apply_allreduce(row)) == L.ERR_STATE  # one rank
    assert code_of(P.comm_local_state) == L.ERR_STATE
    assert P.optimize(1) == 1
    P.close()
    S = make(1)
    assert code_of(lambda: S.comm_apply_allreduce(row)) == L.ERR_STATE  # set_devices with one device: the plain graph
    S.close()
    U = make(2, initialize=False)
    rows2 = np.ones((2, 3))
    assert code_of(lambda: U.comm_apply_allreduce(rows2)) == L.ERR_STATE  # ranks, but no engines yet
    assert code_of(lambda: U.comm_apply_allgatherv([0, 1, 3], rows2)) == L.ERR_STATE
    assert code_of(U.comm_local_state) == L.ERR_STATE
    U.initialize()
    assert R.same_bits(U.comm_apply_allreduce(rows2), 2.0 * rows2)
    U.close()
    F = make(2, initialize=False, linear_solver=1)  # (the exact factorisation is not partitioned: every rank refuses on the host)
    assert code_of(F.initialize) == L.ERR_ARG
    assert code_of(lambda: F.comm_apply_allreduce(rows2)) == L.ERR_STATE
    assert code_of(F.comm_local_state) == L.ERR_STATE
    F.close()


# ------------------------------------------------------------------------------------------------ distinct devices
def test_two_distinct_devices():
    if torch.cuda.device_count() < 2:
        pytest.skip("one HIP device: the ranks of this file share it")
    G = make(2, devices=[0, 1], initialize=False)
    try:
        try:
            G.initialize()
        except L.Sim3OptError as e:
            if e.code == L.ERR_COMM and "peer access" in str(e):
                pytest.skip(str(e))
            raise
        run_scenarios(G, C.allreduce_small(2))
        run_scenarios(G, C.exchange_small(2))
    finally:
        G.close()
