"""GPU tests (-m gpu) of the vector kernels of the columns of the inverse as operators: k_cols_rhs<K>, k_cols_residual,
k_cols_axpy and k_cols_gather (col_kernels.hpp) are launched once each on a caller's data in the buffers a column solve
uses (Graph.debug_column_vectors) and compared with numpy BIT FOR BIT: every entry they write is a copy, a constant or
one correctly rounded sum or difference.  In a solve they sit under PCG iterations and a refinement loop that forgives
errors: a lost odd tail, a unit entry in the wrong system or a block written at the wrong stride shows there, if at
all, as one more refinement round.

The path conditions (asserted from the inputs): the double2 body with and without the odd tail (n odd and even), n / 2
either side of one workgroup's 256 lanes, the stride loop (one workgroup) and a solve's own grid, unit entries at both
ends, on the tail and absent, every K and system base, gathers of less than a workgroup's lanes, of more, and with
repeated rows."""
import ctypes

import numpy as np
import pytest

from sim3opt_amd import lib as L
import dogleg_cases as DC
import lm_cases as C

pytestmark = pytest.mark.gpu
WG = DC.WG
LENGTHS = (1, 2, 3, 510, 511, 512, 513, 514, 515, 560)
PRE = 1000.0  # what the output buffers hold before a launch: PRE (system + 1) + index + 0.5, no entry of it 0 or 1

_G = {}


def graph():
    if "G" not in _G:
        g = DC.graph("columns")
        nb, n = DC.check_graph("columns", g)
        G = C.make(L, g, fd_delta=1e-6, linear_solver=0, preconditioner=0)
        G.linearize()
        assert G.linear_solver_in_use() == 0 and n == 560 == max(LENGTHS) and G.column_vector_stride() == 576
        _G["G"] = G
    return _G["G"]


def prefill(K, vs):
    return PRE * (np.arange(K)[:, None] + 1) + np.arange(vs)[None, :] + 0.5


def test_the_lengths_cover_the_paths():
    halves = sorted({n // 2 for n in LENGTHS})
    assert {255, 256, 257} <= set(halves) and 0 in halves           # n / 2 around one workgroup; no double2 at all
    for h in (255, 256, 257):
        assert 2 * h in LENGTHS and 2 * h + 1 in LENGTHS             # each with and without the odd tail
    assert (560 // 2 + WG - 1) // WG == 2                            # a solve's own grid: two workgroups on 7 x 80 rows


@pytest.mark.parametrize("grid", [0, 1], ids=["own_grid", "one_workgroup"])
@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_rhs_clears_k_vectors_and_sets_their_unit_entries(K, grid):
    G = graph()
    vs = G.column_vector_stride()
    pre = prefill(K, vs)
    for n in LENGTHS:
        odd = max(1, n // 2) | 1
        spots = [0, odd if odd < n else 0, max(n - 2, 0), n - 1, -1]  # first, an odd index, n - 2, n - 1 (the tail), none
        assert n < 4 or (spots[1] % 2 == 1 and len(set(spots)) == 5)
        for off in range(5):
            at = [spots[(off + s) % 5] for s in range(K)]
            out = G.debug_column_vectors("rhs", n, pre, grid=grid, at=at)
            want = pre.copy()
            want[:, :n] = 0.0
            for s, a in enumerate(at):
                if a >= 0:
                    want[s, a] = 1.0
            assert np.array_equal(out, want), (n, K, grid, at, np.argwhere(out != want)[:5])  # (n .. vs untouched too)


@pytest.mark.parametrize("grid", [0, 1], ids=["own_grid", "one_workgroup"])
@pytest.mark.parametrize("kernel", ["residual", "axpy"])
def test_residual_and_axpy_entry_by_entry(kernel, grid):
    G = graph()
    vs = G.column_vector_stride()
    rng = np.random.default_rng(91)
    for n in LENGTHS:
        for system in (0, 3):  # the first and the last base: a wrong stride or base lands in another system
            a = rng.standard_normal(n) * 10.0 ** rng.uniform(-8, 8, n)
            b = rng.standard_normal(n) * 10.0 ** rng.uniform(-8, 8, n)
            pre = prefill(1, vs)[0]
            want = pre.copy()
            if kernel == "residual":
                out = G.debug_column_vectors("residual", n, pre, grid=grid, a=a, b=b, system=system)
                want[:n] = a - b
            else:
                pre[:n] = b
                out = G.debug_column_vectors("axpy", n, pre, grid=grid, a=a, system=system)
                want[:n] = b + a
            assert np.array_equal(out, want), (kernel, n, grid, system, np.argwhere(out != want)[:5])


@pytest.mark.parametrize("grid", [0, 1], ids=["own_grid", "one_workgroup"])
@pytest.mark.parametrize("count", [1, 36, 37, 300])
def test_gather_scatters_into_the_blocks_column(count, grid):
    """7 count lanes: 7 (less than a wavefront), 252 and 259 (either side of one workgroup), 2100 (nine workgroups; one
    workgroup strides nine times).  first > 0; rows with repeats and the largest row; every column."""
    G = graph()
    rng = np.random.default_rng(92 + count)
    n, first = 560, 5
    nblk = first + count + 3
    rows = rng.integers(0, 80, first + count).astype(np.int32)
    rows[first + count // 2] = 79
    if count > 1:
        rows[first] = rows[first + count - 1] = 17
        assert len(set(rows[first:].tolist())) < count and rows[first:].max() == 79
    rows[:first] = 79  # (never read: blocks before `first` belong to other vertices)
    y = rng.standard_normal(n)
    pre = prefill(nblk, 49)
    for col in range(7):
        out = G.debug_column_vectors("gather", n, pre, grid=grid, a=y, first=first, count=count, col=col, rows=rows,
                                     system=col % 4)
        want = pre.copy()
        for k in range(first, first + count):
            want[k, 7 * col:7 * col + 7] = y[7 * rows[k]:7 * rows[k] + 7]
        assert np.array_equal(out, want), (count, grid, col, np.argwhere(out != want)[:5])
    # a shorter vector (its last row is the largest a caller may name), and nothing to gather
    n = 511
    out = G.debug_column_vectors("gather", n, pre, grid=grid, a=y[:n], first=2, count=1, col=6, rows=[0, 0, 72])
    want = pre.copy()
    want[2, 42:49] = y[504:511]
    assert np.array_equal(out, want)
    assert np.array_equal(G.debug_column_vectors("gather", n, pre, grid=grid, a=y[:n], first=2, count=0, rows=[0, 0]), pre)


def test_column_read_out_refuses_what_it_cannot_do():
    lib = L.load()
    dp, ip, lp = (ctypes.POINTER(t) for t in (ctypes.c_double, ctypes.c_int32, ctypes.c_int64))
    g = DC.graph("columns")

    def fresh(**o):
        G = L.Graph(fd_delta=1e-6, **o)
        G.add_vertices(g["states"], g["fixed"])
        G.add_edges(g["v0"], g["v1"], g["meas"])
        return G

    G = fresh(linear_solver=0)
    n, vs = 560, 576
    out, a, b = np.ones(4 * vs), np.ones(n), np.ones(n)
    at = np.array([0, 1, 2, 3], dtype=np.int64)
    rows = np.zeros(8, dtype=np.int32)
    P = lambda x, t=dp: x.ctypes.data_as(t) if x is not None else None

    def call(kernel=2, grid=0, n_=n, K=0, at_=None, system=0, a_=a, b_=None, first=0, count=0, col=0, rows_=None, nblk=0,
             out_=out, G_=None):
        return lib.sim3opt_debug_column_vectors((G_ or G)._g, kernel, grid, n_, K, P(at_, lp), system, P(a_), P(b_), first,
                                                count, col, P(rows_, ip), nblk, P(out_))

    err = lambda G_=None: lib.sim3opt_last_error((G_ or G)._g)
    assert call() == L.ERR_STATE and b"initialize" in err()
    G.initialize()
    assert call(out_=None) == L.ERR_ARG and b"null output" in err()
    assert call() == L.ERR_STATE and b"linearize" in err()
    G.linearize()
    for grid in (-1, DC.MAX_GRID + 1):
        assert call(grid=grid) == L.ERR_ARG and b"grid out of range" in err()
    assert call(kernel=4) == L.ERR_ARG and call(kernel=-1) == L.ERR_ARG and b"unknown kernel" in err()
    for bad in (0, n + 1):
        assert call(n_=bad) == L.ERR_ARG and b"vector length out of range" in err()
    for K in (0, 5):
        assert call(kernel=0, K=K, at_=at) == L.ERR_ARG and b"1 .. 4 systems" in err()
    assert call(kernel=0, K=2, at_=None) == L.ERR_ARG
    assert call(kernel=0, K=2, at_=np.array([0, n], dtype=np.int64)) == L.ERR_ARG and b"past the end" in err()
    for system in (-1, 4):
        assert call(system=system) == L.ERR_ARG and b"system index out of range" in err()
    assert call(a_=None) == L.ERR_ARG and call(kernel=1, b_=None) == L.ERR_ARG
    g3 = dict(kernel=3, rows_=rows, nblk=8)
    assert call(**g3, first=5, count=4) == L.ERR_ARG and b"must lie in the output" in err()
    assert call(**g3, first=-1, count=1) == L.ERR_ARG and call(**g3, count=-1) == L.ERR_ARG
    assert call(**g3, count=1, col=7) == L.ERR_ARG and call(kernel=3, nblk=8, count=1) == L.ERR_ARG
    rows[3] = 80
    assert call(**g3, count=4) == L.ERR_ARG and b"a row past the end" in err()
    assert call(**g3, count=3) == L.OK and call() == L.OK and call(kernel=1, b_=b) == L.OK
    assert call(kernel=0, K=4, at_=at, grid=DC.MAX_GRID) == L.OK
    # where the columns are refused: a graph that factorises exactly
    E = fresh(linear_solver=1)
    E.initialize()
    E.linearize()
    assert E.linear_solver_in_use() == 1
    assert call(G_=E) == L.ERR_STATE and b"factorises exactly" in err(E)
    assert lib.sim3opt_version() == 130  # diagnostics are not part of the versioned interface
