"""Robust kernels beyond Huber, host side (no GPU): the formulas of sim3opt_robustify against a numpy restatement
of the table in include/sim3opt.h, w = rho' against central differences, the argument checks of
sim3opt_add_edge / sim3opt_set_edge_kernels, and the host part of the g2o-named shim's RobustKernel classes
(tests/cxx/robust_conformance.cpp)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from sim3opt_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I8 = [0, 0, 0, 1, 0, 0, 0, 1.0]
KINDS = list(range(10))
DELTAS = [0.1, 1.0, 30.0]


def ref(kind, d, e2):
    """The table of include/sim3opt.h, operation for operation."""
    d2 = d * d
    if kind == L.KERNEL_NONE:
        return e2, 1.0
    if kind == L.KERNEL_HUBER:
        if e2 <= d2:
            return e2, 1.0
        sq = math.sqrt(e2)
        return 2 * sq * d - d2, d / sq
    if kind == L.KERNEL_PSEUDO_HUBER:
        r = math.sqrt(1.0 + e2 / d2)
        return 2.0 * d2 * (r - 1.0), 1.0 / r
    if kind == L.KERNEL_CAUCHY:
        a = 1.0 + e2 / d2
        return d2 * math.log(a), 1.0 / a
    if kind == L.KERNEL_GEMAN_MCCLURE:
        a = d + e2
        return d * e2 / a, d2 / (a * a)
    if kind == L.KERNEL_WELSCH:
        x = math.exp(-e2 / d2)
        return d2 * (1.0 - x), x
    if kind == L.KERNEL_FAIR:
        a = math.sqrt(e2) / d
        return 2.0 * d2 * (a - math.log(1.0 + a)), 1.0 / (1.0 + a)
    if kind == L.KERNEL_TUKEY:
        if e2 <= d2:
            a = 1.0 - e2 / d2
            return d2 / 3.0 * (1.0 - a * a * a), a * a
        return d2 / 3.0, 0.0
    if kind == L.KERNEL_SATURATED:
        return (e2, 1.0) if e2 <= d2 else (d2, 0.0)
    if kind == L.KERNEL_DCS:
        s = 2.0 * d / (d + e2)
        return (e2, 1.0) if s >= 1.0 else (s * s * e2, s * s)
    raise ValueError(kind)


def e2_points(d):
    d2 = d * d
    return [0.0, 1e-3 * d2, 0.5 * d2, d2, 2.0 * d2, 50.0 * d2, 1e12]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", DELTAS)
def test_robustify_matches_the_table(kind, d):
    for e2 in e2_points(d):
        rho, w = L.robustify(kind, d, e2)
        rr, rw = ref(kind, d, e2)
        assert abs(rho - rr) <= 1e-14 * abs(rr) + 1e-300, (kind, d, e2, rho, rr)
        assert abs(w - rw) <= 1e-14 * abs(rw) + 1e-300, (kind, d, e2, w, rw)


@pytest.mark.parametrize("kind", [k for k in KINDS if k != L.KERNEL_DCS])
@pytest.mark.parametrize("d", DELTAS)
def test_weight_is_the_derivative_of_rho(kind, d):
    # DCS is left out: its rho is not the integral of its w (g2o's definition)
    for x in (0.05, 0.3, 0.7, 1.6, 4.0, 40.0):  # away from the kinks at e2 = d^2
        e2 = x * d * d
        h = 1e-5 * e2
        num = (L.robustify(kind, d, e2 + h)[0] - L.robustify(kind, d, e2 - h)[0]) / (2 * h)
        w = L.robustify(kind, d, e2)[1]
        assert abs(num - w) <= 1e-6 * max(abs(w), 1e-3), (kind, d, e2, num, w)


@pytest.mark.parametrize("kind", KINDS)
def test_weights_in_unit_interval_and_rho_below_e2(kind):
    for d in DELTAS:
        grid = [0.0] + list(np.logspace(-6, 14, 81) * d * d) + [d * d]
        for e2 in grid:
            rho, w = L.robustify(kind, d, e2)
            assert 0.0 <= w <= 1.0, (kind, d, e2, w)
            # (small e2: rho ~ e2 (1 - O(e2/d^2)), computed through a cancellation -- a rounding's worth of slack)
            assert 0.0 <= rho <= e2 * (1 + 1e-9), (kind, d, e2, rho)


def test_robustify_rejects_bad_arguments():
    lib = L.load()
    out = np.empty(2)
    p = out.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.sim3opt_robustify(L.KERNEL_CAUCHY, 1.0, 1.0, p) == L.OK
    for kind, d, e2 in [(-1, 1.0, 1.0), (10, 1.0, 1.0), (L.KERNEL_CAUCHY, 0.0, 1.0), (L.KERNEL_HUBER, -1.0, 1.0),
                        (L.KERNEL_DCS, float("nan"), 1.0), (L.KERNEL_TUKEY, float("inf"), 1.0),
                        (L.KERNEL_WELSCH, 1.0, -1.0), (L.KERNEL_FAIR, 1.0, float("nan"))]:
        assert lib.sim3opt_robustify(kind, d, e2, p) == L.ERR_ARG, (kind, d, e2)
    assert lib.sim3opt_robustify(L.KERNEL_NONE, 0.0, 2.0, p) == L.OK and list(out) == [2.0, 1.0]
    assert lib.sim3opt_robustify(L.KERNEL_CAUCHY, 1.0, 1.0, None) == L.ERR_ARG
    assert L.load().sim3opt_version() == 130


def small_graph(m=6):
    G = L.Graph()
    for i in range(4):
        G.add_vertex(i, I8, fixed=(i == 0))
    for k in range(m):
        G.add_edge(k % 4, (k + 1) % 4, I8)
    return G


def test_add_edge_accepts_every_kind_and_round_trips():
    G = small_graph(0)
    for kind in KINDS:
        G.add_edge(kind % 4, (kind + 1) % 4, I8, kernel=kind, kernel_delta=0.5 + kind)
    kinds, deltas = G.edge_kernels()
    assert list(kinds) == KINDS
    assert list(deltas) == [0.0] + [0.5 + k for k in KINDS[1:]]  # NONE stores no delta
    # per-edge arrays in add_edges
    G.add_edges([0, 1, 2], [1, 2, 3], np.tile(I8, (3, 1)), kernel=[L.KERNEL_DCS, L.KERNEL_NONE, L.KERNEL_TUKEY],
                kernel_delta=[2.0, 0.0, 3.0])
    kinds, deltas = G.edge_kernels()
    assert list(kinds[10:]) == [L.KERNEL_DCS, L.KERNEL_NONE, L.KERNEL_TUKEY]
    assert list(deltas[10:]) == [2.0, 0.0, 3.0]
    # a kernel-free graph reads NONE everywhere
    k0, d0 = small_graph(3).edge_kernels()
    assert list(k0) == [0, 0, 0] and list(d0) == [0.0, 0.0, 0.0]


def test_add_edge_rejects_bad_kernels():
    G = small_graph(2)
    for kind, d in [(-1, 1.0), (10, 1.0), (L.KERNEL_CAUCHY, 0.0), (L.KERNEL_GEMAN_MCCLURE, -2.0),
                    (L.KERNEL_WELSCH, float("nan")), (L.KERNEL_FAIR, float("inf"))]:
        with pytest.raises(L.Sim3OptError) as ei:
            G.add_edge(1, 2, I8, kernel=kind, kernel_delta=d)
        assert ei.value.code == L.ERR_ARG
        with pytest.raises(L.Sim3OptError) as ei:
            G.add_edges([1, 2], [2, 3], np.tile(I8, (2, 1)), kernel=[L.KERNEL_NONE, kind], kernel_delta=[0.0, d])
        assert ei.value.code == L.ERR_ARG
    assert G.num_edges == 2
    assert list(G.edge_kernels()[0]) == [0, 0]


def test_set_edge_kernels_validates_the_whole_call_first():
    G = small_graph(6)
    G.set_edge_kernels([1, 3], [L.KERNEL_CAUCHY, L.KERNEL_DCS], [0.5, 2.0])
    before = G.edge_kernels()
    assert list(before[0]) == [0, 3, 0, 9, 0, 0] and list(before[1]) == [0, 0.5, 0, 2.0, 0, 0]
    lib = L.load()
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)  # noqa: E731
    f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)  # noqa: E731
    ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    bad = [  # (edges, kinds, deltas): the first entry is always valid, so a partial update would show
        ([0, 2], [L.KERNEL_WELSCH, 10], [1.0, 1.0]),
        ([0, 2], [L.KERNEL_WELSCH, -1], [1.0, 1.0]),
        ([0, 2], [L.KERNEL_WELSCH, L.KERNEL_TUKEY], [1.0, 0.0]),
        ([0, 2], [L.KERNEL_WELSCH, L.KERNEL_TUKEY], [1.0, -3.0]),
        ([0, 2], [L.KERNEL_WELSCH, L.KERNEL_TUKEY], [1.0, float("nan")]),
        ([0, 2], [L.KERNEL_WELSCH, L.KERNEL_TUKEY], [1.0, float("inf")]),
        ([0, 6], [L.KERNEL_WELSCH, L.KERNEL_TUKEY], [1.0, 1.0]),
        ([0, -1], [L.KERNEL_WELSCH, L.KERNEL_TUKEY], [1.0, 1.0]),
        (None, [L.KERNEL_WELSCH] * 7, [1.0] * 7),  # NULL edges = 0..n-1, n > m
    ]
    for edges, kinds, deltas in bad:
        e = None if edges is None else i32(edges)
        k, d = i32(kinds), f64(deltas)
        assert lib.sim3opt_set_edge_kernels(G._g, k.shape[0], ip(e), ip(k), dp(d)) == L.ERR_ARG, (edges, kinds, deltas)
        after = G.edge_kernels()
        assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])
        with pytest.raises(L.Sim3OptError) as ei:
            G.set_edge_kernels(edges, kinds, deltas)
        assert ei.value.code == L.ERR_ARG
    assert lib.sim3opt_set_edge_kernels(G._g, -1, None, None, None) == L.ERR_ARG
    assert lib.sim3opt_set_edge_kernels(G._g, 1, None, None, None) == L.ERR_ARG
    assert lib.sim3opt_set_edge_kernels(None, 0, None, None, None) == L.ERR_ARG
    # later entries win; NONE takes no delta (any value is accepted and dropped)
    G.set_edge_kernels([2, 2, 1], [L.KERNEL_TUKEY, L.KERNEL_SATURATED, L.KERNEL_NONE], [4.0, 5.0, float("nan")])
    k, d = G.edge_kernels()
    assert list(k) == [0, 0, 8, 9, 0, 0] and list(d) == [0, 0, 5.0, 2.0, 0, 0]
    # NULL edge list: the first n edges
    G.set_edge_kernels(None, [L.KERNEL_GEMAN_MCCLURE] * 2, [0.25, 0.75])
    k, d = G.edge_kernels()
    assert list(k) == [4, 4, 8, 9, 0, 0] and list(d) == [0.25, 0.75, 5.0, 2.0, 0, 0]


def compile_program(tmp_path):
    exe = str(tmp_path / "robust_conformance")
    libdir = os.path.join(ROOT, "sim3opt_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-DSIM3OPT_G2O_NAMES",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "mock_eigen"),
                           os.path.join(ROOT, "tests", "cxx", "robust_conformance.cpp"), "-L" + libdir,
                           "-lsim3opt", "-Wl,-rpath," + libdir, "-o", exe])
    return exe


def test_robust_shim_host_part(tmp_path):
    r = subprocess.run([compile_program(tmp_path), "host"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout
