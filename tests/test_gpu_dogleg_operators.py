"""GPU tests (-m gpu) of the dogleg kernels as operators: k_dl_dots, k_dl_sum, k_dl_final and k_dogleg_oplus
(algo_kernels.hpp) are launched once on a caller's h_gn by the code optimize_dogleg runs (Graph.debug_dogleg) and
compared with tests/algorithms_ref.py / tests/lm_ref.py in long double.  The optimiser runs of
tests/test_gpu_algorithms.py accept 1e-7 on the norms and 5e-9 on chi2 on one 240-vertex graph; a dot product wrong
in its last digits, a grid-stride loop, a second pass of sum_partials or a fixed vertex that is not vertex 0 never
show there.

Every case comes with the PATH CONDITION it exists for (tests/dogleg_cases.py), asserted from the inputs.

Two kinds of check:
  derived ...... the six scalars.  The inputs are the device's own H and b bit for bit and the caller's h_gn; the
                 operation is sums of products: |dev - ld| <= gamma(k) x magnitude (the same sum with absolute values:
                 sum |b_i g_i|, sum |v_i| |H_ij| |w_j|), for any summation order and any contraction.  k: a dot of n
                 entries is n products summed, k_sum(n, 1); a quadratic form adds the 7 m products and sums of a row
                 of m blocks behind every entry of H v, 7 m_max + k_sum(n, 1).  A sum whose magnitude is zero (an empty
                 range, h_gn = 0) must be exact.
  measured ..... the estimates after k_dogleg_oplus go through exp: lm_ref.measured_ratio against lm_ref.oplus of
                 ca b + cg h_gn (32 x |float64 restatement - long double|, floored at 4u), as the LM update test.
  exact ........ the backup, fixed vertices, a failed solve's trial, and every later optimize() / covariances().
"""
import ctypes
import functools

import numpy as np
import pytest

from sim3opt_amd import lib as L
import algorithms_ref as A
import amg_ref as R
import dist_helpers as DH
import dogleg_cases as DC
import lm_cases as C
import lm_ref as LR

LD, U = R.LD, R.U
pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not R.longdouble_ok(), reason="np.longdouble has no 64-bit mantissa here")]
BASE = dict(fd_delta=1e-6, linear_solver=0, preconditioner=0)


@pytest.fixture(autouse=True)
def _no_env_knobs(monkeypatch):
    monkeypatch.delenv("SIM3OPT_SPAN_GRID", raising=False)
    monkeypatch.delenv("SIM3OPT_SPMV", raising=False)


@functools.lru_cache(maxsize=None)
def case(name, **options):
    """A linearised graph of a case and its system as the DEVICE holds it, once for all tests of it."""
    g = DC.graph(name)
    nb, n = DC.check_graph(name, g)
    G = C.make(L, g, **{**BASE, **options})
    G.linearize()
    rp, ci, blk, b = G.get_system()
    assert rp.shape[0] - 1 == nb and b.shape[0] == n
    o = G.options()
    mo = LR.mopts(exp_eps=o.exp_eps, small_rot_half=o.small_rot_half, fix_small_angle_b=o.fix_small_angle_b)
    return dict(g=g, G=G, rp=rp, ci=ci, blk=blk, b=b, nb=nb, n=n, mmax=int(np.diff(rp).max()), o=mo)


@functools.lru_cache(maxsize=None)
def reference(name, kind, j0, j1):
    """(h_gn, values, magnitudes) of a vector kind on a case over [j0, j1) (None: everything), once."""
    s = case(name)
    g = DC.vector(kind, s["b"])
    DC.check_vector(kind, s["b"], g)
    val, mag = A.dogleg_scalars(s["rp"], s["ci"], s["blk"], s["b"], g, j0, j1)
    return g, val, mag


def dots_ratios(s, got, val, mag, nr):
    """error / derived bound of the six scalars; nr: entries of the dots' range."""
    kd, kq = LR.k_sum(nr, 1), 7 * s["mmax"] + LR.k_sum(s["n"], 1)
    ks = (kd, kq, kd, kd, 7 * s["mmax"] + kd, kq)
    return [LR.derived_ratio(got[i], val[i], mag[i], ks[i]) for i in range(6)]


def check_dots(name, kind, grid=0, rng=None, s=None, what=""):
    s = s or case(name)
    j0, j1 = rng if rng else (None, None)
    g, val, mag = reference(name, kind, j0, j1)
    got, _, _ = s["G"].debug_dogleg(g, grid=grid, j0=j0 or 0, j1=j1 or 0, states=False)
    r = dots_ratios(s, got, val, mag, s["n"] if rng is None else j1 - j0)
    print(f"[dl-op] {name:9s} {kind:10s} grid {grid:4d} range {str(rng):14s}{what} error / derived bound: "
          + " ".join(f"{x:.1e}" for x in r))
    assert max(r) <= 1.0, (name, kind, grid, rng, r, got, val)
    return got


# ------------------------------------------------------------------------------------------------ the dots
@pytest.mark.parametrize("kind", DC.VECTORS)
@pytest.mark.parametrize("name", ["rows_36", "rows_37"])
def test_dots_of_one_and_of_two_workgroups(name, kind):
    """252 entries: one partly filled workgroup; 259: a second one with 3 entries.  Every vector kind, the whole vector
    and every range of dogleg_cases.ranges (odd starts off every row and workgroup boundary, one entry, empty)."""
    s = case(name)
    got = check_dots(name, kind)
    if kind == "zero":
        assert got[2] == got[3] == got[4] == got[5] == 0.0 and got[0] > 0 and got[1] > 0
    for rng in DC.ranges(s["n"]):
        sub = check_dots(name, kind, rng=rng)
        assert sub[1] == got[1] and sub[5] == got[5]  # the quadratic forms cover every row whatever the range
        if rng[0] == rng[1]:
            assert sub[0] == sub[2] == sub[3] == sub[4] == 0.0


@pytest.mark.parametrize("count", C.PARTIAL_COUNTS)
def test_partial_counts_of_the_dots(count):
    """`count` workgroups of k_dl_dots, hence partials per dot for k_dl_final, on 21000 entries (83 workgroups of its
    own): 1 strides 83 times; 255 ... 257 sum_partials' tail loop through one full pass; 1023 the last count below the
    unrolled loop; 1024, 1025 its first trip; 2048 the cap (most workgroups empty: their partials are zeros that must
    be written)."""
    s = case("partials")
    n = s["n"]
    own = (n + DC.WG - 1) // DC.WG
    assert own == 83 and (count == 1 or count > own)  # a stride loop, or more workgroups than the run's own
    whole = check_dots("partials", "generic", grid=count)
    sub = check_dots("partials", "generic", grid=count, rng=(1003, n - 1000))
    assert sub[0] < whole[0] and sub[2] < whole[2]
    if count in (1, 257, 2048):
        check_dots("partials", "decades", grid=count)
        check_dots("partials", "orthogonal", grid=count, rng=(2 * DC.WG + 1, 3 * DC.WG + 1))


def test_dots_of_every_vector_kind_at_the_runs_own_grid():
    for kind in DC.VECTORS:
        check_dots("partials", kind)
        for rng in DC.ranges(case("partials")["n"]):
            check_dots("partials", kind, rng=rng)


@pytest.mark.parametrize("request_,cls", DC.SPAN_GRIDS, ids=[f"span_grid_{r}" for r, _ in DC.SPAN_GRIDS])
def test_span_partial_counts_of_the_quadratic_forms(request_, cls):
    """b^T H b (k_dl_sum) and g^T H g (k_dl_final) add the span SpMV's partials, one per workgroup: options.span_grid
    sets their number, the graph's clamp has the last word and get_options reports it."""
    g = DC.graph("rows_8193")
    DC.check_graph("rows_8193", g)
    G = C.make(L, g, span_grid=request_, **BASE)
    count = int(G.options().span_grid)
    assert count == (G.spmv_spans().shape[0] - 1) // 4 == request_
    DC.check_span_count(cls, count)
    G.linearize()
    rp, ci, blk, b = G.get_system()
    s = dict(G=G, rp=rp, ci=ci, blk=blk, b=b, nb=rp.shape[0] - 1, n=b.shape[0], mmax=int(np.diff(rp).max()))
    ref = case("rows_8193")  # (the span table changes no bit of H or b: one reference for every count)
    assert np.array_equal(b, ref["b"]) and np.array_equal(blk, ref["blk"])
    check_dots("rows_8193", "generic", s=s, what=f" spans {count}")
    check_dots("rows_8193", "decades", s=s, rng=(1003, s["n"] - 1000), what=f" spans {count}")
    G.close()


# ------------------------------------------------------------------------------------------------ the update
def step_of(n, seed, size):
    return np.random.default_rng(seed).standard_normal(n) * size


def check_update(name, s, wa, wg, size, seed):
    """One trial's k_dogleg_oplus with h_dl = ca b + cg h_gn of magnitude ~ size."""
    g, G, b = s["g"], s["G"], s["b"]
    ca, cg = wa * size / np.abs(b).max(), wg
    hgn = step_of(s["n"], seed, size)
    h = (LD(ca) * b.astype(LD) + LD(cg) * hgn.astype(LD))
    if wa or wg:  # the branch of exp the step is on, from the inputs: theta = |omega| against exp_eps
        th = np.linalg.norm(h.reshape(-1, 7)[:, :3].astype(np.float64), axis=1)
        assert (th > s["o"]["eps"]).all() if size > 1e-3 else (th < s["o"]["eps"]).all()
    before = G.get_vertices()
    _, st, bk = G.debug_dogleg(hgn, ca=ca, cg=cg, scalars=False)
    assert np.array_equal(bk, before) and np.array_equal(G.get_vertices(), before)
    fixed = g["fixed"] != 0
    assert np.array_equal(st[fixed], before[fixed])
    if wa or wg:
        assert not np.array_equal(st[~fixed], before[~fixed])
    hx = DC.hidx_of(g)
    # the step as the kernel forms it, in each precision: ca b + cg h_gn entry by entry
    Sld = LR.oplus(before, h, hx, s["o"], LD)
    S64 = LR.oplus(before, ca * b + cg * hgn, hx, s["o"], np.float64)
    none = np.zeros(int((~fixed).sum()), dtype=bool)
    rq = LR.measured_ratio(st[~fixed, :4], S64[~fixed, :4], Sld[~fixed, :4], none)
    r = LR.measured_ratio(st[~fixed, 4:], S64[~fixed, 4:], Sld[~fixed, 4:], none)
    r = rq if rq["ratio"] > r["ratio"] else r
    print(f"[dl-op] {name:7s} update ca {ca:.3g} cg {cg:.3g} |h| ~ {size:g}: states noise {r['noise']:.2e} device at "
          f"{r['ratio']:.3f} x tolerance")
    assert r["ratio"] <= 1, (name, wa, wg, size, r)
    return st


@pytest.mark.parametrize("name", DC.UPDATE_GRAPHS)
def test_update_of_a_trial(name):
    """255, 256, 257 vertices (one workgroup short of, exactly, and one vertex beyond 256 threads); fixed vertices
    first, interior and last, so that hidx[v] is no v - const; the four coefficient patterns on both branches of exp."""
    s = case(name)
    for k, (what, wa, wg) in enumerate(DC.COEFFS):
        for size in DC.STEP_SIZES:
            check_update(name, s, wa, wg, size, seed=20 + k)


def test_failed_solve_moves_nothing_but_takes_the_backup():
    s = case("nv_257", linear_solver=1)
    G = s["G"]
    assert G.linear_solver_in_use() == 1
    before = G.get_vertices()
    hgn = step_of(s["n"], 31, 0.3)
    _, moved, _ = G.debug_dogleg(hgn, ca=0.1, cg=0.7, scalars=False)
    assert not np.array_equal(moved, before)
    _, st, bk = G.debug_dogleg(hgn, ca=0.1, cg=0.7, fail=True, scalars=False)
    assert np.array_equal(st, before) and np.array_equal(bk, before) and np.array_equal(G.get_vertices(), before)
    # the token is gone again: the same trial moves as before, bit for bit
    _, again, _ = G.debug_dogleg(hgn, ca=0.1, cg=0.7, scalars=False)
    assert np.array_equal(again, moved)
    # refused where no failure token exists
    P = case("nv_257")["G"]
    assert P.linear_solver_in_use() == 0
    with pytest.raises(L.Sim3OptError) as ei:
        P.debug_dogleg(hgn, fail=True)
    assert ei.value.code == L.ERR_STATE and "exact solver" in str(ei.value)


# ------------------------------------------------------------------------------------------------ exact: nothing changes
FIELDS = ("chi2_before", "chi2_after", "lambda_", "rho", "trials", "pcg_iters", "pcg_rel_res")
TR_FIELDS = ("delta_before", "delta_after", "alpha", "norm_sd", "norm_gn", "norm_dl", "step", "was_pd")
PAIRS = [(1, 20), (20, 1), (2, 2), (1, 2)]


def _run(G, iters, dogleg):
    n = G.optimize(iters)
    kt = G.kernel_times()
    st = [tuple(getattr(t, f) for f in FIELDS) for t in G.stats()]
    tr = [tuple(getattr(t, f) for f in TR_FIELDS) for t in G.trust_region_stats()] if dogleg else []
    counts = {k: getattr(kt, k) for k, _ in L.KernelTimes._fields_ if k.startswith("n_")}
    return n, G.get_vertices().tobytes(), st, tr, counts, G.chi2()


def _read_outs(G, seed, pcg):
    nb, _ = G.system_dims()
    n = 7 * nb
    G.debug_dogleg(step_of(n, seed, 0.2), ca=0.3, cg=0.5)
    G.debug_dogleg(step_of(n, seed + 1, 0.2), grid=3, j0=3, j1=n - 2, states=False)
    if not pcg:
        G.debug_dogleg(step_of(n, seed + 2, 0.2), ca=0.3, cg=0.5, fail=True)
    else:
        vs = G.column_vector_stride()
        G.debug_column_vectors("rhs", n, np.ones((3, vs)), at=[0, n - 1, -1])
        G.debug_column_vectors("residual", n, np.ones(vs), a=step_of(n, seed, 1), b=step_of(n, seed + 1, 1), system=2)
        G.debug_column_vectors("axpy", n - 1, np.ones(vs), a=step_of(n - 1, seed, 1), system=1)
        G.debug_column_vectors("gather", n, np.ones((5, 49)), a=step_of(n, seed, 1), first=1, count=3, col=4,
                               rows=[0, 2, 1, nb - 1])


@pytest.mark.parametrize("algorithm", [0, 2], ids=["lm", "dogleg"])
@pytest.mark.parametrize("solver", [0, 1], ids=["pcg", "exact"])
def test_optimize_and_covariances_after_the_read_outs_are_bit_identical(solver, algorithm):
    g = C.graph("info_kernels")
    opts = dict(fd_delta=1e-6, fix_small_angle_b=1, linear_solver=solver, algorithm=algorithm, cov_solver=1 - solver)
    if algorithm == 2:
        opts["dl_delta_init"] = 0.5
    a = C.make(L, g, **opts)
    want = [_run(a, 3, algorithm == 2), a.covariances(PAIRS, 1e-2).tobytes(), _run(a, 3, algorithm == 2)]
    b = C.make(L, g, **opts)
    b.linearize()
    _read_outs(b, 40, solver == 0)
    b.kernel_times(reset=True)  # (the linearisation above: a has none before its first run)
    a2 = C.make(L, g, **opts)
    a2.kernel_times(reset=True)
    got = [_run(b, 3, algorithm == 2)]
    assert got[0] == _run(a2, 3, algorithm == 2) and got[0][:4] == want[0][:4]
    kt0 = {k: getattr(b.kernel_times(), k) for k, _ in L.KernelTimes._fields_ if k.startswith("n_")}
    _read_outs(b, 50, solver == 0)
    kt1 = {k: getattr(b.kernel_times(), k) for k, _ in L.KernelTimes._fields_ if k.startswith("n_")}
    assert kt0 == kt1 and b.chi2() == a2.chi2() == got[0][5]
    got.append(b.covariances(PAIRS, 1e-2).tobytes())
    assert got[1] == want[1] == a2.covariances(PAIRS, 1e-2).tobytes()
    _read_outs(b, 60, solver == 0)  # (covariances left a linearisation: the read-outs run on it)
    got.append(_run(b, 3, algorithm == 2))
    assert got[2] == _run(a2, 3, algorithm == 2) and got[2][:4] == want[2][:4]
    for G in (a, a2, b):
        G.close()


def test_scalars_do_not_depend_on_an_earlier_read_out():
    """What a read-out with another vector, grid and range left in d_x, d_q, d_p, the partials and d_dl does not show."""
    s = case("rows_37")
    G, n = s["G"], s["n"]
    g1, g2 = step_of(n, 71, 0.1), step_of(n, 72, 10.0)
    first = G.debug_dogleg(g1, states=False)[0]
    G.debug_dogleg(g2, grid=7, j0=5, j1=n - 3, states=False)
    assert np.array_equal(G.debug_dogleg(g1, states=False)[0], first)


# ------------------------------------------------------------------------------------------------ refusals
def test_read_out_refuses_what_it_cannot_do():
    lib = L.load()
    g = C.graph("tail_7")
    G = L.Graph(fd_delta=1e-6, linear_solver=0)
    G.add_vertices(g["states"], g["fixed"])
    G.add_edges(g["v0"], g["v1"], g["meas"])
    x, out = np.zeros(7 * 7), np.zeros(6)
    p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    call = lambda *a: lib.sim3opt_debug_dogleg(G._g, *a)
    err = lambda: lib.sim3opt_last_error(G._g)
    # not initialised
    assert call(p(x), 0.0, 1.0, 0, 0, 0, 0, p(out), None, None) == L.ERR_STATE and b"initialize" in err()
    G.initialize()
    # null h_gn, every output null, a coefficient that is not finite
    assert call(None, 0.0, 1.0, 0, 0, 0, 0, p(out), None, None) == L.ERR_ARG and b"null h_gn" in err()
    assert call(p(x), 0.0, 1.0, 0, 0, 0, 0, None, None, None) == L.ERR_ARG and b"every output is null" in err()
    assert call(p(x), float("nan"), 1.0, 0, 0, 0, 0, p(out), None, None) == L.ERR_ARG and b"not finite" in err()
    # no linearisation yet
    assert call(p(x), 0.0, 1.0, 0, 0, 0, 0, p(out), None, None) == L.ERR_STATE and b"linearize" in err()
    G.linearize()
    # grid outside 0 .. MAX_GRID
    for grid in (-1, DC.MAX_GRID + 1):
        assert call(p(x), 0.0, 1.0, 0, grid, 0, 0, p(out), None, None) == L.ERR_ARG and b"grid out of range" in err()
    # ranges outside 0 <= j0 <= j1 <= 7 nb
    for j0, j1 in ((-1, 5), (6, 5), (0, 50), (50, 50)):
        assert call(p(x), 0.0, 1.0, 0, 0, j0, j1, p(out), None, None) == L.ERR_ARG and b"range out of bounds" in err()
    # with_fail on the PCG path
    assert G.linear_solver_in_use() == 0
    assert call(p(x), 0.0, 1.0, 1, 0, 0, 0, p(out), None, None) == L.ERR_STATE and b"exact solver" in err()
    assert call(p(x), 0.0, 1.0, 0, DC.MAX_GRID, 0, 49, p(out), None, None) == L.OK
    assert out[2] == out[3] == out[4] == out[5] == 0.0 and out[0] > 0  # h_gn = 0
    assert lib.sim3opt_version() == 130  # diagnostics are not part of the versioned interface


def test_read_outs_refuse_a_partitioned_graph():
    g = C.graph("tail_1")
    errs = []
    tg = DH.ThreadGroup(2)

    def body(rank):
        G = L.Graph(device=0, fd_delta=1e-6)
        G.add_vertices(g["states"], g["fixed"])
        G.add_edges(g["v0"], g["v1"], g["meas"])
        tg.attach(G, rank)
        G.initialize()
        G.linearize()
        nb, _ = G.system_dims()
        vs = G.column_vector_stride()
        for call in (lambda: G.debug_dogleg(np.zeros(7 * nb)),
                     lambda: G.debug_column_vectors("axpy", 7 * nb, np.ones(vs), a=np.ones(7 * nb))):
            try:
                call()
                errs.append("accepted")
            except L.Sim3OptError as e:
                errs.append((e.code, "partitioned" in str(e)))

    tg.run(body)
    assert errs == [(L.ERR_STATE, True)] * 4  # both read-outs, on both ranks, before any launch or collective
