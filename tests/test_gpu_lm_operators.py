"""GPU tests (-m gpu) of the Sim(3) LM set-up and update kernels as operators: what every iteration of the main path
runs -- k_linearize_numeric / k_linearize_analytic with their Gram phase, k_diag_reduce, k_final_trace_max, k_oplus,
k_scale, k_chi2 with k_final_sum_two (lm_kernels.hpp) -- is read out of the device (Graph.debug_linearization,
Graph.debug_update) and compared with tests/lm_ref.py in long double, entry by entry.  The parity tests hold the
assembled H to 1e-7 of its largest entry and an LM trace forgives a slightly wrong b; these tests do not
(tests/test_lm_ref.py asserts that each seeded defect moves the checked quantity by >= 1e3 x the tolerance used here).

Every case comes with the PATH CONDITION it exists for (tests/lm_cases.py), asserted on what the DEVICE reports.

Three kinds of check:
  derived ...... the inputs are the device's own arrays bit for bit (the J, e and w the Gram phase read, Omega, the
                 scratch, x and b, the per-edge rho) and the operation is sums of products: |dev - ld| <= gamma(k) x
                 (the same expression with absolute values), for any summation order and any FMA contraction (the
                 counts: lm_ref.K_GRAM ... k_sum, with their reasons).  An entry whose bound is zero -- a frozen DoF's
                 row and column, everything a Tukey-rejected edge stores, a row with one incidence -- must be exact.
  measured ..... the Jacobians, e, w, rho, exp(dx) S go through libm, a quotient of differences or a pivoted solve:
                 lm_ref.measured_ratio (32 x |float64 restatement - long double|, floored at 4u, every edge relative to
                 its own largest entry; residuals that amplify rounding -- lm_ref.ill_edges -- gauged among themselves).
                 Each case prints noise and the device's ratio (-s, `[lm-op]` lines); DESIGN.md 5c'' records the table.
  exact ........ a DUMP linearisation is a plain one; H10 = H01^T; the diagonal blocks are symmetric; max |H_dd| is the
                 maximum of the device's own diagonal; fixed vertices and a failed trial move nothing; the read-outs
                 change no later result; a rank's rows are the single-rank rows.
"""
import functools

import numpy as np
import pytest

from sim3opt_amd import lib as L
import amg_ref as R
import dist_helpers as DH
import lm_cases as C
import lm_ref as LR

LD, U = R.LD, R.U
pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not R.longdouble_ok(), reason="np.longdouble has no 64-bit mantissa here")]

NUM9, NUM6, ANA = ("numeric", 1e-9), ("numeric", 1e-6), ("analytic", 0.0)


def modes_of(name):
    if name in ("rows_8193", "big_e"):  # what these exist for does not depend on the mode: one numeric, one analytic
        return (NUM6, ANA)
    return (NUM9, NUM6) if name == "branches_b0" else (NUM9, NUM6, ANA)  # (the closed form refuses the as-written B)


LIN = [(n, m) for n in C.CASES for m in modes_of(n)]
LIN_IDS = [f"{n}-{m[0]}{m[1]:g}" for n, m in LIN]


def hidx_of(g):
    h = np.full(g["fixed"].shape[0], -1)
    h[g["fixed"] == 0] = np.arange(int((g["fixed"] == 0).sum()))
    return h


def graph_of(name, mode, **options):
    g = C.graph(name)
    opts = dict(jacobians=1, fix_small_angle_b=1) if mode[0] == "analytic" else dict(jacobians=0, fd_delta=mode[1])
    opts.update(options)
    return g, C.make(L, g, **opts)


@functools.lru_cache(maxsize=None)
def linearisation(name, mode):
    """The device's read-out of a case in a mode and the inputs as the DEVICE holds them, once for all tests of it."""
    g, G = graph_of(name, mode)
    d = G.debug_linearization()
    rowptr, colidx, blocks, b = G.get_system()
    G.linearize()
    plain = G.get_system()
    m = g["v0"].shape[0]
    states = G.get_vertices()
    meas = np.array([G.get_edge(k)[2] for k in range(m)])
    o = LR.mopts(**{k: v for k, v in G_options(G).items()})
    return dict(g=g, G=G, d=d, rowptr=rowptr, colidx=colidx, blocks=blocks, b=b, plain=plain, states=states, meas=meas,
                o=o, mask=int(G.options().dof_mask))


def G_options(G):
    o = G.options()
    return dict(exp_eps=o.exp_eps, small_rot_half=o.small_rot_half, fix_small_angle_b=o.fix_small_angle_b)


def report(name, mode, what, r):
    ill = f"  | {r['n_ill']} ill-conditioned: noise {r['noise_ill']:.2e} ratio {r['ratio_ill']:.3f}" if r["n_ill"] else ""
    print(f"[lm-op] {name:12s} {mode[0]:8s} {mode[1]:<6g} {what:4s} noise {r['noise']:.2e}  device at {r['ratio']:.3f} x tolerance{ill}")


# ------------------------------------------------------------------------------------------------ exact: DUMP = plain
@pytest.mark.parametrize("name,mode", LIN, ids=LIN_IDS)
def test_dump_linearisation_is_the_plain_one_and_meets_the_path_condition(name, mode):
    """All eight instantiations (tail_* / fixed_ends / parallel <false, false>, info <true, false>, kernels <false,
    true>, info_kernels <true, true>, in both Jacobian modes): the system after the read-out equals linearize()'s."""
    s = linearisation(name, mode)
    for a, b in zip((s["rowptr"], s["colidx"], s["blocks"], s["b"]), s["plain"]):
        assert np.array_equal(a, b)
    f = C.check_path(name, s["g"], s["d"])
    o = s["G"].options()
    assert bool(o.jacobians) == (mode[0] == "analytic") and (mode[0] == "analytic" or o.fd_delta == mode[1])
    print(f"[lm-op] {name}: {f}, info {s['g']['info'] is not None}, kernels {s['g']['kinds'] is not None}")
    # the read-out's edge list and weights are those of the graph
    assert s["d"]["J"].shape == (f["n_active"], 15, 7) and np.isfinite(s["d"]["J"]).all()
    if s["g"]["kinds"] is None:
        assert (s["d"]["w"] == 1).all()
    assert np.all(s["colidx"][s["rowptr"][:-1]] == np.arange(f["rows"]))  # the diagonal block first in every row


# ------------------------------------------------------------------------------------------------ derived: Gram phase
@pytest.mark.parametrize("name,mode", LIN, ids=LIN_IDS)
def test_gram_phase_stores_entry_by_entry(name, mode):
    s = linearisation(name, mode)
    g, d = s["g"], s["d"]
    act = d["active"]
    Om = None if g["info"] is None else np.asarray(g["info"])[act]
    G, Gm = LR.gram(d["J"], d["w"], Om, LD)
    H01, H10, s0, s1 = LR.edge_stores(G)
    M01, M10, m0, m1 = LR.edge_stores(Gm)
    k = LR.K_GRAM if Om is None else LR.K_GRAM_INFO
    ratios = {}
    for what, slot, ref, mag, dev in (("H01", d["slot01"][act], H01, M01, s["blocks"]), ("H10", d["slot10"][act], H10, M10, s["blocks"]),
                                      ("inc0", d["inc0"][act], s0, np.abs(m0), d["scratch"]), ("inc1", d["inc1"][act], s1, np.abs(m1), d["scratch"])):
        own = slot >= 0
        assert np.unique(slot[own]).shape[0] == own.sum()  # one owner per slot: parallel edges have their own
        ratios[what] = LR.derived_ratio(dev[slot[own]], ref[own], mag[own], k) if own.any() else 0.0
    both = d["slot01"][act] >= 0
    assert np.array_equal(s["blocks"][d["slot10"][act][both]], s["blocks"][d["slot01"][act][both]].transpose(0, 2, 1))
    # every off-diagonal block and every incidence has been checked: none is left to another writer
    nb = d["incptr"].shape[0] - 1
    offdiag = np.ones(s["blocks"].shape[0], dtype=bool)
    offdiag[s["rowptr"][:-1]] = False
    owned = np.concatenate([d["slot01"][act][both], d["slot10"][act][both]])
    assert np.array_equal(np.sort(owned), np.flatnonzero(offdiag)) and nb == s["rowptr"].shape[0] - 1
    # what a zero bound means here, stated outright
    dead = d["w"] == 0
    if g["kinds"] is not None:
        assert dead.any() and (g["kinds"][act][dead] >= 7).all()  # Tukey / saturated, rejected
        for slot, dev in ((d["slot01"], s["blocks"]), (d["slot10"], s["blocks"]), (d["inc0"], d["scratch"]), (d["inc1"], d["scratch"])):
            sl = slot[act][dead]
            assert (dev[sl[sl >= 0]] == 0).all()
    frozen = [i for i in range(7) if not (s["mask"] >> i) & 1]
    if frozen:
        assert (d["J"][:, frozen] == 0).all() and (d["J"][:, [7 + i for i in frozen]] == 0).all()
        assert (s["blocks"][:, frozen, :] == 0).all() and (s["blocks"][:, :, frozen] == 0).all()
        assert (s["b"].reshape(-1, 7)[:, frozen] == 0).all()
    print(f"[lm-op] {name:12s} {mode[0]:8s} {mode[1]:<6g} Gram phase, error / derived bound (k = {k}): " +
          ", ".join(f"{a} {b:.3f}" for a, b in ratios.items()))
    assert max(ratios.values()) <= 1, ratios


# ------------------------------------------------------------------------------------------------ derived: k_diag_reduce
@pytest.mark.parametrize("name,mode", LIN, ids=LIN_IDS)
def test_diag_reduce_trace_and_max(name, mode):
    s = linearisation(name, mode)
    d = s["d"]
    want, mag, cnt = LR.row_sums(d["scratch"], d["incptr"], LD)
    Dw, bw = LR.diag_block(want)
    Dm, bm = LR.diag_block(mag)
    D = s["blocks"][s["rowptr"][:-1]]
    kr = LR.k_row(cnt)
    ratios = dict(H_dd=LR.derived_ratio(D, Dw, Dm, kr[:, None, None]),
                  b=LR.derived_ratio(s["b"].reshape(-1, 7), bw, bm, kr[:, None]))
    assert np.array_equal(D, D.transpose(0, 2, 1))
    dg = np.diagonal(D, axis1=1, axis2=2)
    tr, trm, mx = LR.trace_and_max(D, LD)
    ratios["trace"] = LR.derived_ratio(d["trace"], tr, trm, LR.k_trace(D.shape[0]))
    assert d["maxdiag"] == np.abs(dg).max()  # exactly: the maximum of the device's own diagonal
    print(f"[lm-op] {name:12s} {mode[0]:8s} {mode[1]:<6g} k_diag_reduce, error / derived bound: " +
          ", ".join(f"{a} {b:.3f}" for a, b in ratios.items()) + f"; up to {int(cnt.max())} incidences per row")
    assert max(ratios.values()) <= 1, ratios


# ------------------------------------------------------------------------------------------------ measured: J, e, w, rho
@functools.lru_cache(maxsize=None)
def restated(name, mode):
    """float64 and long-double restatement of a case's J (with e) from the DEVICE's inputs, and the ill-conditioned set."""
    s = linearisation(name, mode)
    g = s["g"]
    act = s["d"]["active"]
    a = (s["meas"][act], s["states"][g["v0"][act]], s["states"][g["v1"][act]], s["o"])
    out = {}
    for dt in (np.float64, LD):
        out[dt] = (LR.analytic_jacobian(*a, s["mask"], dt) if mode[0] == "analytic"
                   else LR.numeric_jacobian(*a, mode[1], s["mask"], dt))
    out["ill"] = LR.ill_edges(out[np.float64][:, 14], out[LD][:, 14])
    return out


@pytest.mark.parametrize("name,mode", LIN, ids=LIN_IDS)
def test_jacobians_residuals_and_weights(name, mode):
    s = linearisation(name, mode)
    g, d = s["g"], s["d"]
    r = restated(name, mode)
    ill = r["ill"]
    assert ill.mean() <= 0.10
    res = dict(J=LR.measured_ratio(d["J"][:, :14], r[np.float64][:, :14], r[LD][:, :14], ill, ill_above=LR.ill_level(*mode)),
               e=LR.measured_ratio(d["J"][:, 14], r[np.float64][:, 14], r[LD][:, 14], ill, floor=1.0))
    act = d["active"]
    if g["kinds"] is not None:
        Om = None if g["info"] is None else np.asarray(g["info"])[act]
        k, dl = g["kinds"][act], g["deltas"][act]
        _, _, w64 = LR.chi_rho_w(r[np.float64][:, 14], Om, k, dl, np.float64)
        _, _, wld = LR.chi_rho_w(r[LD][:, 14], Om, k, dl, LD)
        res["w"] = LR.measured_ratio(d["w"][:, None], w64[:, None], wld[:, None], ill, floor=1.0)
        for kind in range(1, 10):  # both sides of every threshold are in what was compared
            assert (g["above"][act] & (k == kind)).any() and (~g["above"][act] & (k == kind)).any()
    for what, v in res.items():
        report(name, mode, what, v)
    assert res["J"]["n_ill"] <= 0.10 * ill.size  # (tests/test_lm_ref.py asserts the same from the restatement alone)
    assert max(max(v["ratio"], v["ratio_ill"]) for v in res.values()) <= 1, res


@pytest.mark.parametrize("name", ["kernels", "info_kernels", "big_e", "branches_b0"])
def test_edge_chi2_rho_and_weight(name):
    """The per-edge chi2, rho and w of k_edge_chi2 (every edge, the inactive ones too): the terms of the chi2 sum."""
    s = linearisation(name, NUM6)
    g = s["g"]
    chi, rho, w = s["G"].edge_chi2()
    a = (s["meas"], s["states"][g["v0"]], s["states"][g["v1"]], s["o"])
    e64, eld = LR.edge_error(*a, np.float64), LR.edge_error(*a, LD)
    ill = LR.ill_edges(e64, eld)
    c64, r64, w64 = LR.chi_rho_w(e64, g["info"], g["kinds"], g["deltas"], np.float64)
    cld, rld, wld = LR.chi_rho_w(eld, g["info"], g["kinds"], g["deltas"], LD)
    sc = np.maximum(cld, 1).astype(LD)[:, None]  # (chi2 itself is relative to max(chi2, 1), as e is to max(|e|, 1))
    res = dict(chi2=LR.measured_ratio(chi[:, None] / sc, c64[:, None] / sc, cld[:, None] / sc, ill, floor=1.0),
               rho=LR.measured_ratio(rho[:, None] / sc, r64[:, None] / sc, rld[:, None] / sc, ill, floor=1.0),
               w=LR.measured_ratio(w[:, None], w64[:, None], wld[:, None], ill, floor=1.0))
    for what, v in res.items():
        report(name, NUM6, what, v)
    assert max(max(v["ratio"], v["ratio_ill"]) for v in res.values()) <= 1, res


# ------------------------------------------------------------------------------------------------ the update
def step_of(nb, seed, size):
    return np.random.default_rng(seed).standard_normal(7 * nb) * size


def update_checks(name, s, x, lam, grid=0, what=""):
    """One debug_update against the restatement: states measured, backup / fixed exact, scale and chi2 derived."""
    g, G = s["g"], s["G"]
    before = G.get_vertices()
    st, bk, chi, sc = G.debug_update(x, lam, grid=grid)
    assert np.array_equal(bk, before) and np.array_equal(G.get_vertices(), before)
    fixed = g["fixed"] != 0
    assert np.array_equal(st[fixed], before[fixed]) and not np.array_equal(st[~fixed], before[~fixed])
    h = hidx_of(g)
    Sld, S64 = LR.oplus(before, x, h, s["o"], LD), LR.oplus(before, x, h, s["o"], np.float64)
    none = np.zeros(int((~fixed).sum()), dtype=bool)
    rq = LR.measured_ratio(st[~fixed, :4], S64[~fixed, :4], Sld[~fixed, :4], none)  # the quaternion on its own scale
    r = LR.measured_ratio(st[~fixed, 4:], S64[~fixed, 4:], Sld[~fixed, 4:], none)
    r = rq if rq["ratio"] > r["ratio"] else r
    want, mag = LR.scale_terms(x, s["b"], lam, LD)
    ratios = dict(scale=LR.derived_ratio(sc, want, mag, LR.k_sum(x.size, LR.K_SCALE_TERM)))
    # chi2 at the trial's estimates, from the device's own per-edge rho there
    G.set_vertices(st)
    _, rho, _ = G.edge_chi2()
    G.set_vertices(before)
    G.linearize()  # (set_vertices drops the linearisation; the same estimates give the same system)
    assert np.array_equal(G.get_vertices(), before) and np.array_equal(G.get_system()[3], s["b"])
    ratios["chi2"] = LR.derived_ratio(chi, rho.astype(LD).sum(), np.abs(rho).astype(LD).sum(), rho.size - 1)
    print(f"[lm-op] {name:12s} update{what}: states noise {r['noise']:.2e} device at {r['ratio']:.3f} x tolerance; "
          f"error / derived bound: scale {ratios['scale']:.3f}, chi2 {ratios['chi2']:.3f}")
    assert r["ratio"] <= 1 and max(ratios.values()) <= 1, (r, ratios)
    return chi, sc


@pytest.mark.parametrize("name", ["fixed_ends", "info_kernels", "branches_b1", "big_e", "rows_8193"])
def test_update_scale_and_chi2(name):
    s = linearisation(name, NUM6)
    nb = s["rowptr"].shape[0] - 1
    lam = 1e-3 * s["d"]["maxdiag"]
    for seed, size in ((1, 0.3), (2, 1e-7)):  # a step on exp's generic branch, one on its small-angle branch
        update_checks(name, s, step_of(nb, seed, size), lam, what=f" |x| ~ {size:g}")
    if name == "fixed_ends":  # both fixed vertices' edge counts in chi2 although it is not linearised
        g = s["g"]
        chi, rho, w = s["G"].edge_chi2()
        both = (g["fixed"][g["v0"]] != 0) & (g["fixed"][g["v1"]] != 0)
        assert both.sum() == 1 and rho[both][0] > 0.01 * rho.sum() / rho.size
        assert abs(s["G"].chi2() - rho.sum()) <= 1e-13 * rho.sum()


def test_failed_trial_moves_nothing_but_takes_the_backup():
    g, G = graph_of("fixed_ends", NUM6, linear_solver=1)
    assert G.linear_solver_in_use() == 1
    G.linearize()
    nb, _ = G.system_dims()
    before = G.get_vertices()
    x = step_of(nb, 3, 0.3)
    moved, _, chi_m, _ = G.debug_update(x, 1.0)
    assert not np.array_equal(moved, before)
    st, bk, chi, sc = G.debug_update(x, 1.0, fail=True)
    assert np.array_equal(st, before) and np.array_equal(bk, before) and np.array_equal(G.get_vertices(), before)
    assert chi == G.chi2() and chi != chi_m
    # refused where no failure token exists
    g2, G2 = graph_of("fixed_ends", NUM6, linear_solver=0)
    G2.linearize()
    with pytest.raises(L.Sim3OptError) as ei:
        G2.debug_update(x, 1.0, fail=True)
    assert ei.value.code == L.ERR_STATE and "exact solver" in str(ei.value)


@pytest.mark.parametrize("count", C.PARTIAL_COUNTS)
def test_partial_counts_of_the_chi2_and_scale_sums(count):
    """`count` workgroups, hence partial sums, for k_chi2 and k_scale (k_final_sum_two adds them).  A trial's own
    counts are ceil(edges / 256) and ceil(7 rows / 256), capped at 2048; each count here stands for the production
    shape that yields it:
        1 ............. up to 256 edges (KITTI-size scale sums: 7 x 36 rows); this graph then strides 16 / 83 times,
                        as k_chi2 / k_scale stride beyond 524288 edges / 74899 rows
        255, 256, 257 . 65k edges or 9.3k rows: sum_partials' tail loop alone, through one full pass of 256 threads
        1023 .......... the last count below the four-way unrolled loop
        1024, 1025 .... 262k edges: the unrolled loop's first trip (i + 768 < n for i = 0 ... 255), and one beyond
        2048 .......... the cap: 524k edges and more (the 1M-edge benchmark graph)"""
    s = linearisation("partials", NUM6)
    m, nb = s["g"]["v0"].shape[0], s["rowptr"].shape[0] - 1
    assert 3000 < m < 5000  # a few thousand edges: several strides at small counts, empty workgroups at large ones
    update_checks("partials", s, step_of(nb, 4, 0.1), 1e-3 * s["d"]["maxdiag"], grid=count, what=f" grid {count}")


# ------------------------------------------------------------------------------------------------ exact: nothing changes
def _run(G, iters):
    n = G.optimize(iters)
    kt = G.kernel_times()
    st = [(t.chi2_before, t.chi2_after, t.lambda_, t.rho, t.trials, t.pcg_iters, t.pcg_rel_res) for t in G.stats()]
    counts = {k: getattr(kt, k) for k, _ in L.KernelTimes._fields_ if k.startswith("n_")}
    return n, G.get_vertices(), st, counts


@pytest.mark.parametrize("opts", [dict(linear_solver=0, algorithm=0), dict(linear_solver=1, algorithm=0),
                                  dict(linear_solver=1, algorithm=2)], ids=["lm_pcg", "lm_direct", "dogleg"])
def test_optimize_after_the_read_outs_is_bit_identical(opts):
    g = C.graph("info_kernels")
    a = C.make(L, g, fd_delta=1e-6, **opts)
    ref = _run(a, 4)
    b = C.make(L, g, fd_delta=1e-6, **opts)
    nb, _ = b.system_dims()
    b.debug_linearization()
    b.debug_update(step_of(nb, 5, 0.2), 0.7)
    b.debug_update(step_of(nb, 6, 0.2), 0.1, grid=3)
    if opts["linear_solver"] == 1:
        b.debug_update(step_of(nb, 7, 0.2), 0.1, fail=True)
    b.debug_linearization()
    b.kernel_times(reset=True)  # (the linearisations before: a's has none of them)
    a2 = C.make(L, g, fd_delta=1e-6, **opts)
    a2.kernel_times(reset=True)
    got, want = _run(b, 4), _run(a2, 4)
    assert got[0] == want[0] == ref[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[1], ref[1])
    assert got[2] == want[2] and got[3] == want[3]
    # and between two optimize() calls: solver scalars, the cached chi2 and the counters stay as they were
    kt0 = {k: getattr(b.kernel_times(), k) for k, _ in L.KernelTimes._fields_ if k.startswith("n_")}
    b.debug_linearization()
    b.debug_update(step_of(nb, 8, 0.2), 0.3)
    kt1 = {k: getattr(b.kernel_times(), k) for k, _ in L.KernelTimes._fields_ if k.startswith("n_")}
    assert kt0 == kt1
    got, want = _run(b, 3), _run(a2, 3)
    assert got[0] == want[0] and np.array_equal(got[1], want[1]) and got[2] == want[2]


def test_read_outs_refuse_what_they_cannot_do():
    import ctypes
    lib = L.load()
    g = C.graph("tail_7")
    G = L.Graph()
    G.add_vertices(g["states"], g["fixed"])
    G.add_edges(g["v0"], g["v1"], g["meas"])
    na, ni = ctypes.c_int32(), ctypes.c_int32()
    x = np.zeros(7 * 7)
    p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    out = np.zeros(64)
    # not initialised
    assert lib.sim3opt_debug_linearization_dims(G._g, ctypes.byref(na), ctypes.byref(ni)) == L.ERR_STATE
    assert lib.sim3opt_debug_update(G._g, p(x), 1.0, 0, 0, None, None, p(out), None) == L.ERR_STATE
    assert b"initialize" in lib.sim3opt_last_error(G._g)
    G.initialize()
    assert lib.sim3opt_debug_linearization_dims(G._g, ctypes.byref(na), ctypes.byref(ni)) == L.OK
    assert (na.value, ni.value) == (7, 13)
    # null pointers
    assert lib.sim3opt_debug_linearization(G._g, *([None] * 11)) == L.ERR_ARG
    assert b"null" in lib.sim3opt_last_error(G._g)
    assert lib.sim3opt_debug_update(G._g, None, 1.0, 0, 0, None, None, p(out), None) == L.ERR_ARG
    assert lib.sim3opt_debug_update(G._g, p(x), 1.0, 0, 0, None, None, None, None) == L.ERR_ARG
    assert lib.sim3opt_debug_update(G._g, p(x), float("nan"), 0, 0, None, None, p(out), None) == L.ERR_ARG
    # no linearisation yet: no b for the scale
    assert lib.sim3opt_debug_update(G._g, p(x), 1.0, 0, 0, None, None, p(out), None) == L.ERR_STATE
    G.linearize()
    assert lib.sim3opt_debug_update(G._g, p(x), 1.0, 0, 4096, None, None, p(out), None) == L.ERR_ARG
    assert lib.sim3opt_debug_update(G._g, p(x), 1.0, 0, 0, None, None, p(out), None) == L.OK
    assert out[0] == G.chi2()  # a zero step: the chi2 of the estimates
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
        for call in (G.debug_linearization, lambda: G.debug_update(np.zeros(7 * nb), 1.0)):
            try:
                call()
                errs.append("accepted")
            except L.Sim3OptError as e:
                errs.append((e.code, "partitioned" in str(e)))

    tg.run(body)
    assert errs == [(L.ERR_STATE, True)] * 4  # both read-outs, on both ranks, before any launch or collective


@pytest.mark.parametrize("world", [2, 3])
def test_partitioned_numeric_linearisation_is_the_single_rank_rows(world):
    """Each rank's rows of a numeric-mode graph with information matrices and kernels, bit for bit."""
    g = C.graph("partitioned")
    single = C.make(L, g, device=0, row_order=1, fd_delta=1e-6)  # (a partition orders its rows by locality)
    single.linearize()
    rp, ci, blocks, b = single.get_system()
    tg = DH.ThreadGroup(world)
    seen = []

    def body(rank):
        G = L.Graph(device=0, fd_delta=1e-6)
        G.add_vertices(g["states"], g["fixed"])
        G.add_edges(g["v0"], g["v1"], g["meas"], info=g["info"], kernel=g["kinds"], kernel_delta=g["deltas"])
        tg.attach(G, rank)
        G.initialize()
        G.linearize()
        r0, r1 = G.local_rows()
        rp_, ci_, bl_, b_ = G.get_system()
        ok = (np.array_equal(rp_, rp) and np.array_equal(ci_, ci) and np.array_equal(bl_[rp[r0]:rp[r1]], blocks[rp[r0]:rp[r1]])
              and np.array_equal(b_[7 * r0:7 * r1], b[7 * r0:7 * r1]))
        seen.append((r0, r1, ok))

    tg.run(body)
    seen.sort()
    assert [s[2] for s in seen] == [True] * world
    assert seen[0][0] == 0 and seen[-1][1] == rp.shape[0] - 1 and all(seen[i][1] == seen[i + 1][0] for i in range(world - 1))
