"""CPU tests of tests/pcg_ref.py and tests/pcg_cases.py, the yardstick and the cases of tests/test_gpu_pcg_operator.py:
the reference product against a dense product, the kernel-walk model against the reference, the path condition of
every case on the host's pattern and span partition, the PCG restatement against a dense solve -- and the
SENSITIVITY of the comparisons: every defect of pcg_ref.SPAN_DEFECTS moves some entry of q by at least 1e4 x the
bound the GPU test applies to that entry, every defect of pcg_ref.PCG_DEFECTS moves the iterate x_k by at least
1e4 x the GPU test's tolerance (32 x noise).

Nothing here needs a GPU: patterns and span partitions are host-only read-outs; values are random blocks (the index
logic does not care) or the CPU oracle's dense H on the product's pattern (the recurrence needs an SPD system).
"""
import numpy as np
import pytest

from oracle import oracle as O
from sim3opt_amd import lib as L
import amg_ref as R
import pcg_cases as C
import pcg_ref as P

LD, U = R.LD, R.U
pytestmark = pytest.mark.skipif(not R.longdouble_ok(), reason="np.longdouble has no 64-bit mantissa here")
KS = C.ITERATE_CAPS  # iteration caps of the GPU test


def rule_grid(nb, requested=0):
    """Engine::init's choice of the span SpMV's workgroups, restated for THIS file only (the GPU test reads the table
    the device holds): ~4 rows per wavefront, at least the resident set while every wavefront still gets a row."""
    g = max(min(2048, (nb + 3) // 4), (nb + 15) // 16)
    if requested > 0:
        g = min(requested, (nb + 3) // 4)
    return max(8, min(65536, g))


_pat = {}


def pattern(name):
    """(graph, rowptr, colidx, span table) of a case, host only."""
    if name not in _pat:
        gname, opts = C.CASES[name]
        g = C.graph_of(gname)
        G = L.Graph(**opts)
        G.add_vertices(g["states"], g["fixed"])
        G.add_edges(g["v0"], g["v1"], g["meas"])
        rp, ci = G.system_pattern()
        G.close()
        wrow = L.partition_rows(rp, 4 * rule_grid(rp.shape[0] - 1, opts.get("span_grid", 0)))
        _pat[name] = (g, rp, ci, wrow)
    return _pat[name]


def random_system(rp, ci, m, seed=5):
    """Random blocks on a pattern (diagonal blocks ten times larger), m Gaussian vectors, m distinct dampings around
    1e-3 x max diag."""
    rng = np.random.default_rng(seed)
    blk = rng.standard_normal((ci.shape[0], 7, 7))
    blk[rp[:-1]] *= 10.0
    p = rng.standard_normal((m, 7 * (rp.shape[0] - 1)))
    maxdiag = np.abs(blk[rp[:-1]].diagonal(0, 1, 2)).max()
    lam = 1e-3 * maxdiag * (1.0 + np.arange(m))
    return blk, p, lam


def bound_ratio(q, q_ld, mag, rp):
    """max over the entries of |q - q_ld| / (gamma(7 m_i + 3) mag_i): the GPU test asserts <= 1."""
    g = P.gamma_k(7 * P.blocks_per_row(rp).astype(LD) + 3)
    err = np.abs(np.asarray(q, dtype=LD) - q_ld)
    tol = g * mag
    assert ((tol > 0) | (err == 0)).all()
    return float((err[tol > 0] / tol[tol > 0]).max())


# ------------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("name", list(C.CASES))
def test_every_case_meets_its_path_condition_on_the_host(name):
    g, rp, ci, wrow = pattern(name)
    f = C.facts(rp, ci, wrow, C.hub_row(g))
    print(C.describe(name, f))
    C.check_path(name, f)


def test_right_hand_sides():
    names, vs = C.rhs_set(np.arange(70.0), hub=3)
    assert names == ["b", "gauss0", "gauss1", "gauss2", "e_first", "e_last", "e_hub", "decades"]
    assert vs[4, 0] == 1 and vs[5, -1] == 1 and vs[6, 21] == 1 and [np.count_nonzero(v) for v in vs[4:7]] == [1, 1, 1]
    d = vs[7]
    assert (np.sign(d[::2]) > 0).all() and (np.sign(d[1::2]) < 0).all()
    assert np.log10(np.abs(d).max() / np.abs(d).min()) > 10  # (70 samples of twelve decades)


# ------------------------------------------------------------------------------------------------ the product
def test_reference_product_is_the_dense_product_and_counts_parallel_blocks_separately():
    g, rp, ci, _ = pattern("hub_mid")
    blk, p, lam = random_system(rp, ci, 2)
    nb = rp.shape[0] - 1
    A = R.dense_of(nb, R._row_of_block(rp), ci, blk, LD)  # (sums the blocks of a repeated column)
    q, mag = P.bcsr_apply(rp, ci, blk, lam, p, LD)
    for s in range(2):
        ref = A @ p[s].astype(LD) + LD(lam[s]) * p[s].astype(LD)
        # two long-double evaluations in different orders: gamma(7 m + 3) with u_longdouble = 2^-64
        assert (np.abs(q[s] - ref) <= 2.0 ** -11 * P.gamma_k(7 * P.blocks_per_row(rp) + 3) * mag[s]).all()
    hub = C.hub_row(g)
    c = ci[rp[hub]:rp[hub + 1]]
    assert c.shape[0] - np.unique(c).shape[0] >= C.HUB_DOUBLE
    # the magnitude dominates the product and is reached when all signs agree
    qa, ma = P.bcsr_apply(rp, ci, np.abs(blk), lam[0], np.abs(p[0]), LD)
    assert (mag[0] >= np.abs(q[0])).all() and np.array_equal(qa, ma)


@pytest.mark.parametrize("name,CH", [("tiny1", 8), ("tiny3", 4), ("m400", 8), ("hub_first", 8), ("hub_mid", 4),
                                     ("hub_last", 8), ("chain10k_g8", 8), ("m3000", 8)])
def test_kernel_walk_without_a_defect_is_the_reference_product(name, CH):
    """... in long double to long-double rounding, and in float64 within the GPU test's bound (the bound holds for a
    float64 evaluation in the kernel's order)."""
    _, rp, ci, wrow = pattern(name)
    m = 3 if name in ("m3000", "hub_mid") else 1
    blk, p, lam = random_system(rp, ci, m)
    q_ld, mag = P.bcsr_apply(rp, ci, blk, lam, p, LD)
    w_ld = P.span_model(rp, ci, blk, wrow, lam, p, CH=CH, dt=LD)
    assert bound_ratio(w_ld, q_ld, mag, rp) <= 2.0 ** -10
    w64 = P.span_model(rp, ci, blk, wrow, lam, p, CH=CH, dt=np.float64)
    r = bound_ratio(w64, q_ld, mag, rp)
    print(f"[pcg-ref] {name} CH {CH}: float64 walk at {r:.3f} of the bound")
    assert r <= 1.0


SPAN_PAIRS = [(n, d) for n in ("hub_first", "hub_mid", "hub_last")
              for d in P.SPAN_DEFECTS if d != "rowend_no_refill"] + \
             [("chain10k_g8", d) for d in ("rowend_no_refill", "window_stale", "skip_64", "dup_64", "lam_prev_p")]


@pytest.mark.parametrize("name,defect", SPAN_PAIRS)
def test_sensitivity_of_the_product_check(name, defect):
    """Each defect, on a case whose path reaches it, moves some entry of q by >= 1e4 x the entry's bound."""
    _, rp, ci, wrow = pattern(name)
    blk, p, lam = random_system(rp, ci, 3 if defect == "batch_lambda0" else 1)
    q_ld, mag = P.bcsr_apply(rp, ci, blk, lam, p, LD)
    qd = P.span_model(rp, ci, blk, wrow, lam, p, dt=np.float64, defect=defect)
    r = bound_ratio(qd, q_ld, mag, rp)
    rows = np.unique(np.flatnonzero(np.abs(qd - q_ld.astype(np.float64)).reshape(qd.shape[0], -1, 7).max(axis=(0, 2))
                                    > 1e-9 * np.abs(mag).max()))
    print(f"[pcg-ref] {name}: {defect:20s} moves q by {r:.2e} x the bound, in {rows.shape[0]} block rows")
    assert r >= 1e4, (name, defect, r)


def test_every_span_defect_is_paired_with_a_case():
    assert {d for _, d in SPAN_PAIRS} == set(P.SPAN_DEFECTS)


# ------------------------------------------------------------------------------------------------ the recurrence
_sys = {}


def spd_case(name):
    """The CPU oracle's dense H and b on the product's pattern (a repeated column: the whole block in its first slot)."""
    if name not in _sys:
        g, rp, ci, _ = pattern(name)
        OG = O.Graph(g["states"], g["fixed"], g["v0"], g["v1"], g["meas"])
        H, b = OG.build_dense(O.default_options(fix_small_angle_b=1, fd_delta=1e-6))
        _sys[name] = dict(rp=rp, ci=ci, blk=R.blocks_from_dense(H, rp, ci), b=b, H=H,
                          lam=C.ITERATE_CASES[name] * H.diagonal().max())
    return _sys[name]


REL_TOL = C.PCG_REL_TOL  # what the GPU test sets


@pytest.mark.parametrize("name", ["m400", "hub_mid"])
def test_pcg_restatement_solves_the_system_and_the_cap_stops_it(name):
    c = spd_case(name)
    a = (c["rp"], c["ci"], c["blk"], c["b"], c["lam"])
    full = P.pcg(*a, 2000, 1e-13, LD)
    A = c["H"] + c["lam"] * np.eye(c["H"].shape[0])
    assert full["iters"] < 2000 and not full["fail"]
    assert R.relerr(full["x"][-1], np.linalg.solve(A, c["b"])) < 1e-9
    # stopped by the tolerance: rel_res is the gamma the stopping test saw
    assert full["rel_res"] <= 1e-13 and len(full["gamma"]) == full["iters"] + 1
    run = P.pcg(*a, max(KS), REL_TOL, LD)
    assert run["iters"] == max(KS) and len(run["x"]) == max(KS)
    g = np.array(run["gamma"], dtype=LD)
    # the condition of the GPU test: at every cap used the tolerance is far from met, so the cap stops the solve
    assert (g / g[0] > LD(REL_TOL) ** 2).all() and float(REL_TOL) ** 2 > np.finfo(np.float64).tiny
    assert g[-1] / g[0] > C.ITERATE_FLOOR
    print(f"[pcg-ref] {name}: gamma_k / gamma_0 at k = {max(KS) - 1}: {float(g[-1] / g[0]):.2e}")
    # stopped by the cap after k steps: rel_res is the gamma of the residual BEFORE step k
    for k in KS:
        rk = P.pcg(*a, k, REL_TOL, LD)
        assert rk["iters"] == k and rk["rel_res"] == np.sqrt(g[k - 1] / g[0])
        assert np.array_equal(rk["x"][-1], run["x"][k - 1])


@pytest.mark.parametrize("name", ["m400", "hub_mid"])
def test_sensitivity_of_the_iterate_check(name):
    """x_k of each defective recurrence against the long-double x_k, in units of the GPU test's tolerance
    (32 x |float64 restatement - long double|, floored at 4u).  beta_parity and alpha_old_stale read a slot that is
    still zero at the second step: the device would flag a breakdown there and keep x_1.  Every defect needs two
    steps to show, except the cap."""
    c = spd_case(name)
    a = (c["rp"], c["ci"], c["blk"], c["b"], c["lam"])
    xld = P.pcg(*a, max(KS), REL_TOL, LD)["x"]
    x64 = P.pcg(*a, max(KS), REL_TOL, np.float64)["x"]
    worst = {}
    for mut in P.PCG_DEFECTS:
        for k in KS:
            if k == 1 and mut != "cap_plus_one":
                continue
            xm = P.pcg(*a, k, REL_TOL, np.float64, mut=mut)["x"][-1]
            noise, tol = R.noise_and_tol(x64[k - 1], xld[k - 1])
            f = R.relerr(xm, xld[k - 1]) / tol
            worst[mut] = min(worst.get(mut, np.inf), f)
            print(f"[pcg-ref] {name} k {k:2d}: noise {noise:.2e}  {mut:16s} moves x_k by {f:.2e} x tolerance")
    assert min(worst.values()) >= 1e4, worst
