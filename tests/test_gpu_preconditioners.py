"""GPU tests (-m gpu) of the PCG's preconditioners AS OPERATORS: the multigrid hierarchy's numbers, the dense
coarsest inverse and z = M^-1 r of block-Jacobi, the chain segments and the multigrid cycle are read out of the
device (the diagnostic entries of include/sim3opt.h) and compared with tests/amg_ref.py in long double.  CG converges
with any SPD M^-1, so the parity tests of test_gpu_parity.py cannot see a wrong Galerkin term, sign, damping, visit
count or stale FP32 copy; these can (tests/test_amg_ref.py asserts that each such defect moves z by >= 1e4 x the
tolerance used here).

Three kinds of check:
  exact ........ FP32 copies, diagH, patterns, "a read-out changes nothing": array_equal.
  derived ...... P_0 = Ad(S_v): 16 u B entrywise; each Galerkin product and W, formed by the reference from the
                 DEVICE's level above: gamma |P|^T |A| |P| entrywise, gamma = (k + 16) u (k u for plain sums).
  measured ..... Minv, dense inverse, chain, the cycle: noise = |float64 restatement - long double| (kernel-style
                 elimination, another summation order), relative, max norm over the case, floored at 4u; the device
                 must be within 32 x noise of the long-double result.  Each case prints noise and the device's
                 ratio (-s); DESIGN.md 5a records the table.
"""
import numpy as np
import pytest

from sim3opt_amd import lib as L, synth
import amg_ref as R
import kitti_graph as K

LD, U = R.LD, R.U
pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not R.longdouble_ok(), reason="np.longdouble has no 64-bit mantissa here")]
# (dampings are given relative to max diag(H): 1e-7 lightly damped, 1e-3 g2o's usual, 1 damping-dominated)


# ------------------------------------------------------------------------------------------------ graphs
def spd_info(m, seed):
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((m, 7, 7)) * 0.3
    return np.einsum("kij,klj->kil", M, M) + np.eye(7)


def graph_of(name):
    synth.DRIFT_TARGET = 0.05
    if name == "m400":
        return synth.manhattan(400, 4000, dims=(6, 6, 10))
    if name == "m400_far":  # the same graph in units 50 times smaller: |t| ~ 300, cond(W) ~ |t|^4
        g = dict(synth.manhattan(400, 4000, dims=(6, 6, 10)))
        g["states"], g["meas"] = g["states"].copy(), g["meas"].copy()
        g["states"][:, 4:7] *= 50.0
        g["meas"][:, 4:7] *= 50.0
        return g
    if name == "m400_shuffled":
        # The generator inserts the vertices in walk order, so EVERY row has a block to row i - 1; vertices inserted
        # in a seeded random order (vertex 0, the fixed one, stays first) give the rows without one.
        g = dict(synth.manhattan(400, 4000, dims=(6, 6, 10)))
        perm = np.concatenate([[0], 1 + np.random.default_rng(17).permutation(g["states"].shape[0] - 1)])
        inv = np.argsort(perm)
        g["states"], g["fixed"] = g["states"][perm], np.asarray(g["fixed"])[perm]
        g["v0"], g["v1"] = inv[g["v0"]].astype(np.int32), inv[g["v1"]].astype(np.int32)
        return g
    if name == "m1500":
        return synth.manhattan(1500, 15000, dims=(14, 14, 8))
    if name == "chain_150":
        return synth.chain_loop(150, 300)
    if name == "chain_519":
        return synth.chain_loop(519, 1038)
    if name == "chain_150_parallel":  # every fourth odometry edge twice: sub_cnt > 1 between consecutive rows
        g = dict(synth.chain_loop(150, 300))
        odo = np.flatnonzero(np.abs(g["v1"].astype(int) - g["v0"].astype(int)) == 1)[::4]
        for k in ("v0", "v1", "meas"):
            g[k] = np.concatenate([g[k], g[k][odo]])
        return g
    if name == "kitti_one":
        return K.build_direct_graph(True)
    if name == "kitti_all":
        return K.build_direct_graph(False)
    raise KeyError(name)


def mk(name, info=False, huber=0.0, optimize=0, **opts):
    g = graph_of(name)
    o = dict(fix_small_angle_b=1, fd_delta=1e-6, linear_solver=0)
    o.update(opts)
    G = L.Graph(**o)
    G.add_vertices(g["states"], g["fixed"])
    G.add_edges(g["v0"], g["v1"], g["meas"], info=spd_info(g["v0"].shape[0], 7) if info else None,
                kernel=1 if huber else 0, kernel_delta=huber)
    G.initialize()
    if optimize:
        assert G.optimize(optimize) == optimize
    G.linearize()
    G._free = np.flatnonzero(np.asarray(g["fixed"]) == 0)
    return G


def system(G):
    rp, ci, blk, b = G.get_system()
    maxdiag = float(np.abs(blk[rp[:-1]].diagonal(0, 1, 2)).max())
    return dict(rp=rp, ci=ci, blk=blk, b=b, S=G.get_vertices()[G._free], maxdiag=maxdiag)


def rhs_set(s, seed=0):
    """The system's own b, four seeded Gaussian vectors, one near-kernel mode Ad(S_v) g (range of P_0)."""
    rng = np.random.default_rng(seed)
    near = np.einsum("irc,c->ir", R.adjoint(s["S"], np.float64), rng.standard_normal(7)).ravel()
    return np.stack([s["b"]] + [rng.standard_normal(s["b"].shape[0]) for _ in range(4)] + [near])


def levels_of(G, lam):
    st = G.amg_structure()
    fp32 = bool(G.options().amg_fp32)
    return st, [G.amg_level_numbers(lam, l, s["nb"], s["nnzb"], fp32=fp32) for l, s in enumerate(st)]


def report(what, noise, err):
    ratio = err / noise
    print(f"[precond] {what}: noise {noise:.2e}  device {err:.2e} = {ratio:.2f} x noise (limit 32)")
    return ratio


def within(what, dev, z64, zld):
    noise, tol = R.noise_and_tol(z64, zld)
    err = R.relerr(dev, zld)
    report(what, noise, err)
    assert err <= tol, (what, noise, err)


# ------------------------------------------------------------------------------------------------ exact checks
@pytest.mark.parametrize("name,opts", [("m400", dict(amg_coarsest=16)), ("m1500", dict(amg_coarsest=16)),
                                       ("kitti_all", dict(amg_coarsest=46))])
def test_fp32_copies_patterns_and_diagonals_are_exact(name, opts):
    G = mk(name, preconditioner=2, **opts)
    s = system(G)
    st = G.amg_structure()
    und = None
    # lambda = 0 first: the undamped diagonal itself (D + 0 W is exact); then three set-ups in a row: the refresh.
    # (KITTI-00 without damping is too close to singular to rely on its unpivoted set-up: there diagH is pinned by
    # the bound below and by the Galerkin test, which compares it with the product.)
    first = 0.0 if name != "kitti_all" else 1e-5
    for lam_rel in (first, 1e-3, 1.0, 1e-7):
        lam = lam_rel * s["maxdiag"]
        _, lv = levels_of(G, lam)
        for l, (h, d) in enumerate(zip(st, lv)):
            # the device's pattern is the host read-out's
            assert np.array_equal(d["rowptr"], h["rowptr"]) and np.array_equal(d["colidx"], h["colidx"])
            # FP32 copy = float32(blocks) bit for bit: level 0 undamped, coarse levels with the damped diagonal
            assert np.array_equal(d["vals32"], d["vals"].astype(np.float32)), (lam_rel, l)
            if l == 0:
                assert np.array_equal(d["vals"], s["blk"])
        if und is None:
            und = [d["vals"].copy() for d in lv]
            for l in range(1, len(st)):
                und[l][st[l]["rowptr"][:-1]] = lv[l]["diagH"]
                if lam_rel == 0.0:  # diagH = the Galerkin diagonal before damping, bit for bit
                    assert np.array_equal(lv[l]["diagH"], lv[l]["vals"][st[l]["rowptr"][:-1]])
        if lam_rel > 0.0:
            for l in range(1, len(st)):
                dg = st[l]["rowptr"][:-1]
                off = np.ones(st[l]["nnzb"], dtype=bool)
                off[dg] = False
                assert np.array_equal(lv[l]["vals"][off], und[l][off])  # a trial refreshes the diagonal only
                assert np.array_equal(lv[l]["diagH"], und[l][dg])
                # the damped diagonal: D + lambda W, one rounding per operation (or one fused): 2u relative to |D| + lambda |W|
                ref = lv[l]["diagH"].astype(LD) + LD(lam) * lv[l]["W"].astype(LD)
                bound = 2 * U * (np.abs(lv[l]["diagH"]) + lam * np.abs(lv[l]["W"]))
                assert (np.abs(lv[l]["vals"][dg].astype(LD) - ref) <= bound).all()


def test_fp32_pair_layout_sees_odd_and_even_block_counts():
    """The FP32 copies are stored as pairs of blocks: a level with an odd block count ends in half a pair.  The cases
    of the test above must hold both parities (asserted here on the host read-out, so that a change of the
    generators cannot silently drop one)."""
    seen = set()
    for name, cap in (("m400", 16), ("m1500", 16), ("kitti_all", 46)):
        g = graph_of(name)
        G = L.Graph(preconditioner=2, amg_coarsest=cap)
        G.add_vertices(g["states"], g["fixed"])
        G.add_edges(g["v0"], g["v1"], g["meas"])
        seen |= {h["nnzb"] % 2 for h in G.amg_structure()}
    assert seen == {0, 1}


def _stats_tuple(G):
    return [tuple(getattr(s, f) for f, _ in s._fields_) for s in G.stats()]


@pytest.mark.parametrize("name,prec,opts", [("m400", 2, dict(amg_coarsest=16)), ("kitti_one", 1, {}), ("m400", 0, {}),
                                            ("m400", 2, dict(amg_coarsest=16, amg_additive=1))])
def test_readouts_change_nothing(name, prec, opts):
    """solve and optimize(3) with read-outs and M^-1 applications interleaved are bit-identical to a fresh graph
    without them (pcg_graph on: the default)."""
    def run(diag):
        G = mk(name, preconditioner=prec, **opts)
        assert G.preconditioner_in_use() == prec and G.options().pcg_graph == 1
        s = system(G)
        lam = 1e-3 * s["maxdiag"]
        r = rhs_set(s)[:3]

        def poke(k):
            if not diag:
                return
            G.preconditioner_apply(prec, lam * 10.0 ** k, r)
            G.preconditioner_apply(0, lam, r[0])
            if prec == 2:
                st = G.amg_structure()
                G.amg_level_numbers(7.0 * lam, len(st) - 1, st[-1]["nb"], st[-1]["nnzb"])
                G.amg_coarsest_inverse(3.0 * lam, st[-1]["nb"])
        poke(1)
        x1, it1, rr1 = G.solve(lam)
        poke(-2)
        x2, it2, rr2 = G.solve(10 * lam)
        poke(0)
        assert G.optimize(3) == 3
        poke(2)
        v = G.get_vertices()
        G.linearize()
        poke(-1)
        x3, it3, rr3 = G.solve(lam)
        return (x1, x2, x3, v), (it1, it2, it3, rr1, rr2, rr3), _stats_tuple(G)

    a, b = run(False), run(True)
    for u, v in zip(a[0], b[0]):
        assert np.array_equal(u, v)
    assert a[1] == b[1] and a[2] == b[2]
    print(f"[precond] read-outs change nothing, prec {prec}: PCG iterations {a[1][:3]}")
    if prec == 0:
        assert a[1][0] > 16  # (more iterations than one captured graph holds: the replay ran)


def test_readouts_refuse_what_they_cannot_do():
    G = mk("chain_150", preconditioner=0)
    s = system(G)
    with pytest.raises(L.Sim3OptError):
        G.preconditioner_apply(2, 1.0, s["b"])  # no hierarchy on this graph
    with pytest.raises(L.Sim3OptError):
        G.preconditioner_apply(1, 1.0, s["b"])
    with pytest.raises(L.Sim3OptError):
        G.amg_coarsest_inverse(1.0, 8)
    with pytest.raises(L.Sim3OptError) as e:
        G.preconditioner_apply(0, -1.0, s["b"])  # a negative damping
    assert e.value.code == L.ERR_ARG
    # A failed set-up pivot is reported, not hidden behind the block-Jacobi fallback of a solve: with the rotations
    # frozen (dof_mask 0x78) their rows of H are zero, and without damping the first pivot of every block is 0.
    H = mk("m400", preconditioner=2, amg_coarsest=16, dof_mask=0x78)
    hs = system(H)
    for prec in (2, 0):
        with pytest.raises(L.Sim3OptError) as e:
            H.preconditioner_apply(prec, 0.0, hs["b"])
        assert e.value.code == L.ERR_STATE
    with pytest.raises(L.Sim3OptError) as e:
        H.amg_coarsest_inverse(0.0, H.amg_structure()[-1]["nb"])
    assert e.value.code == L.ERR_STATE
    z = H.preconditioner_apply(2, 1e-3 * hs["maxdiag"], hs["b"])  # ... and with damping the same graph sets up
    assert np.isfinite(z).all()


# ------------------------------------------------------------------------------------------------ derived bounds
@pytest.mark.parametrize("name,optimize", [("m400", 0), ("m400", 3), ("m400_far", 0), ("kitti_all", 0)])
def test_prolongation_blocks_are_the_adjoint(name, optimize):
    """P_0 = Ad(S_v) entrywise within 16 u B, B = the entry's expression with every term replaced by its absolute
    value (amg_ref.adjoint_abs): R is at most 4 operations deep on products of quaternion entries, [t]x R adds three,
    s R one -- 16 covers the deepest chain twice over.  sim3::R_from_quat does not normalise q; neither does the
    reference.  optimize = 3: scales != 1."""
    G = mk(name, preconditioner=2, amg_coarsest=64, optimize=optimize)
    s = system(G)
    if optimize:
        assert np.abs(s["S"][:, 7] - 1).max() > 1e-6
    st = G.amg_structure()
    P = G.amg_level_numbers(1e-3 * s["maxdiag"], 0, st[0]["nb"], st[0]["nnzb"])["P"]
    ref, B = R.adjoint(s["S"], LD), R.adjoint_abs(s["S"])
    d = np.abs(P.astype(LD) - ref)
    worst = float((d[B > 0] / (16 * U * B[B > 0])).max())
    print(f"[precond] P0 {name} optimize={optimize}: worst entry at {worst:.3f} of 16 u B")
    assert (d <= 16 * U * B).all()
    assert (P[B == 0] == 0).all()


@pytest.mark.parametrize("name,opts,info,huber", [("m400", dict(amg_coarsest=16), False, 0.0),
                                                  ("m1500", dict(amg_coarsest=16), False, 0.0),
                                                  ("m400", dict(amg_coarsest=16, amg_passes=(3, 3, 3)), True, 0.5),
                                                  ("m400_far", dict(amg_coarsest=16), False, 0.0)])
def test_galerkin_products_and_W_forward_error(name, opts, info, huber):
    """Each product on its own: the reference forms level l + 1 in long double from the DEVICE's level l (and the
    device's P_0, checked above), so the bound is that of one fixed-order sum of k terms, each a 7-term inner product
    of 7-term inner products (Higham, Accuracy and Stability, 3.1 / 3.5): gamma = (k + 16) u on |P|^T |A| |P|;
    plain sums below level 1: gamma = k u on sum |A|."""
    G = mk(name, preconditioner=2, info=info, huber=huber, **opts)
    s = system(G)
    st, lv = levels_of(G, 1e-3 * s["maxdiag"])
    assert len(st) >= 3
    for l in range(len(st) - 1):
        d, c = lv[l], lv[l + 1]
        und = d["vals"].copy()
        if l > 0:
            und[st[l]["rowptr"][:-1]] = d["diagH"]
        cund = c["vals"].copy()
        cund[st[l + 1]["rowptr"][:-1]] = c["diagH"]
        rows = R._row_of_block(st[l]["rowptr"])
        P = d["P"].astype(LD) if l == 0 else None
        rp, ci, C, cnt = R.galerkin(und, rows, st[l]["colidx"], st[l]["agg"], P, LD)
        assert np.array_equal(rp, st[l + 1]["rowptr"]) and np.array_equal(ci, st[l + 1]["colidx"])
        _, _, Cabs, _ = R.galerkin(np.abs(und), rows, st[l]["colidx"], st[l]["agg"], None if P is None else np.abs(P), LD)
        gam = ((cnt + 16) if l == 0 else cnt)[:, None, None] * U
        err = np.abs(cund.astype(LD) - C)
        used = float((err / (gam * Cabs + 1e-300)).max())
        assert (err <= gam * Cabs).all(), (l, used)
        # W
        src = d["P"] if l == 0 else d["W"]
        Wref = R.wsum(src, st[l]["agg"], l == 0, LD)
        Wabs = R.wsum(np.abs(src), st[l]["agg"], l == 0, LD)
        k = np.bincount(st[l]["agg"])
        gw = ((k + 16) if l == 0 else k)[:, None, None] * U
        werr = np.abs(c["W"].astype(LD) - Wref)
        wused = float((werr / (gw * Wabs + 1e-300)).max())
        assert (werr <= gw * Wabs).all(), (l, wused)
        print(f"[precond] galerkin {name} level {l}->{l + 1}: up to {int(cnt.max())} fine blocks per coarse block, worst "
              f"entry at {used:.3f} of the bound (W: {wused:.3f})")


# ------------------------------------------------------------------------------------------------ measured: Minv
@pytest.mark.parametrize("name,lam_rel,want_cond", [("m400", 1e-7, 0), ("m400", 1e-3, 0), ("m1500", 1.0, 0),
                                                   ("m400_far", 1.0, 1e8)])
def test_smoother_inverses_of_every_level(name, lam_rel, want_cond):
    G = mk(name, preconditioner=2, amg_coarsest=16)
    s = system(G)
    lam = lam_rel * s["maxdiag"]
    st, lv = levels_of(G, lam)
    om = G.options().amg_omega
    worst = 0.0
    for l, d in enumerate(lv):
        D = s["blk"][s["rp"][:-1]] + lam * np.eye(7) if l == 0 else d["vals"][st[l]["rowptr"][:-1]]
        worst = max(worst, float(np.linalg.cond(D).max()))
        mld = LD(om) * R.accurate_inverse(D, LD)
        assert np.abs(D.astype(LD) @ mld / LD(om) - np.eye(7, dtype=LD)).max() < 1e-9  # (the reference inverted)
        m64 = om * R.gj_inverse(D)
        within(f"Minv {name} lambda {lam_rel:g} level {l}", d["Minv"], m64, mld)
    if want_cond:  # coverage: a level whose D + lambda W has condition >= 1e8 (large |t|)
        assert worst >= want_cond, worst


# ------------------------------------------------------------------------------------------------ measured: dense inverse
DENSE_CASES = [("m400", dict(amg_coarsest=8), 14), ("kitti_all", dict(amg_coarsest=46), 28),
               ("kitti_all", dict(amg_coarsest=46), 14), ("chain_519", dict(amg_coarsest=64), 14),
               ("chain_519", dict(amg_coarsest=64), 28), ("m1500", dict(amg_coarsest=174), 14)]


def test_dense_inverse_cases_cover_the_kernel_paths():
    """Coverage is a condition on the cases (host read-out: no GPU work): one tile, a 7-row tail, the 28 -> 14 -> 7
    hand-over through the look-ahead workgroup, no ragged tile, more than 1024 unknowns, both parities of the step
    count (the ping-pong decides which buffer is filled first).  NOT produced: k_amg_dense_gj_first<7>, which needs a
    coarsest level of ONE block row -- the aggregation stops at more than amg_coarsest / 2 >= 4 rows."""
    seen = set()
    for name, opts, pivot in DENSE_CASES:
        g = graph_of(name)
        G = L.Graph(preconditioner=2, **opts)
        G.add_vertices(g["states"], g["fixed"])
        G.add_edges(g["v0"], g["v1"], g["meas"])
        nd = 7 * int(G.amg_hierarchy()[0][-1])
        sched = R.pivot_schedule(nd, pivot)
        seen |= {"tile" if nd <= 64 else "", "tail" if sched[-1] == 7 else "", "mult64" if nd % 64 == 0 else "",
                 "big" if nd > 1024 else "", "28-14-7" if sched[-3:] == [28, 14, 7] else "", f"parity{len(sched) % 2}",
                 f"first{sched[0]}"}
    assert {"tile", "tail", "mult64", "big", "28-14-7", "parity0", "parity1", "first14", "first28"} <= seen, seen


def _ld_inverse(A, X0):
    """Long-double inverse by two residual corrections of a float64 one, X <- X + X0 (I - A X): the residual (the n^3
    product) in long double, the small correction in float64.  Returns (X, first residual, second residual): the
    second is already at the long-double floor u_ld |A||X| when it is 2^9 or more below the first (2^11 = u / u_ld is
    the most there is), and the second correction removes what of it is not rounding."""
    X = X0.astype(LD)
    eye = np.eye(A.shape[0], dtype=LD)
    Al = A.astype(LD)
    res = []
    for _ in range(2):
        E = eye - Al @ X
        res.append(float(np.abs(E).max()))
        X = X + (X0 @ E.astype(np.float64)).astype(LD)
    return X, res[0], res[1]


@pytest.mark.parametrize("name,opts,pivot", DENSE_CASES)
def test_dense_coarsest_inverse(name, opts, pivot):
    G = mk(name, preconditioner=2, amg_pivot=pivot, **opts)
    s = system(G)
    lam = 1e-3 * s["maxdiag"]
    st, lv = levels_of(G, lam)
    c, h = lv[-1], st[-1]
    A = R.dense_of(h["nb"], R._row_of_block(h["rowptr"]), h["colidx"], c["vals"], np.float64)
    Xd = G.amg_coarsest_inverse(lam, h["nb"])
    X64 = R.block_gj_inverse(A, pivot)
    Xld, e0, e1 = _ld_inverse(A, np.linalg.inv(A))
    assert e0 < 1e-3 and e1 <= max(e0 / 512, 1e-17)  # (the reference sits >= 2^9 below float64 rounding: far below noise)
    within(f"dense inverse {name} n={A.shape[0]} pivot {pivot} ({len(R.pivot_schedule(A.shape[0], pivot))} steps)", Xd, X64, Xld)
    eye = np.eye(A.shape[0], dtype=LD)
    res64 = float(np.abs(A.astype(LD) @ X64.astype(LD) - eye).max())
    resd = float(np.abs(A.astype(LD) @ Xd.astype(LD) - eye).max())
    noise = max(res64, 4 * U)
    report(f"dense ||A X - I|| {name} pivot {pivot}", noise, resd)
    assert resd <= 32 * noise


# ------------------------------------------------------------------------------------------------ measured: the cycle
# Kernel instantiations launched (engine_amg.hip), by configuration:
#   spmv_mode  FP32: level 0 <true,1> <true,2> every multiplicative fp32 case; coarse <false,1> <false,3> three or more
#              levels (c2, c3, ...); coarse <false,2> (the smoothing pass between two visits) visits >= 2 below level 1
#              (c2, c3, c5) -- FP64: the same with amg_fp32 = 0 (c4: V-cycle, no <false,2>; c6: {3,3,3})
#   amg_restrict  k_amg_restrict0 with Minv_c (three or more levels) and without (c1, c13: two levels);
#              k_amg_restrict with Minv_c (four levels: c3 ...) and without (into the dense level)
#   amg_prolong  <true> every case (multiplicative: in place; additive c7, c8: d_z -> d_az); <false> is launched on
#              partitioned levels only (one rank prolongs coarse levels inside mode 3): out of scope here
#   dense_inverse  first / step <14> and <28> (c6, c9), step <7> (odd coarsest: c4 ... 5 rows)
CYCLE_CASES = {
    "c1_two_levels": ("m1500", dict(amg_coarsest=256), {}, 1e-3),
    "c2_three_levels": ("m1500", dict(amg_coarsest=64), {}, 1e-7),
    "c3_four_levels": ("m1500", dict(amg_coarsest=16), {}, 1e-3),
    "c4_V_fp64": ("m1500", dict(amg_coarsest=16, amg_cycle=(1, 1, 1, 1), amg_fp32=0), {}, 1e-3),
    "c5_122_damped": ("m1500", dict(amg_coarsest=16, amg_cycle=(1, 2, 2, 2)), {}, 1.0),
    "c6_333_fp64_pivot28": ("m400", dict(amg_coarsest=16, amg_cycle=(3, 3, 3, 3), amg_fp32=0, amg_pivot=28), {}, 1e-3),
    "c7_additive": ("m400", dict(amg_coarsest=16, amg_additive=1), {}, 1e-3),
    "c8_additive_fp64_over1": ("m400", dict(amg_coarsest=16, amg_additive=1, amg_fp32=0, amg_over=(1.0, 1.0)), {}, 1e-7),
    "c9_over1_pivot28": ("m400", dict(amg_coarsest=16, amg_over=(1.0, 1.0), amg_pivot=28), {}, 1e-3),
    "c10_virtual_ranks": ("m1500", dict(amg_coarsest=16, amg_virtual_ranks=4), {}, 1e-3),
    "c11_info_huber": ("m400", dict(amg_coarsest=16), dict(info=True, huber=0.5), 1e-3),
    "c12_after_optimize": ("m400", dict(amg_coarsest=16), dict(optimize=3), 1e-3),
    "c13_kitti": ("kitti_all", dict(), {}, 1e-3),
}
LEVELS = {"c1_two_levels": 2, "c2_three_levels": 3, "c3_four_levels": 4}


def reference_cycles(G, s, lam):
    o = G.options()
    st = G.amg_structure()
    aggs = [h["agg"] for h in st[:-1]]
    use = G.amg_in_use()
    kw = dict(omega=o.amg_omega, fp32=bool(o.amg_fp32), additive=bool(o.amg_additive), pivot=28 if o.amg_pivot >= 28 else 14)
    ck = dict(visits=tuple(use["cycle"]), over=(o.amg_over[0], o.amg_over[1]), additive=bool(o.amg_additive))
    out = []
    for dt in (np.float64, LD):
        lv = R.build(dt, s["rp"], s["ci"], s["blk"], s["S"], aggs, lam, **kw)
        out.append(R.Cycle(lv, **ck))
    return st, out[0], out[1]


@pytest.mark.parametrize("case", list(CYCLE_CASES))
def test_multigrid_cycle_is_the_reference_operator(case):
    """z = M^-1 r for b, four Gaussian vectors and a near-kernel mode (the coarse correction does all the work there).
    The over-correction switched off after a PCG breakdown (amg_over_on = false) is not reachable through options;
    amg_over = (1, 1) launches the same kernels with the same factor 1 (c8, c9)."""
    name, opts, extra, lam_rel = CYCLE_CASES[case]
    G = mk(name, preconditioner=2, **opts, **extra)
    s = system(G)
    lam = lam_rel * s["maxdiag"]
    st, c64, cld = reference_cycles(G, s, lam)
    if case in LEVELS:
        assert len(st) == LEVELS[case]
    if "virtual" in case:
        assert not np.array_equal(st[0]["agg"], mk(name, preconditioner=2, amg_coarsest=16).amg_structure()[0]["agg"])
    rs = rhs_set(s)
    zd = G.preconditioner_apply(2, lam, rs)
    z64 = np.stack([c64.apply(r) for r in rs])
    zld = np.stack([cld.apply(r.astype(LD)) for r in rs])
    within(f"cycle {case} ({len(st)} levels, lambda {lam_rel:g})", zd, z64, zld)
    # and right-hand side by right-hand side (the near-kernel mode's z is orders larger than the others')
    for q in range(rs.shape[0]):
        noise, tol = R.noise_and_tol(z64[q], zld[q])
        assert R.relerr(zd[q], zld[q]) <= tol, (q, noise, R.relerr(zd[q], zld[q]))


@pytest.mark.parametrize("case", ["c3_four_levels", "c7_additive"])
def test_device_operator_is_symmetric(case):
    name, opts, extra, lam_rel = CYCLE_CASES[case]
    G = mk(name, preconditioner=2, **opts, **extra)
    s = system(G)
    lam = lam_rel * s["maxdiag"]
    _, c64, _ = reference_cycles(G, s, lam)
    rng = np.random.default_rng(9)
    u, v = rng.standard_normal(s["b"].shape[0]), rng.standard_normal(s["b"].shape[0])
    zd = G.preconditioner_apply(2, lam, np.stack([u, v]))
    mu, mv = c64.apply(u), c64.apply(v)
    dot = lambda a, b: float(np.dot(a.astype(LD), b.astype(LD)))
    ref = max(abs(dot(u, mv) - dot(v, mu)), 64 * U * float(np.linalg.norm(u) * np.linalg.norm(mv)))
    dev = abs(dot(u, zd[1]) - dot(v, zd[0]))
    print(f"[precond] symmetry {case}: float64 restatement {ref:.2e}, device {dev:.2e} = {dev / ref:.2f} x")
    assert dev <= 32 * ref


# ------------------------------------------------------------------------------------------------ measured: chain, Jacobi
@pytest.mark.parametrize("name,seg,lam_rel", [("kitti_one", 256, 1e-3), ("kitti_one", 7, 1e-7), ("kitti_all", 2, 1e-3),
                                              ("kitti_all", 256, 1.0), ("chain_150", 4, 1e-3), ("m400", 256, 1e-3),
                                              ("m400_shuffled", 256, 1e-3),
                                              ("chain_150_parallel", 7, 1e-3)])
def test_chain_segments_are_the_reference_operator(name, seg, lam_rel):
    G = mk(name, preconditioner=1, chain_segment=seg)
    assert G.preconditioner_in_use() == 1
    s = system(G)
    rows = R._row_of_block(s["rp"])
    links = np.bincount(rows[s["ci"] == rows - 1], minlength=rows.max() + 1)
    if name == "chain_150":
        assert (s["rp"].shape[0] - 1) % seg == 1  # a one-row last segment
    if name == "m400_shuffled":
        assert (links[1:] == 0).mean() > 0.5  # most rows have no block to row i - 1
    if name == "chain_150_parallel":
        assert links.max() > 1  # parallel edges between consecutive vertices: sub_cnt > 1
    lam = lam_rel * s["maxdiag"]
    rs = rhs_set(s)
    zd = G.preconditioner_apply(1, lam, rs)
    a = (s["rp"], s["ci"], s["blk"], lam, seg)
    z64 = np.stack([R.chain_apply(*a, r, np.float64) for r in rs])
    zld = np.stack([R.chain_apply(*a, r, LD) for r in rs])
    within(f"chain {name} segment {seg} lambda {lam_rel:g}", zd, z64, zld)


@pytest.mark.parametrize("name,prec,lam_rel", [("m400", 0, 1e-3), ("m400_far", 2, 1e-7), ("kitti_all", 1, 1.0)])
def test_block_jacobi_is_the_reference_operator(name, prec, lam_rel):
    """prec = 0 through the read-out on graphs initialised with each of the three preconditioners."""
    G = mk(name, preconditioner=prec, **(dict(amg_coarsest=16) if prec == 2 else {}))
    s = system(G)
    lam = lam_rel * s["maxdiag"]
    rs = rhs_set(s)
    zd = G.preconditioner_apply(0, lam, rs)
    z64 = np.stack([R.jacobi_apply(s["rp"], s["blk"], lam, r, np.float64) for r in rs])
    zld = np.stack([R.jacobi_apply(s["rp"], s["blk"], lam, r, LD) for r in rs])
    within(f"block-Jacobi {name} lambda {lam_rel:g}", zd, z64, zld)
