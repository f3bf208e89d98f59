"""The exact block Cholesky, its solves, the selected inversion and the blocks of the inverse outside the pattern
(direct_kernels.hpp, selinv_kernels.hpp, cov_kernels.hpp) as OPERATORS on the device: every buffer is read out
(Graph.debug_factor) and every block compared with its long-double value computed from the device's own inputs to that
block (tests/factor_ref.py), on the patterns of tests/factor_cases.py whose paths through the kernels
test_factor_ref.py pins on the CPU.  Bounds and their derivations: DESIGN.md, "How the exact factorisation is tested as
an operator"."""
import ctypes
import functools

import numpy as np
import pytest

from conftest import gpu_available
from sim3opt_amd import lib as L
import cov_ref as CR
import dist_helpers as DH
import factor_cases as C
import factor_ref as F
import lm_cases as LC
import lm_ref as R

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

BITS = ("Aperm", "bp", "L", "Dinv", "y", "xp", "x")


@functools.lru_cache(maxsize=None)
def case(name):
    """The case's graph with the exact solver, linearised; its plan and injected values.  Shared, left unchanged."""
    g = C.CASES[name]()
    G = C.graph_of(g, linear_solver=1)
    G.initialize()
    G.linearize()
    P = F.plan_of(G)
    rp, ci = G.system_pattern()
    vals, b = C.injected(g, rp, ci)
    return dict(g=g, G=G, P=P, rp=rp, ci=ci, vals=vals, b=b)


def held(P, vals, b, lam, d, what, exempt=None):
    if exempt is None:
        r = F.check(P, vals, b, lam, d)
    else:
        with np.errstate(all="ignore"):
            r = F.check(P, vals, b, lam, d, with_solve=False, with_selinv=False, exempt=exempt)
    print(what, " ".join(f"{k} {v[0]:.3f}" for k, v in r.items()))
    bad = {k: v for k, v in r.items() if not v[0] <= 1.0}
    assert not bad, f"{what}: error / bound and the worst block (column for Ldiag, Dinv, y, xp): {bad}"
    return r


# ------------------------------------------------------------------------------------------------ factor and solve
@pytest.mark.parametrize("lam", C.LAMBDAS)
@pytest.mark.parametrize("name", sorted(C.CASES))
def test_every_block_of_the_factorisation_and_the_solves(name, lam):
    c = case(name)
    G, P = c["G"], c["P"]
    d0 = G.debug_factor(0, lam, c["vals"], c["b"])
    d1 = G.debug_factor(1, lam, c["vals"], c["b"], selinv=True)
    assert np.array_equal(d0["bord"], P["bord"]) and np.array_equal(d0["brow"], P["brow"])
    for k in BITS:  # the two contexts run the same plan: the same bits
        assert np.array_equal(d0[k], d1[k]), k
    must_fail, must_pass, _, between = F.fail_expected(P, d1, lam)
    assert between == 0 and must_pass and not must_fail and d0["fail"] == 0 and d1["fail"] == 0
    # (the per-vertex scaling puts pivots of the small vertices below 1e-13 of the largest diagonal entry on some cases)
    assert d1["singular"] == F.singular_expected(P, c["vals"], c["rp"], d1)
    held(P, c["vals"], c["b"], lam, d1, f"{name} lambda {lam:g}:")


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_the_linearisation_s_own_system_and_solve(name):
    """Nothing injected: the factor of the last linearisation, x the bits of Graph.solve."""
    c = case(name)
    G, P = c["G"], c["P"]
    lam = 1e-2
    _, _, vals, b = G.get_system()
    d = G.debug_factor(0, lam)
    assert np.array_equal(d["x"].ravel(), G.solve(lam)[0]) and d["fail"] == 0
    held(P, vals, b, lam, d, f"{name} (linearised):")
    assert np.array_equal(G.get_system()[2], vals)


# ------------------------------------------------------------------------------------------------ schedules
@pytest.mark.parametrize("name", ["clique_12_tail20", "kitti_all_loops"])
def test_every_schedule_gives_the_same_bits(name, monkeypatch):
    c = case(name)
    lam = 1e-2
    seen, groups = [], set()
    for sub in (8, 48):
        for wg in (64, 192, 512):
            monkeypatch.setenv("SIM3OPT_DIRECT_SUBTREE", str(sub))
            monkeypatch.setenv("SIM3OPT_DIRECT_WG_SUB", str(wg))
            G = C.graph_of(c["g"], linear_solver=1)
            G.initialize()
            P = F.plan_of(G)  # (the host plan reads the same knobs)
            groups.add(P["ngroups"])
            d = G.debug_factor(1, lam, c["vals"], c["b"], selinv=True)
            d0 = G.debug_factor(0, lam, c["vals"], c["b"])
            assert all(np.array_equal(d0[k], d[k]) for k in BITS)
            held(P, c["vals"], c["b"], lam, d, f"{name} subtree {sub} wg {wg}:")
            key = list(zip(P["perm"][P["lrow"]].tolist(), P["perm"][P["lcol"]].tolist()))
            order = np.argsort(np.array([a * P["nb"] + b for a, b in key]), kind="stable")
            byrow = np.argsort(P["perm"])
            seen.append((sorted(key), d["L"][order], d["Z"][order], d["Dinv"][byrow], d["y"][byrow], d["x"]))
    assert len(groups) > 1  # the knob does move the schedule
    for s in seen[1:]:
        assert s[0] == seen[0][0]
        for a, b in zip(s[1:], seen[0][1:]):
            assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------ selected inverse
@pytest.mark.parametrize("name", ["parallel", "star_16", "clique_66", "clique_12_tail20", "two_components",
                                  "kitti_all_loops"])
def test_marginals_returns_the_read_out_s_blocks(name):
    """sim3opt_marginals on every block of the pattern: the bits of Z of the read-out (whose every block the factor
    test holds against its long-double value)."""
    c = case(name)
    G, P = c["G"], c["P"]
    lam = 1e-2
    ids = np.nonzero(c["g"]["fixed"] == 0)[0]
    d = G.debug_factor(1, lam, selinv=True)
    _, _, vals, b = G.get_system()
    held(P, vals, b, lam, d, f"{name} (linearised, Z):")
    pairs = np.stack([ids[P["perm"][P["lrow"]]], ids[P["perm"][P["lcol"]]]], 1)
    assert np.array_equal(G.marginals(pairs, lam), d["Z"])
    if name == "two_components":  # (cross blocks of a forest are not on the pattern: test_blocks_outside_the_pattern)
        assert C.paths(P)["roots"] == 2


# ------------------------------------------------------------------------------------------------ outside the pattern
def _info_graph(name):
    g = dict(C.CASES[name]())
    g["info"] = LC.spd_info(np.random.default_rng(77), g["v0"].shape[0])
    G = L.Graph(linear_solver=1)
    G.add_vertices(g["states"], g["fixed"])
    G.add_edges(g["v0"], g["v1"], g["meas"], info=g["info"])
    G.initialize()
    G.linearize()
    return g, G


def _requests(T, nreq):
    """nreq columns: leaves of the elimination tree, deepest first (two leaves are never on the pattern)"""
    return C.leaves_of(T)[:nreq]


@pytest.mark.parametrize("nreq", [1, 2, 3, 5])
@pytest.mark.parametrize("name", ["clique_12_tail20", "chain_40", "two_components", "kitti_all_loops"])
def test_blocks_outside_the_pattern(name, nreq):
    """k_cov_paths / k_cov_pairs on real linearisations with non-diagonal information matrices over four decades:
    every pair among nreq vertices (1, 2, 3, 5: the last workgroup of four wavefronts is partly empty; one vertex
    alone has no pair outside the pattern and asks for its diagonal block only) and its reverse,
    against the long-double root-path recursion on the DEVICE's L and Dinv; the float64 recursion is the noise gauge
    (lm_ref.measured_ratio: 32 x noise, floored at 4 u, every block relative to its own largest entry)."""
    g, G = _info_graph(name)
    lam = 1e-2
    ids = np.nonzero(g["fixed"] == 0)[0]
    d = G.debug_factor(1, lam, selinv=True)
    P = F.plan_of(G)
    T = CR.Tree(P)
    cols = _requests(T, nreq)
    if name == "two_components" and nreq > 1:  # a column of each tree at least
        root = [j for j in range(T.nb) if T.parent[j] < 0]
        cols = [int(x) for x in dict.fromkeys(root + cols)][:max(nreq, 2)]
    pr = [(a, b) for a in cols for b in cols]
    rows = P["perm"]
    got = G.covariances([(ids[rows[a]], ids[rows[b]]) for a, b in pr], lam)
    # the same factor: the on-pattern pairs are the read-out's bits
    slot = {(int(i), int(j)): s for s, (i, j) in enumerate(zip(P["lrow"], P["lcol"]))}
    non = 0
    for q, (a, b) in enumerate(pr):
        if (max(a, b), min(a, b)) in slot:
            z = d["Z"][slot[(max(a, b), min(a, b))]]
            assert np.array_equal(got[q], z if a >= b else z.T)
            non += 1
    assert non >= len(cols)
    W64, Wld = F.root_paths(T, d["L"], d["Dinv"], cols, np.float64), F.root_paths(T, d["L"], d["Dinv"], cols, F.LD)
    off = [q for q, (a, b) in enumerate(pr) if (max(a, b), min(a, b)) not in slot]
    suffix = set()
    for q, (a, b) in enumerate(pr):
        assert np.array_equal(got[q], got[pr.index((b, a))].T)  # a pair and its reverse: exact transposes
    if off:
        z64 = np.stack([F.pair_block(T, W64, *pr[q], np.float64)[0] for q in off])
        zl = [F.pair_block(T, Wld, *pr[q], F.LD) for q in off]
        zld = np.stack([z[0] for z in zl])
        suffix = {z[1] for z in zl}
        cross = np.array([z[1] == 0 for z in zl])
        assert (got[off][cross] == 0).all()  # two trees: exactly zero
        if (~cross).any():
            keep = np.nonzero(~cross)[0]
            n64 = R.edge_scaled_err(z64[keep], zld[keep])
            ill = n64 > R.ILL
            m = R.measured_ratio(got[off][keep], z64[keep], zld[keep], ill)
            print(f"{name} {nreq} requests: {len(keep)} blocks outside the pattern, common suffixes {sorted(suffix)}, "
                  f"noise {m['noise']:.2e} ratio {m['ratio']:.3f}; ill {m['n_ill']} noise {m['noise_ill']:.2e} "
                  f"ratio {m['ratio_ill']:.3f}")
            assert m["ratio"] <= 1.0 and m["ratio_ill"] <= 1.0, m
            assert m["n_ill"] <= 0.1 * len(keep)
    if name == "two_components" and nreq > 1:
        assert 0 in suffix
    elif nreq > 1:
        assert off and suffix - {0}


def test_common_suffixes_of_1_8_9_and_17_blocks():
    """COV_BATCH = 8: a pair whose root paths share 1, 8, 9 and 17 blocks (one batch, a full one, one more, two and
    one more), on KITTI-00's tree (21 levels)."""
    g, G = _info_graph("kitti_all_loops")
    lam = 1e-2
    ids = np.nonzero(g["fixed"] == 0)[0]
    d = G.debug_factor(1, lam, selinv=True)
    P = F.plan_of(G)
    T = CR.Tree(P)
    want = C.suffix_pairs(T)
    pr = [want[n] for n in (1, 8, 9, 17)]
    cols = sorted({c for p in pr for c in p})
    got = G.covariances([(ids[P["perm"][a]], ids[P["perm"][b]]) for a, b in pr], lam)
    W64, Wld = F.root_paths(T, d["L"], d["Dinv"], cols, np.float64), F.root_paths(T, d["L"], d["Dinv"], cols, F.LD)
    z64 = np.stack([F.pair_block(T, W64, a, b, np.float64)[0] for a, b in pr])
    zl = [F.pair_block(T, Wld, a, b, F.LD) for a, b in pr]
    assert [z[1] for z in zl] == [1, 8, 9, 17]
    zld = np.stack([z[0] for z in zl])
    m = R.measured_ratio(got, z64, zld, np.zeros(4, bool))
    print(f"suffixes 1 8 9 17: noise {m['noise']:.2e} ratio {m['ratio']:.3f}")
    assert m["ratio"] <= 1.0, m


# ------------------------------------------------------------------------------------------------ fail and singular
@pytest.mark.parametrize("where", ["bottom", "top"])
def test_a_negative_definite_source_block_fails_its_column_only(where):
    c = case("clique_12_tail20")
    G, P = c["G"], c["P"]
    T = CR.Tree(P)
    top0 = P["lcolp"][P["gptr"][P["ngroups"] - 1]]
    assert 0 < top0 < P["nb"]
    j = 0 if where == "bottom" else int(top0)  # (the first column of a bottom group / of the top group)
    vals, b = c["vals"].copy(), c["b"]
    vals[c["rp"][P["perm"][j]]] = -np.eye(7)
    for lam in (0.0, 1e-2):
        d = G.debug_factor(1, lam, vals, b, selinv=True)
        must_fail, _, bad, _ = F.fail_expected(P, d, lam)
        assert must_fail and bad[j] and d["fail"] != 0
        path = np.zeros(P["nb"], bool)
        path[T.path(j)] = True
        assert not (bad & ~path).any()  # nothing off the column's root path fails
        # ... and every column off it is held as ever (a failed pivot is replaced by 1: the path's own blocks are
        # garbage, and the backward solve and the inverse, which start at the root, with them)
        off = ~path[P["lcol"]]
        assert (~path).sum() >= 10 and all(np.isfinite(d[k][off if k == "L" else ~path]).all() for k in ("L", "Dinv", "y"))
        held(P, vals, b, lam, d, f"-I in a {where} column, lambda {lam:g}:", exempt=path)
    assert G.debug_factor(0, 1e-2, vals, b)["fail"] != 0


def test_a_zero_pivot_and_a_nan_set_the_fail_word():
    c = case("clique_12_tail20")
    G, P = c["G"], c["P"]
    clean = G.debug_factor(1, 0.0, c["vals"], c["b"], selinv=True)
    assert clean["fail"] == 0
    vals = c["vals"].copy()
    vals[c["rp"][P["perm"][0]]] = 0.0  # column 0: a leaf of the tree, no products: R = 0 exactly
    assert P["np"][0] == 0
    d = G.debug_factor(1, 0.0, vals, c["b"], selinv=True)
    must_fail, _, bad, _ = F.fail_expected(P, d, 0.0)
    assert d["fail"] != 0 and must_fail and bad[0]
    vals = c["vals"].copy()
    vals[c["rp"][P["perm"][3]], 2, 2] = np.nan
    for ctx in (0, 1):
        assert G.debug_factor(ctx, 0.0, vals, c["b"])["fail"] != 0
    again = G.debug_factor(1, 0.0, c["vals"], c["b"], selinv=True)
    for k in BITS + ("Z",):
        assert np.array_equal(again[k], clean[k]), k
    assert again["fail"] == 0 and again["singular"] == clean["singular"]


def test_the_pivot_threshold_of_the_selected_inversion():
    """k_selinv_pivots: a pivot below 1e-13 max |H_dd|.  diag(1, ..., 1, p): L(6,6)^2 = p to a rounding, max |H_dd| = 1
    from the injected blocks; 2^-43 = 1.137e-13 is above, 2^-44 = 5.7e-14 below (a margin of 13 % and 43 %)."""
    c = case("one_free")
    G = c["G"]
    for p, flag in ((2.0 ** -43, 0), (2.0 ** -44, 1)):
        vals = np.diag([1.0] * 6 + [p])[None]
        d = G.debug_factor(1, 0.0, vals, c["b"], selinv=True)
        assert d["fail"] == 0 and d["singular"] == flag and abs(d["L"][0, 6, 6] ** 2 - p) <= 4 * R.U * p


# ------------------------------------------------------------------------------------------------ nothing moves
def _run(G, iters):
    n = G.optimize(iters)
    kt = G.kernel_times()
    st = [(t.chi2_before, t.chi2_after, t.lambda_, t.rho, t.trials, t.pcg_iters, t.pcg_rel_res) for t in G.stats()]
    counts = {k: getattr(kt, k) for k, _ in L.KernelTimes._fields_ if k.startswith("n_")}
    return n, G.get_vertices(), st, counts


@pytest.mark.parametrize("solver", [1, 0], ids=["lm_direct", "lm_pcg"])
def test_optimize_after_the_read_outs_is_bit_identical(solver):
    c = case("chain_40")
    make = lambda: C.graph_of(c["g"], linear_solver=solver, fd_delta=1e-6)
    ctxs = (0, 1) if solver == 1 else (1,)
    counts = lambda G: {k: getattr(G.kernel_times(), k) for k, _ in L.KernelTimes._fields_ if k.startswith("n_")}
    same = lambda got, want: (got[0] == want[0] and np.array_equal(got[1], want[1]) and got[2] == want[2]
                              and got[3] == want[3])
    a = make()
    a.initialize()
    ref = _run(a, 3)
    xa = a.solve(0.3)[0]
    a.solve(0.3)
    ref2 = _run(a, 2)
    b = make()
    b.initialize()
    for ctx in ctxs:  # before the first call: injected values only (there is no linearisation yet)
        b.debug_factor(ctx, 0.5, c["vals"], c["b"], selinv=ctx == 1)
    assert same(_run(b, 3), ref)
    x0 = b.solve(0.3)[0]
    assert np.array_equal(x0, xa)
    kt0 = counts(b)
    for ctx in ctxs:  # between two calls: without injection, with it, with values alone
        b.debug_factor(ctx, 0.5, selinv=ctx == 1)
        b.debug_factor(ctx, 0.5, c["vals"], c["b"], selinv=ctx == 1)
        b.debug_factor(ctx, 0.0, c["vals"], None, solve=False)
    assert counts(b) == kt0
    assert np.array_equal(b.solve(0.3)[0], x0)  # the context starts from the real system's blocks again
    assert same(_run(b, 2), ref2)


# ------------------------------------------------------------------------------------------------ refusals
def test_the_read_out_refuses_what_it_cannot_do():
    lib = L.load()
    g = C.CASES["two_free"]()
    dp = ctypes.POINTER(ctypes.c_double)
    p = lambda a: a.ctypes.data_as(dp)
    nb_, nL_, nz_ = ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int64()
    o = [np.zeros(3 * 49) for _ in range(8)]
    fw, sg = ctypes.c_int32(), ctypes.c_int32()

    def call(G, ctx, lam=0.0, solve=1, selinv=0, outs=None):
        outs = [p(a) for a in o[:7]] if outs is None else outs
        return lib.sim3opt_debug_factor(G._g, ctx, lam, None, None, solve, selinv, *outs, ctypes.byref(fw), p(o[7]),
                                        ctypes.byref(sg), None, None)

    G = C.graph_of(g, linear_solver=1)
    dims = lambda G, ctx: lib.sim3opt_debug_factor_dims(G._g, ctx, ctypes.byref(nb_), ctypes.byref(nL_), ctypes.byref(nz_))
    assert dims(G, 0) == L.ERR_STATE and call(G, 0) == L.ERR_STATE  # not initialised
    assert b"initialize" in lib.sim3opt_last_error(G._g)
    G.initialize()
    assert dims(G, 0) == L.OK and (nb_.value, nL_.value, nz_.value) == (2, 3, 4)
    assert lib.sim3opt_debug_factor_dims(G._g, 0, None, None, None) == L.ERR_ARG
    assert call(G, 0) == L.ERR_STATE and b"linearize" in lib.sim3opt_last_error(G._g)  # nothing to factor yet
    G.linearize()
    assert call(G, 0) == L.OK and fw.value == 0
    assert call(G, 0, outs=[None] * 7) == L.ERR_ARG and b"null" in lib.sim3opt_last_error(G._g)
    assert call(G, 0, outs=[p(a) for a in o[:5]] + [None, None]) == L.ERR_ARG  # with_solve needs xp and x
    assert call(G, 0, solve=0, outs=[p(a) for a in o[:5]] + [None, None]) == L.OK
    assert call(G, 0, selinv=1) == L.ERR_ARG and b"context 1" in lib.sim3opt_last_error(G._g)
    assert call(G, 2) == L.ERR_ARG and call(G, 0, lam=-1.0) == L.ERR_ARG and call(G, 0, lam=float("nan")) == L.ERR_ARG
    assert call(G, 1, selinv=1) == L.OK and sg.value == 0
    Gp = C.graph_of(g, linear_solver=0)
    Gp.initialize()
    Gp.linearize()
    assert call(Gp, 0) == L.ERR_STATE and b"PCG" in lib.sim3opt_last_error(Gp._g)  # context 0 on a PCG graph
    assert dims(Gp, 0) == L.ERR_STATE and dims(Gp, 1) == L.OK and call(Gp, 1, selinv=1) == L.OK
    assert lib.sim3opt_version() == 130  # diagnostics are not part of the versioned interface


def test_the_read_out_refuses_a_partitioned_graph():
    g = LC.graph("tail_1")
    errs = []
    tg = DH.ThreadGroup(2)

    def body(rank):
        G = L.Graph(device=0, fd_delta=1e-6)
        G.add_vertices(g["states"], g["fixed"])
        G.add_edges(g["v0"], g["v1"], g["meas"])
        tg.attach(G, rank)
        G.initialize()
        G.linearize()
        try:
            G.debug_factor(1, 1.0)
            errs.append("accepted")
        except L.Sim3OptError as e:
            errs.append((e.code, "partitioned" in str(e)))

    tg.run(body)
    assert errs == [(L.ERR_STATE, True)] * 2
