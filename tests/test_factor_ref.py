"""CPU side of the operator tests of the exact block Cholesky (tests/test_gpu_factor_operators.py): the restatement
tests/factor_ref.py is pinned to dense numpy, the path every case of tests/factor_cases.py takes through the kernels
is asserted from the host plan, and every seeded defect of the restatement must exceed its local bound 1000-fold.
No GPU needed."""
import functools

import numpy as np
import pytest
import scipy.linalg as sl

import cov_ref as CR
import factor_cases as C
import factor_ref as F
import lm_ref as R


@functools.lru_cache(maxsize=None)
def case(name):
    g = C.CASES[name]()
    G = C.graph_of(g)
    P = F.plan_of(G)
    rp, ci = G.system_pattern()
    vals, b = C.injected(g, rp, ci)
    return dict(g=g, P=P, rp=rp, ci=ci, vals=vals, b=b)


@functools.lru_cache(maxsize=None)
def restated(name, lam):
    c = case(name)
    return F.restate(c["P"], c["vals"], c["b"], lam)


# ------------------------------------------------------------------------------------------------ paths
# What each case is for, measured on the host plan with the current planner (factor_cases.paths).  A planner change
# that moves a case off its path fails here; then choose a new case for the path, do not delete the row.
PATHS = {
    "one_free": dict(nb=1, nL=1, npairs=0, ngroups=1),
    "two_free": dict(nb=2, nL=3, npairs=1, ngroups=1),
    "parallel": dict(nb=3, max_sources=3, ngroups=1),
    # one diagonal block with n products: 112 the largest round that all wavefronts stage together, 113 the first that
    # its wavefront stages alone, 14 at a time; 130 = nine full pieces and a tail of four
    "star_16": dict(max_products=16, max_coop_round=16, wide_rounds=0, ngroups=5, height=2),
    "star_112": dict(max_products=112, max_coop_round=112, wide_rounds=0, ngroups=17, height=2),
    "star_113": dict(max_products=113, max_round=113, wide_rounds=1, max_pieces=9, ngroups=18, height=2),
    "star_130": dict(max_products=130, max_round=130, wide_rounds=1, max_pieces=10, ngroups=18, height=2),
    "clique_24": dict(wide_rounds=11, blocks_spanning_pieces=56, pairs_cut=20, no_source_blocks=0, max_offdiag=23),
    # a column of 65 off-diagonal blocks: ldl_back's second pass of 64; 65 = 8 * 8 + 1 for SEL_BATCH / COV_BATCH
    "clique_66": dict(max_offdiag=65, max_cell_blocks=8, max_rounds_per_level=2, max_round=1089, height=66,
                      npairs=47905, nprod=95810, max_root_path=66),
    "clique_12_tail20": dict(ngroups=7, no_source_blocks=19, max_root_path=14, height=14),
    "chain_40": dict(ngroups=10, no_source_blocks=44, max_root_path=9),
    "two_components": dict(roots=2, ngroups=6),
    "kitti_one_loop": dict(nb=770, max_coop_round=111, wide_rounds=0, max_round=111),
    "kitti_all_loops": dict(nb=770, max_round=191, wide_rounds=2, blocks_spanning_pieces=13, pairs_cut=7, max_root_path=21),
}


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_every_case_takes_its_path(name):
    got = C.paths(case(name)["P"])
    assert {k: got[k] for k in PATHS[name]} == PATHS[name]
    if name.startswith("star_"):  # the hub's block is the one with all the products, and it is a diagonal block
        P = case(name)["P"]
        s = int(np.argmax(P["np"]))
        assert P["isdiag"][s] and P["np"][s] == P["nb"] - 1 and (np.delete(P["np"], s) == 0).all()
    if name in ("clique_12_tail20", "chain_40"):  # bottom groups AND a top group, fill in the top group
        P = case(name)["P"]
        top0 = P["colptr"][P["lcolp"][P["gptr"][P["ngroups"] - 1]]]
        assert 0 < top0 < P["nL"] and (P["nsrc"][top0:] == 0).any()


def test_common_suffixes_and_requests_exist():
    """what test_gpu_factor_operators.py asks of the elimination trees: pairs outside the pattern whose root paths share
    1, 8, 9 and 17 blocks on KITTI-00, and five leaves on every graph of the covariance test"""
    T = CR.Tree(case("kitti_all_loops")["P"])
    sp = C.suffix_pairs(T)
    assert sorted(sp) == [1, 8, 9, 17]
    for n, (a, b) in sp.items():
        assert (max(a, b), min(a, b)) not in T.stored and T.depth[T.lca(a, b)] + 1 == n
    for name in ("clique_12_tail20", "chain_40", "two_components", "kitti_all_loops"):
        assert len(C.leaves_of(CR.Tree(case(name)["P"]))) >= 5


# ------------------------------------------------------------------------------------------------ pins
def pin_lambdas(name):
    return (0.0,) if name.startswith("kitti") else C.LAMBDAS  # (a dense 5390 x 5390 Cholesky takes a second)


def extreme_eigenvalues(S, Lc):
    """(smallest, largest) eigenvalue of the SPD matrix S = Lc Lc^T; beyond a thousand rows to a few per cent by power
    iterations, the smallest through triangular solves (an eigendecomposition of KITTI-00's 5390 rows takes ten
    seconds), with a margin of 10 % either way"""
    if S.shape[0] <= 1000:
        ev = np.linalg.eigvalsh(S)
        return ev[0], ev[-1]
    from scipy.linalg import solve_triangular as st
    rng = np.random.default_rng(0)
    v, w = rng.standard_normal(S.shape[0]), rng.standard_normal(S.shape[0])
    for _ in range(40):
        v = S @ v
        v /= np.linalg.norm(v)
        w = st(Lc, st(Lc, w, lower=True), lower=True, trans=1)
        w /= np.linalg.norm(w)
    return 0.9 * (w @ S @ w), 1.1 * (v @ S @ v)


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_restatement_matches_dense_numpy(name):
    """float64 restatement against dense Cholesky / solve / inverse of the symmetrically equilibrated matrix
    S = D^-1/2 (M + lambda I) D^-1/2, D = its diagonal: the error of a Cholesky solve is governed by cond(S) whatever
    the scaling of the rows (Higham, Theorem 10.6), so the tolerance is 64 n cond(S) u on the equilibrated
    quantities, relative to their largest entry."""
    c = case(name)
    P = c["P"]
    nb = P["nb"]
    p7 = (7 * P["perm"][:, None] + np.arange(7)).ravel()
    for lam in pin_lambdas(name):
        d = restated(name, lam)
        assert d["fail"] == 0  # every pivot of the float64 restatement is positive
        M = F.dense_of(c["rp"], c["ci"], c["vals"], lam)[np.ix_(p7, p7)]
        ds = np.sqrt(np.diag(M))
        S = M / np.outer(ds, ds)
        Lc = np.linalg.cholesky(S)
        lo, hi = extreme_eigenvalues(S, Lc)
        assert lo > 0
        tol = 64 * 7 * nb * (hi / lo) * R.U
        dsb = ds.reshape(nb, 7)
        i, j = P["lrow"], P["lcol"]
        Lref = Lc.reshape(nb, 7, nb, 7).transpose(0, 2, 1, 3)[i, j]
        assert np.abs(d["L"] / dsb[i][:, :, None] - Lref).max() < tol
        mask = np.ones((nb, nb), bool)
        mask[i, j] = False  # nothing of the dense factor lies outside the plan's pattern
        assert np.abs(Lc.reshape(nb, 7, nb, 7).transpose(0, 2, 1, 3)[mask]).max(initial=0) < tol
        bt = (c["b"][P["perm"]] / dsb).ravel()
        yref = sl.solve_triangular(Lc, bt, lower=True)
        assert np.abs(d["y"].ravel() - yref).max() < tol * np.abs(yref).max()
        xref = sl.cho_solve((Lc, True), bt)
        assert np.abs((d["xp"] * dsb).ravel() - xref).max() < tol * np.abs(xref).max()
        assert np.array_equal(d["x"][P["perm"]], d["xp"])
        # the inverse: every block column, or on KITTI-00 a sample of them
        cols = np.arange(nb) if nb <= 150 else np.unique(np.r_[0, nb - 1, np.random.default_rng(1).integers(0, nb, 14)])
        E = np.zeros((7 * nb, 7 * len(cols)))
        E[(7 * cols[:, None] + np.arange(7)).ravel(), np.arange(7 * len(cols))] = 1
        Zc = sl.cho_solve((Lc, True), E).reshape(nb, 7, len(cols), 7)
        at = {int(cj): q for q, cj in enumerate(cols)}
        sel = np.array([s for s in range(P["nL"]) if int(j[s]) in at])
        Zb = np.stack([Zc[i[s], :, at[int(j[s])], :] for s in sel])
        Zs = d["Z"][sel] * dsb[i[sel]][:, :, None] * dsb[j[sel]][:, None, :]
        assert np.abs(Zs - Zb).max() < tol * np.abs(Zc).max()
        DL = d["Dinv"] @ d["L"][P["colptr"][:-1]]
        assert np.abs(DL - np.eye(7)).max() < tol


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_restatement_passes_its_own_local_checks(name):
    """the float64 restatement is an implementation like the device's: every bound holds, no pivot near its bound"""
    c = case(name)
    for lam in C.LAMBDAS:
        d = restated(name, lam)
        r = F.check(c["P"], c["vals"], c["b"], lam, d)
        assert max(v[0] for v in r.values()) <= 1.0, (lam, r)
        must_fail, must_pass, _, between = F.fail_expected(c["P"], d, lam)
        assert between == 0 and must_pass and not must_fail and d["fail"] == 0


def test_long_double_restatement_is_the_float64_one_to_rounding():
    c = case("clique_12_tail20")
    d64, dld = restated("clique_12_tail20", 1e-2), F.restate(c["P"], c["vals"], c["b"], 1e-2, dt=F.LD)
    x = np.abs(np.asarray(dld["xp"], dtype=np.float64))
    assert np.abs(d64["xp"] - dld["xp"]).max() < 1e-9 * x.max() and dld["L"].dtype == F.LD


def test_restatement_noise_of_blocks_outside_the_pattern():
    """The share of requested pairs whose float64 root-path recursion is further than lm_ref.ILL from long double (set
    apart by the device test) is at most 10 % per case -- from the restatement alone."""
    for name in ("clique_12_tail20", "chain_40", "two_components", "kitti_all_loops"):
        P = case(name)["P"]
        d = restated(name, 1e-2)
        T = CR.Tree(P)
        cols = C.leaves_of(T)[:5]
        W64, Wld = F.root_paths(T, d["L"], d["Dinv"], cols, np.float64), F.root_paths(T, d["L"], d["Dinv"], cols, F.LD)
        pr = [(a, b) for a in cols for b in cols if a != b and T.lca(a, b) >= 0]
        z64 = np.stack([F.pair_block(T, W64, a, b, np.float64)[0] for a, b in pr])
        zld = np.stack([F.pair_block(T, Wld, a, b, F.LD)[0] for a, b in pr])
        ill = R.edge_scaled_err(z64, zld) > R.ILL
        assert ill.sum() <= 0.1 * len(pr), (name, int(ill.sum()), len(pr))


# ------------------------------------------------------------------------------------------------ seeded defects
def multiple(c, lam, d, first_level=False):
    """The largest error / bound of a (defective) restatement.  Nothing is forgiven: an entry that must be exact and is
    not, or a NaN, fails the test with check()'s own message.  first_level: the columns of the first level alone (a
    defect after which later pivots fail turns everything behind them into garbage; the first level still measures)."""
    P = c["P"]
    if not first_level:
        return max(v[0] for v in F.check(P, c["vals"], c["b"], lam, d).values())
    later = np.arange(P["nb"]) >= P["lcolp"][1]
    with np.errstate(all="ignore"):
        r = F.check(P, c["vals"], c["b"], lam, d, with_solve=False, with_selinv=False, exempt=later)
    return max(v[0] for v in r.values())


def _products(name):
    """a sample of products to drop: the first and the last of the block with the most, and six at random"""
    P = case(name)["P"]
    s = int(np.argmax(P["np"]))
    rng = np.random.default_rng(4)
    return [int(P["pairptr"][s]), int(P["pairptr"][s + 1] - 1)] + [int(k) for k in rng.integers(0, P["npairs"], 6)]


DEFECTS = [  # (defect, case, lambda, products to drop)
    ("product_dropped", "clique_24", 1e-2, "sample"),
    ("product_dropped", "kitti_all_loops", 0.0, "sample"),
    ("last_piece_dropped", "star_130", 1e-2, "last_piece"),
    ("pa_pb_swapped", "clique_24", 1e-2, None),
    ("lambda_everywhere", "clique_12_tail20", 1e-2, None),
    ("lambda_omitted", "clique_12_tail20", 1e-2, None),
    ("second_source_dropped", "parallel", 0.0, None),
    ("dinv_untransposed", "chain_40", 1e-2, None),
    ("y_without_products", "chain_40", 1e-2, None),
    ("back_65th_dropped", "clique_66", 1e-2, None),
    ("z_untransposed", "clique_24", 1e-2, None),
    ("z_9th_dropped", "clique_24", 1e-2, None),
    ("z0_omitted", "two_free", 1e-2, None),
]
FLOOR = 1e3  # the floor DESIGN.md section 5c' uses


@pytest.mark.parametrize("mut,name,lam,arg", DEFECTS, ids=[f"{d[0]}-{d[1]}" for d in DEFECTS])
def test_seeded_defects_exceed_their_bounds(mut, name, lam, arg):
    c = case(name)
    P = c["P"]
    if arg == "sample":
        args = [[k] for k in _products(name)]
    elif arg == "last_piece":  # products 127 .. 130 of the hub's block: the tail of four behind nine pieces of 14
        s = int(np.argmax(P["np"]))
        args = [list(range(P["pairptr"][s] + 126, P["pairptr"][s] + 130))]
    else:
        args = [None]
    worst = np.inf
    for a in args:
        with np.errstate(all="ignore"):
            d = F.restate(P, c["vals"], c["b"], lam, mut=mut, mut_arg=a)
        worst = min(worst, multiple(c, lam, d, first_level=mut == "dinv_untransposed"))
    print(f"{mut} on {name}: smallest error / bound {worst:.3g}")
    assert worst >= FLOOR


def test_mirroring_the_diagonal_of_z_the_other_way_moves_nothing():
    """The thirteenth defect provably stays within the bounds: the upper triangle of (Z0 - acc) Dinv is as good a
    rounding of the symmetric block as the lower one, both mirrors are exactly symmetric, and the bound of entry (r, c)
    is checked on the lower triangle only.  What the test can hold is the symmetry, and that every bound still holds
    on the triangle it reads."""
    c = case("clique_24")
    d = F.restate(c["P"], c["vals"], c["b"], 1e-2, mut="z_mirror_wrong")
    ok = restated("clique_24", 1e-2)
    dg = c["P"]["colptr"][:-1]
    assert not np.array_equal(d["Z"][dg], ok["Z"][dg]) and np.array_equal(d["Z"][dg], d["Z"][dg].transpose(0, 2, 1))
    assert np.abs(d["Z"][dg] - ok["Z"][dg]).max() <= 1e-12 * np.abs(ok["Z"][dg]).max()


@pytest.mark.parametrize("where", ["bottom", "top"])
def test_a_failing_column_spoils_its_root_path_only(where):
    """the device test's fail case on the restatement: -I for a source diagonal block; the fail word is set, no column
    off the root path fails, and L, Dinv, y of every column off the path hold their bounds"""
    c = case("clique_12_tail20")
    P = c["P"]
    T = CR.Tree(P)
    j = 0 if where == "bottom" else int(P["lcolp"][P["gptr"][P["ngroups"] - 1]])
    vals = c["vals"].copy()
    vals[c["rp"][P["perm"][j]]] = -np.eye(7)
    path = np.zeros(P["nb"], bool)
    path[T.path(j)] = True
    with np.errstate(all="ignore"):
        d = F.restate(P, vals, c["b"], 1e-2)
        must_fail, _, bad, _ = F.fail_expected(P, d, 1e-2)
        r = F.check(P, vals, c["b"], 1e-2, d, with_solve=False, with_selinv=False, exempt=path)
    assert d["fail"] == 1 and must_fail and bad[j] and not (bad & ~path).any()
    assert max(v[0] for v in r.values()) <= 1.0


def test_a_zero_block_at_a_leaf_is_an_exactly_zero_pivot():
    c = case("clique_12_tail20")
    P = c["P"]
    vals = c["vals"].copy()
    vals[c["rp"][P["perm"][0]]] = 0.0
    assert P["np"][0] == 0
    with np.errstate(all="ignore"):
        d = F.restate(P, vals, c["b"], 0.0)
        must_fail, _, bad, _ = F.fail_expected(P, d, 0.0)
    assert d["fail"] == 1 and must_fail and bad[0]
