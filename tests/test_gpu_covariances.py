"""GPU tests (-m gpu) of sim3opt_covariances -- blocks of (H + lambda I)^-1 for ANY pair of free vertices: on the
factor's pattern the selected inversion's, outside it sums over the common ancestors in the elimination tree
(cov_kernels.hpp) -- and of sim3opt_gate_edges, the chi-square gate of candidate edges built on them
(gate_kernels.hpp).  The covariances are checked against a dense inverse of the system the library itself linearised,
to the bound of test_gpu_marginals.py; the gate against a numpy restatement from that inverse and the CPU oracle.

The gate's Jacobian term.  The restatement takes J from the oracle's central differences at delta = 1e-6 with the exact
small-angle coefficient; the library's closed form is a second reference (lib.edge_jacobian_host, host code).  On the
candidates of test_gate_matches_numpy_restatement the two differ by 2.9e-6 of ||J||_2 at most (measured on the host;
neither is under test): that much on the candidates perturbed by 1e-3, whose residual rotation lies inside the band
where log takes the theta = 0 coefficients of W, and 2.5e-9 / 3.1e-9 on those perturbed by 0 / 0.3.  The test holds
the two references to JAC_REFS_DISAGREE = 3.0e-6 and allows JAC_MARGIN = 10 times that on the device's J, so that
last-bit differences of exp / log between device and host cannot trip it."""
import numpy as np
import pytest

from oracle import oracle as O
from sim3opt_amd import lib as L, synth
import cov_ref as R
import kitti_graph as K

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
JAC_REFS_DISAGREE = 3.0e-6
JAC_MARGIN = 10.0


def mk(g, ids=None, info=None, kernel=0, kdelta=0.0, fixed=None, **opts):
    G = L.Graph(**opts)
    ids = np.arange(g["states"].shape[0], dtype=np.int32) if ids is None else ids
    G.add_vertices(g["states"], g["fixed"] if fixed is None else fixed, ids)
    if info is None:
        G.add_edges(ids[g["v0"]], ids[g["v1"]], g["meas"])
    else:
        G.add_edges(ids[g["v0"]], ids[g["v1"]], g["meas"], info=info, kernel=kernel, kernel_delta=kdelta)
    G.initialize()
    return G, ids


def huber_chain():
    """test_gpu_marginals.py's chain: information matrices, Huber, parallel edges, sparse ids, two fixed vertices"""
    g = synth.chain_loop(300, 340)
    rng = np.random.default_rng(5)
    dup = rng.choice(g["v0"].shape[0], 25, replace=False)
    g = dict(g)
    g["v0"] = np.concatenate([g["v0"], g["v0"][dup]]).astype(np.int32)
    g["v1"] = np.concatenate([g["v1"], g["v1"][dup]]).astype(np.int32)
    g["meas"] = np.concatenate([g["meas"], g["meas"][dup]])
    g["fixed"] = g["fixed"].copy()
    g["fixed"][150] = 1
    M = rng.standard_normal((g["v0"].shape[0], 7, 7)) * 0.3
    info = np.einsum("kij,klj->kil", M, M) + np.eye(7)
    ids = (np.arange(300) * 7 + 3).astype(np.int32)
    return g, dict(ids=ids, info=info, kernel=L.KERNEL_HUBER, kdelta=0.3)


# name -> (graph and the arguments of mk, options, every ordered pair instead of a sample)
CASES = {
    "chain_40": (lambda: (R.GRAPHS["chain_40"](), {}), {}, True),
    "two_chains": (lambda: (R.two_chains(), {}), {}, True),
    "manhattan_300": (lambda: (R.GRAPHS["manhattan_300"](), {}), dict(linear_solver=1), False),
    "kitti_all_loops": (lambda: (K.build_direct_graph(False), {}), {}, False),
    "huber_chain_pcg": (huber_chain, dict(fd_delta=1e-6, linear_solver=0), False),
}


def free_ids(g, ids):
    """ids of the free vertices by block row (one rank: insertion order, g2o's hessianIndex)"""
    return ids[np.flatnonzero(np.asarray(g["fixed"]) == 0)]


def request(T, everything):
    """block rows (ra, rb) of the requested pairs: every ordered pair, or 2000 seeded ones plus one full block column
    (every free vertex against the deepest vertex of the tree)"""
    if everything:
        ra, rb = (x.ravel() for x in np.meshgrid(np.arange(T.nb), np.arange(T.nb)))
        return ra, rb
    ra, rb = R.seeded_pairs(T, 2000, 17)
    row_of = np.empty(T.nb, dtype=np.int64)
    row_of[T.pos] = np.arange(T.nb)
    deep = row_of[int(np.argmax(T.depth))]
    return np.concatenate([ra, np.arange(T.nb)]), np.concatenate([rb, np.full(T.nb, deep)])


def blocks(Z, ra, rb):
    return np.stack([Z[7 * a:7 * a + 7, 7 * b:7 * b + 7] for a, b in zip(ra, rb)])


def pairs_of(fid, ra, rb):
    return np.stack([fid[ra], fid[rb]], axis=1)


@pytest.mark.parametrize("name", sorted(CASES))
def test_covariances_match_dense_inverse(name):
    make, opts, everything = CASES[name]
    g, extra = make()
    G, ids = mk(g, fix_small_angle_b=1, **extra, **opts)
    assert G.linear_solver_in_use() == (0 if name == "huber_chain_pcg" else 1)
    fid = free_ids(g, ids)
    T = R.Tree(G.marginal_plan())
    ra, rb = request(T, everything)
    cls = [T.classes(a, b) for a, b in zip(ra, rb)]
    seen = set().union(*cls)
    assert set(R.CLASSES) <= seen, set(R.CLASSES) - seen
    on = np.array(["on_pattern" in c for c in cls])
    cross = np.array(["off_disconnected" in c for c in cls])
    assert cross.any() == (name == "two_chains")
    pairs = pairs_of(fid, ra, rb)
    G.linearize()
    H, _ = G.dense_system()
    n = H.shape[0]
    assert n == 7 * T.nb
    ev = np.linalg.eigvalsh(H)  # (the spectrum of H + lam I is that of H, shifted)
    for lam in (0.0, 1e-2, 1.0):
        cond = (ev[-1] + lam) / (ev[0] + lam)
        Zr = np.linalg.inv(H + lam * np.eye(n))
        ref = blocks(Zr, ra, rb)
        Z = G.covariances(pairs, lam)
        st = G.covariance_stats()
        assert Z.shape == ref.shape
        scale = np.abs(ref).max()
        tol = max(1e-10, 1e3 * n * EPS * cond) * scale
        err = np.abs(Z - ref).max()
        err_off = np.abs(Z[~on] - ref[~on]).max()
        print(f"{name} lambda={lam:g}: cond2 {cond:.3e}, {on.sum()} pairs on / {(~on).sum()} off the pattern, "
              f"{st['chunks']} chunk(s), {st['paths']} paths, max|err| / max|ref| {err / scale:.2e} "
              f"(off the pattern {err_off / scale:.2e}; bound {tol / scale:.2e})")
        assert err <= tol, (lam, cond, err / scale)
        assert st["chunks"] >= 1 and st["selinv"] == 1 and st["on_pattern_pairs"] == on.sum()
        assert np.all(Z[cross] == 0.0)  # no common ancestor: exactly zero
        if lam == 1e-2:
            # pairs on the pattern: the bits of sim3opt_marginals; reversed pairs: the exact transpose
            assert np.array_equal(Z[on], G.marginals(pairs[on], lam))
            assert np.array_equal(G.covariances(pairs[:, ::-1], lam), Z.transpose(0, 2, 1))
    G.close()


def test_covariance_bits_do_not_depend_on_the_request():
    """shuffled, with duplicates, split over two calls, asked twice: the same bits per pair; a request on the pattern
    launches none of the new kernels, one off it no selected inversion"""
    for name in ("chain_40", "kitti_all_loops"):
        make, opts, everything = CASES[name]
        g, extra = make()
        G, ids = mk(g, fix_small_angle_b=1, **extra, **opts)
        fid = free_ids(g, ids)
        T = R.Tree(G.marginal_plan())
        ra, rb = request(T, everything)
        if not everything:
            ra, rb = ra[:600], rb[:600]
        pairs = pairs_of(fid, ra, rb)
        on = np.array(["on_pattern" in T.classes(a, b) for a, b in zip(ra, rb)])
        lam = 1e-2
        Z = G.covariances(pairs, lam)
        assert np.array_equal(G.covariances(pairs, lam), Z)
        rng = np.random.default_rng(23)
        order = rng.permutation(pairs.shape[0])
        assert np.array_equal(G.covariances(pairs[order], lam), Z[order])
        dup = np.concatenate([order[:50], np.arange(pairs.shape[0]), order[:50]])
        assert np.array_equal(G.covariances(pairs[dup], lam), Z[dup])
        h = pairs.shape[0] // 3
        assert np.array_equal(np.concatenate([G.covariances(pairs[:h], lam), G.covariances(pairs[h:], lam)]), Z)
        assert np.array_equal(G.covariances(pairs[on], lam), Z[on])
        st = G.covariance_stats()
        assert (st["chunks"], st["paths"], st["off_pattern_pairs"], st["selinv"]) == (0, 0, 0, 1)
        assert np.array_equal(G.covariances(pairs[~on], lam), Z[~on])
        st = G.covariance_stats()
        assert st["chunks"] >= 1 and st["selinv"] == 0 and st["on_pattern_pairs"] == 0
        assert st["off_pattern_pairs"] == len({(min(a, b), max(a, b)) for a, b in zip(ra[~on], rb[~on])})
        G.close()


def test_covariances_do_not_depend_on_the_schedule(monkeypatch):
    """The four schedules of test_marginals_do_not_depend_on_the_schedule renumber the columns; a root path and the
    common suffix of two are the same vertices in the same order under each: the same bits."""
    g = K.build_direct_graph(False)
    ref, groups = None, set()
    for subtree, wg in (("16", "256"), ("48", "512"), ("128", "384"), ("8", "64")):
        monkeypatch.setenv("SIM3OPT_DIRECT_SUBTREE", subtree)
        monkeypatch.setenv("SIM3OPT_DIRECT_WG_SUB", wg)
        G, ids = mk(g)
        if ref is None:  # the request is fixed under the first schedule, in vertex ids
            ra, rb = request(R.Tree(G.marginal_plan()), False)
            pairs = pairs_of(free_ids(g, ids), ra[:800], rb[:800])
        groups.add(G.marginal_plan()["ngroups"])
        cur = G.covariances(pairs, 1e-2)
        G.close()
        if ref is None:
            ref = cur
        assert np.array_equal(cur, ref)
    assert len(groups) > 1


def test_covariances_in_chunks(monkeypatch):
    """A workspace too small for the request: at least three chunks on the 40-chain's all-pairs request, the bits of
    the run in one chunk."""
    g = R.GRAPHS["chain_40"]()
    G, ids = mk(g, fix_small_angle_b=1)
    T = R.Tree(G.marginal_plan())
    ra, rb = request(T, True)
    pairs = pairs_of(free_ids(g, ids), ra, rb)
    Z = G.covariances(pairs, 1e-2)
    st = G.covariance_stats()
    total = int((T.depth + 1).sum())  # blocks of 392 bytes when every vertex is in one chunk
    assert st["chunks"] == 1 and st["paths"] == T.nb and st["workspace_bytes"] == 392 * total
    assert G.options().cov_workspace_mb == 256.0
    G.close()
    limit = total // 4
    assert limit >= 2 * (int(T.depth.max()) + 1)  # one pair always fits
    monkeypatch.setenv("SIM3OPT_COV_WORKSPACE_MB", repr(limit * 392 / 2.0**20))
    G, _ = mk(g, fix_small_angle_b=1)
    Zc = G.covariances(pairs, 1e-2)
    st = G.covariance_stats()
    print(f"chain_40: {total} blocks in one chunk; limit {limit}: {st['chunks']} chunks, {st['paths']} paths, "
          f"{st['workspace_bytes']} bytes")
    assert st["chunks"] >= 3 and st["workspace_bytes"] <= limit * 392 and st["paths"] > T.nb
    assert np.array_equal(Zc, Z)
    # too small for a single pair: refused, and the field itself has a floor of 1
    monkeypatch.setenv("SIM3OPT_COV_WORKSPACE_MB", repr(392 / 2.0**20))
    G2, _ = mk(g, fix_small_angle_b=1)
    off = np.array(["on_pattern" not in T.classes(a, b) for a, b in zip(ra, rb)])
    with pytest.raises(L.Sim3OptError) as e:
        G2.covariances(pairs[off][:1], 1e-2)
    assert e.value.code == L.ERR_STATE
    with pytest.raises(L.Sim3OptError):
        G2.set_options(cov_workspace_mb=0.5)
    G2.close()
    G.close()


def test_covariance_error_paths():
    g = synth.chain_loop(200, 230)
    # no fixed vertex: H is singular (the gauge) -- an error at lambda = 0, the next call at lambda = 1 finite
    for opts in (dict(), dict(linear_solver=0)):
        G, ids = mk(g, fixed=np.zeros_like(g["fixed"]), fix_small_angle_b=1, **opts)
        far = [(int(ids[3]), int(ids[120])), (int(ids[7]), int(ids[7]))]
        with pytest.raises(L.Sim3OptError) as e:
            G.covariances(far, 0.0)
        assert e.value.code == L.ERR_STATE
        with pytest.raises(L.Sim3OptError) as e:  # ... also when no pair needs the selected inversion
            G.covariances(far[:1], 0.0)
        assert e.value.code == L.ERR_STATE
        assert np.isfinite(G.covariances(far, 1.0)).all()
        G.close()
    G, ids = mk(g, fix_small_angle_b=1)
    T = R.Tree(G.marginal_plan())
    fid = free_ids(g, ids)
    off = next((int(fid[a]), int(fid[b])) for a in range(T.nb) for b in range(a) if "on_pattern" not in T.classes(a, b))
    fixed_id = int(ids[np.flatnonzero(g["fixed"])[0]])
    for bad in ([(fixed_id, 5)], [(5, fixed_id)], [(5, 100000)], [(-7, 5)]):
        with pytest.raises(L.Sim3OptError) as e:
            G.covariances(bad)
        assert e.value.code == L.ERR_ARG
    assert G.covariances(np.zeros((0, 2), dtype=np.int32)).shape == (0, 7, 7)  # n = 0 is OK
    with pytest.raises(L.Sim3OptError) as e:
        G.covariances([(5, 120)], -1.0)
    assert e.value.code == L.ERR_ARG
    # sim3opt_marginals still refuses the pair sim3opt_covariances answers
    with pytest.raises(L.Sim3OptError) as e:
        G.marginals([off])
    assert e.value.code == L.ERR_ARG
    assert np.isfinite(G.covariances([off])).all()
    # the gate: identical endpoints, an unknown id, a bad measurement, an information matrix that is not SPD --
    # SIM3OPT_ERR_ARG and the outputs untouched
    meas = np.tile(np.array([0, 0, 0, 1, 0, 0, 0, 1.0]), (2, 1))
    bad_info = np.stack([np.eye(7), np.diag([1, 1, 1, -1.0, 1, 1, 1])])
    nan_meas = meas.copy()
    nan_meas[1, 4] = np.nan
    asym = np.stack([np.eye(7), np.eye(7)])
    asym[1, 0, 3] = 0.5
    for v0, v1, m, info in (([5, 9], [120, 9], meas, None), ([5, 9], [120, 100000], meas, None),
                            ([5, 9], [120, 150], meas, bad_info), ([5, 9], [120, 150], nan_meas, None),
                            ([5, 9], [120, 150], meas, asym)):
        out = (np.full((2, 7), -3.0), np.full((2, 49), -3.0), np.full(2, -3.0))
        with pytest.raises(L.Sim3OptError) as e:
            G.gate_edges(v0, v1, m, info=info, out=out)
        assert e.value.code == L.ERR_ARG
        assert all(np.all(o == -3.0) for o in out)
    e0, S0, d0 = G.gate_edges(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 8)))
    assert e0.shape == (0, 7) and S0.shape == (0, 7, 7) and d0.shape == (0,)
    G.close()


@pytest.mark.parametrize("name", ["kitti_direct", "chain_200_pcg"])
def test_covariances_and_gate_between_optimize_calls_change_nothing(name):
    """optimize(5); covariances + gate_edges; optimize(5) is bit-identical to optimize(5); optimize(5)"""
    if name == "kitti_direct":
        g, opts = K.build_direct_graph(True), {}
    else:
        g, opts = synth.chain_loop(200, 230), dict(linear_solver=0, fix_small_angle_b=1)
    runs = []
    for with_call in (False, True):
        G, _ = mk(g, **opts)
        assert G.linear_solver_in_use() == (1 if name == "kitti_direct" else 0)
        n1 = G.optimize(5)
        s1 = [(s.trials, s.chi2_before, s.chi2_after, s.lambda_, s.pcg_iters) for s in G.stats()]
        if with_call:
            assert np.isfinite(G.covariances([(1, 150), (150, 1), (2, 2), (1, 2)], 1e-2)).all()
            try:  # (KITTI-00 at its noise floor: H may be numerically singular -- a failing call must not interfere)
                G.covariances([(1, 150)], 0.0)
            except L.Sim3OptError as e:
                assert e.code == L.ERR_STATE
            meas = np.tile(np.array([0, 0, 0, 1, 0.5, 0, 0, 1.0]), (3, 1))
            _, _, d2 = G.gate_edges([1, 3, 0], [150, 90, 60], meas, lam=1e-2)  # (vertex 0 is fixed)
            assert np.isfinite(d2).all() and (d2 > 0).all()
        n2 = G.optimize(5)
        s2 = [(s.trials, s.chi2_before, s.chi2_after, s.lambda_, s.pcg_iters) for s in G.stats()]
        runs.append((n1, s1, n2, s2, np.array(G.get_vertices(), copy=True), G.chi2()))
        G.close()
    a, b = runs
    assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2] and a[3] == b[3]
    assert np.array_equal(a[4], b[4]) and a[5] == b[5]


# ---- the gate against a numpy restatement ----

def gate_candidates(g, states):
    """64 seeded pairs of vertices no edge joins (the last two with the fixed vertex 0 as an endpoint), each as three
    candidates: the current relative pose S1 S0^-1 composed with exp of a seeded tangent scaled to norm 0, 1e-3, 0.3.
    Returns (v0, v1, meas) with candidate 3 p + k = pair p, norm k."""
    rng = np.random.default_rng(41)
    opt = O.default_options(fix_small_angle_b=1)
    V = g["states"].shape[0]
    joined = set(zip(g["v0"].tolist(), g["v1"].tolist())) | set(zip(g["v1"].tolist(), g["v0"].tolist()))
    assert g["fixed"][0] == 1 and g["fixed"].sum() == 1
    pairs = []
    while len(pairs) < 64:
        a, b = (int(x) for x in rng.integers(1, V, 2))
        if len(pairs) >= 62:
            a, b = (0, b) if len(pairs) == 62 else (a, 0)
        if a != b and (a, b) not in joined and (a, b) not in pairs:
            pairs.append((a, b))
    v0, v1, meas = [], [], []
    for a, b in pairs:
        rel = O.sim3_mul(states[b], O.sim3_inv(states[a]))
        xi = rng.standard_normal(7)
        xi /= np.linalg.norm(xi)
        for norm in (0.0, 1e-3, 0.3):
            v0.append(a)
            v1.append(b)
            meas.append(O.sim3_mul(O.sim3_exp(norm * xi, opt), rel))
    return np.array(v0, np.int32), np.array(v1, np.int32), np.array(meas)


@pytest.mark.parametrize("mode", ["analytic", "numeric", "numeric_1e-6"])
def test_gate_matches_numpy_restatement(mode):
    """S = J Sigma J^T + Omega^-1 and d2 = e^T S^-1 e with Sigma from the dense inverse of the system the library
    linearised, e from oracle.edge_error, J from oracle.edge_jacobians at delta = 1e-6.

    Bounds (2-norms, per candidate).  Sigma carries the covariance bound of test_covariances_match_dense_inverse,
    dSigma = 14 max(1e-10, 1e3 n eps cond2) max|Sigma| (a 14 x 14 matrix of entries that good), J the relative
    error dJ = JAC_MARGIN * JAC_REFS_DISAGREE (module docstring; measured again below and printed), Omega^-1 its
    Cholesky's rounding:  |dS| <= |J|^2 dSigma + (2 dJ + dJ^2) |J|^2 |Sigma| + 1e-13 |Omega^-1|,
    |d d2| <= |S^-1 e|^2 |dS| + 2 |S^-1 e| |de| with |de| = 1e-13 max(1, |e|), the bound the device's residual is
    held to elsewhere (test_gpu_analytic_jacobians.py).
    With options.jacobians = 0 the device's J are central differences with fd_delta and carry that mode's rounding
    noise, eps |e| / fd_delta per entry: ~1e-7 at the default fd_delta = 1e-9, inside dJ = 3e-5, so the one bound
    serves every mode.  Measured error / bound: S 2.0e-4 (closed form), 7.7e-4 (fd_delta = 1e-9), 2.3e-9 (1e-6);
    d2 7.6e-6, 1.3e-4, 7.0e-10; the figures are printed per mode."""
    opts = {"analytic": dict(jacobians=1), "numeric": dict(jacobians=0),
            "numeric_1e-6": dict(jacobians=0, fd_delta=1e-6)}
    g = R.GRAPHS["manhattan_300"]()
    G, _ = mk(g, linear_solver=1, fix_small_angle_b=1, **opts[mode])
    G.optimize(3)
    states = np.array(G.get_vertices(), copy=True)
    v0, v1, meas = gate_candidates(g, states)
    m = v0.size
    half = m // 2  # the first 32 pairs without an information matrix, the others with a random SPD one
    rng = np.random.default_rng(43)
    M = rng.standard_normal((m - half, 7, 7)) * 0.3
    info = np.einsum("kij,klj->kil", M, M) + np.eye(7)
    e, S, d2 = (np.concatenate(x) for x in zip(G.gate_edges(v0[:half], v1[:half], meas[:half]),
                                               G.gate_edges(v0[half:], v1[half:], meas[half:], info=info[:])))
    eI, SI, dI = G.gate_edges(v0[:half], v1[:half], meas[:half], info=np.tile(np.eye(7), (half, 1, 1)))
    assert np.array_equal(eI, e[:half]) and np.array_equal(SI, S[:half]) and np.array_equal(dI, d2[:half])
    # the system the library linearised, its dense inverse
    G.linearize()
    H, _ = G.dense_system()
    n = H.shape[0]
    ev = np.linalg.eigvalsh(H)
    cond = ev[-1] / ev[0]
    Zr = np.linalg.inv(H)
    row = np.full(g["fixed"].shape[0], -1)
    row[g["fixed"] == 0] = np.arange(n // 7)
    covrel = max(1e-10, 1e3 * n * EPS * cond)
    oopt = O.default_options(fix_small_angle_b=1, fd_delta=1e-6)
    Sig = np.zeros((m, 14, 14))
    for k in range(m):
        r = (row[v0[k]], row[v1[k]])
        for i in range(2):
            for j in range(2):
                if r[i] >= 0 and r[j] >= 0:
                    Sig[k, 7 * i:7 * i + 7, 7 * j:7 * j + 7] = Zr[7 * r[i]:7 * r[i] + 7, 7 * r[j]:7 * r[j] + 7]
    dSigma = 14 * covrel * np.abs(Sig).max()
    dJ = JAC_MARGIN * JAC_REFS_DISAGREE
    worst = dict(S=0.0, d2=0.0, refs=0.0, e=0.0)
    refs = np.zeros(3)  # the references' disagreement by perturbation: 0, 1e-3, 0.3
    fails = []
    for k in range(m):
        s0, s1 = states[v0[k]], states[v1[k]]
        er = O.edge_error(meas[k], s0, s1, oopt)
        A, B = O.edge_jacobians(meas[k], s0, s1, oopt)
        J = np.hstack([A, B])
        _, Jh = L.edge_jacobian_host(meas[k], s0, s1)
        refs[k % 3] = max(refs[k % 3], np.linalg.norm(J - Jh, 2) / np.linalg.norm(Jh, 2))
        Oi = np.eye(7) if k < half else np.linalg.inv(info[k - half])
        Sr = J @ Sig[k] @ J.T + Oi
        x = np.linalg.solve(Sr, er)
        dr = float(er @ x)
        nJ2 = np.linalg.norm(J, 2) ** 2
        tS = nJ2 * dSigma + (2 * dJ + dJ * dJ) * nJ2 * np.linalg.norm(Sig[k], 2) + 1e-13 * np.linalg.norm(Oi, 2)
        de = 1e-13 * max(1.0, np.linalg.norm(er))
        td = np.linalg.norm(x) ** 2 * tS + 2 * np.linalg.norm(x) * de
        errS, errd, erre = np.linalg.norm(S[k] - Sr, 2), abs(d2[k] - dr), np.abs(e[k] - er).max()
        worst["S"] = max(worst["S"], errS / tS)
        worst["d2"] = max(worst["d2"], errd / td if td > 0 else 0.0)
        worst["e"] = max(worst["e"], erre / de)
        if not (errS <= tS and erre <= de):
            fails.append(("S / e", k, errS, tS, erre, de))
        if k % 3 == 0:  # no perturbation: e and d2 vanish
            if not (np.linalg.norm(e[k]) <= 1e-12 and d2[k] <= 1e-20):
                fails.append(("zero", k, np.linalg.norm(e[k]), d2[k]))
        elif not errd <= td:
            fails.append(("d2", k, errd, td))
        assert np.array_equal(S[k], S[k].T)
    worst["refs"] = refs.max()
    print(f"gate {mode}: cond2 {cond:.3e}, covariance bound {covrel:.2e}, the two reference Jacobians differ by "
          f"{refs[0]:.2e} / {refs[1]:.2e} / {refs[2]:.2e} (allowed on the device: {dJ:.1e}); worst error / bound: "
          f"S {worst['S']:.2e}, d2 {worst['d2']:.2e}, e {worst['e']:.2e}; d2 in [{d2.min():.2e}, {d2.max():.2e}]")
    assert worst["refs"] <= JAC_REFS_DISAGREE
    assert not fails, fails[:5]
    # the same pair, farther off: a larger distance
    assert np.all(d2[2::3] > d2[1::3]) and np.all(d2[1::3] > d2[0::3])
    G.close()
