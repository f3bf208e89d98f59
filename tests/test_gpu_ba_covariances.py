"""GPU tests (-m gpu) of the bundle-adjustment covariances (sim3opt_ba_covariances; BundleAdjuster.covariances): blocks of
(H + lambda I)^-1 over cameras and points by the selected inversion of the reduced camera system, against the dense
long-double inverse of the oracle's normal matrix (tests/ba_cov_ref.py) by the comparison rule of the marginals' test
applied to the diagonally equilibrated system; the request's order, duplicates and split, the schedule knobs, the error
paths and the absence of side effects."""
import numpy as np
import pytest

from sim3opt_amd import lib as L
import ba_cov_cases as CC
import ba_cov_ref as CR

pytestmark = pytest.mark.gpu


def mk(P, fixed=None, **opts):
    b = L.BundleAdjuster(**opts)
    b.set_problem(P.cams, P.points, P.oc, P.op, P.uv, P.f, P.cx, P.cy)
    fixed = P.fixed if fixed is None else fixed
    if np.any(fixed):
        b.set_fixed_cameras(np.asarray(fixed).astype(np.uint8))
    return b


_defs = {}


def definition(name, lam):
    if (name, lam) not in _defs:
        _defs[(name, lam)] = CR.Definition(CC.problem(name), lam)
    return _defs[(name, lam)]


def bits(*arrays):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)


@pytest.mark.parametrize("name,lam", CC.ACCURACY)
def test_covariances_match_the_dense_inverse(name, lam):
    P = CC.problem(name)
    if name == "cov_tracks":
        CC.check_tracks(P)
    D = definition(name, lam)
    assert D.bound < 1e-3  # the rule's condition on its inputs
    cam_pairs, points, pc = CC.requests(P)
    b = mk(P)
    cc, pp, pcb = b.covariances(cam_pairs, points, pc, lam=lam)
    assert cc.shape == (len(cam_pairs), 6, 6) and pp.shape == (len(points), 3, 3) and pcb.shape == (len(pc), 3, 6)
    worst = dict(cc=D.worst(cam_pairs, cc, [], [], [], []), pp=D.worst([], [], points, pp, [], []),
                 pc=D.worst([], [], [], [], pc, pcb))
    print(f"[ba-cov] {name} lambda={lam:g}: cond2 {D.cond:.3e}, bound {D.bound:.2e}, worst block ratios "
          + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst
    fixed = np.asarray(P.fixed, dtype=bool)
    diag = cam_pairs[:, 0] == cam_pairs[:, 1]
    # diagonal camera blocks and point blocks: exactly symmetric, Cholesky-factorable
    assert np.array_equal(cc[diag], cc[diag].transpose(0, 2, 1)) and np.array_equal(pp, pp.transpose(0, 2, 1))
    for M in cc[diag & ~fixed[cam_pairs[:, 0]]]:
        np.linalg.cholesky(M)
    for M in pp:
        np.linalg.cholesky(M)
    # the reversed pair is the exact transpose (the request holds both orders)
    where = {(int(a), int(c)): q for q, (a, c) in enumerate(cam_pairs)}
    for (a, c), q in where.items():
        assert np.array_equal(cc[where[(c, a)]], cc[q].T)
    # fixed cameras: exact zeros
    fc = fixed[cam_pairs[:, 0]] | fixed[cam_pairs[:, 1]]
    assert fc.any() and not cc[fc].any() and not np.signbit(cc[fc]).any()
    assert not pcb[fixed[pc[:, 1]]].any() and not np.signbit(pcb[fixed[pc[:, 1]]]).any()
    # the conveniences are the same numbers
    assert np.array_equal(b.camera_covariances(lam), cc[diag]) and np.array_equal(b.point_covariances(lam), pp)
    if name == "cov_tracks":
        # a point seen by fixed cameras only: H_pp^-1 of the reduced system's read-out, bit for bit
        Hi = b.debug_reduced(lam)["Hpp_inv"][CC.FIXED_ONLY_POINT]
        assert np.array_equal(pp[CC.FIXED_ONLY_POINT], Hi)
        st = b.covariance_stats()
        assert st["columns"] == 12 and st["selinv"] == 1 and st["blocks"] >= 12
        free_obs = np.bincount(P.op[~fixed[P.oc]], minlength=len(points))
        assert st["point_pair_terms"] == int((free_obs ** 2).sum())
    b.close()


def test_the_request_does_not_change_the_bits():
    P = CC.problem("cov_tracks")
    cam_pairs, points, pc = CC.requests(P)
    lam = 1e-2
    b = mk(P)
    cc, pp, pcb = b.covariances(cam_pairs, points, pc, lam=lam)
    # a repeated call
    assert bits(*b.covariances(cam_pairs, points, pc, lam=lam)) == bits(cc, pp, pcb)
    # the three kinds in three calls
    assert bits(b.covariances(cam_pairs=cam_pairs, lam=lam)[0]) == bits(cc)
    assert bits(b.covariances(points=points, lam=lam)[1]) == bits(pp)
    assert bits(b.covariances(point_cams=pc, lam=lam)[2]) == bits(pcb)
    # any order, with duplicates
    rng = np.random.default_rng(3)
    for _ in range(2):
        i = rng.integers(0, len(cam_pairs), 2 * len(cam_pairs))
        j = rng.integers(0, len(points), 2 * len(points))
        k = rng.integers(0, len(pc), 2 * len(pc))
        c2, p2, x2 = b.covariances(cam_pairs[i], points[j], pc[k], lam=lam)
        assert bits(c2, p2, x2) == bits(cc[i], pp[j], pcb[k])
    # split into pieces (the three request lists cut at the same piece size)
    for piece in (1, 63, 64, 65, 300):
        sel = [np.arange(n) for n in (len(cam_pairs), len(points), len(pc))]
        for req, ref, key in ((cam_pairs, cc, "cam_pairs"), (points, pp, "points"), (pc, pcb, "point_cams")):
            idx = sel[("cam_pairs", "points", "point_cams").index(key)]
            got = []
            for s in range(0, len(idx), piece):
                out = b.covariances(**{key: req[idx[s:s + piece]]}, lam=lam)
                got.append(next(o for o in out if o is not None))
            assert bits(np.concatenate(got)) == bits(ref[idx]), (piece, key)
    # empty requests
    lib = L.load()
    assert lib.sim3opt_ba_covariances(b._b, lam, 0, None, None, None, 0, None, None, 0, None, None, None) == L.OK
    e = np.zeros((0, 2), dtype=np.int32)
    c0, p0, x0 = b.covariances(e, np.zeros(0, dtype=np.int32), e, lam=lam)
    assert c0.shape == (0, 6, 6) and p0.shape == (0, 3, 3) and x0.shape == (0, 3, 6)
    assert b.covariance_stats()["selinv"] == 0
    b.close()


def test_covariances_do_not_depend_on_the_schedule(monkeypatch):
    """Bottom-subtree size and wavefronts per bottom group change which workgroup factors and inverts what, never the
    order of summation: the same bits under every schedule."""
    P = CC.problem("branches")
    cam_pairs, points, pc = CC.requests(P)
    ref, groups = None, set()
    for subtree, wg in (("16", "256"), ("3", "512"), ("6", "384"), ("1", "64")):
        monkeypatch.setenv("SIM3OPT_BA_SUBTREE", subtree)
        monkeypatch.setenv("SIM3OPT_BA_WG_SUB", wg)
        b = mk(P)
        cur = bits(*b.covariances(cam_pairs, points, pc, lam=1e-2))
        groups.add(b.covariance_plan()["ngroups"])
        b.close()
        ref = cur if ref is None else ref
        assert cur == ref, (subtree, wg)
    print(f"[ba-cov] group counts of the schedules: {sorted(groups)}")
    assert len(groups) > 1


def off_pattern_pair(b, fixed):
    """two free cameras whose block the covariances' factor does not store (from its plan), or None"""
    Q = b.covariance_plan()
    stored = set(zip(Q["lrow"].tolist(), np.repeat(np.arange(Q["nb"]), np.diff(Q["colptr"])).tolist()))
    pos = np.empty(Q["nb"], dtype=np.int64)
    pos[Q["perm"]] = np.arange(Q["nb"])
    return next(((a, c) for a in range(Q["nb"]) for c in range(a)
                 if not fixed[a] and not fixed[c] and (max(pos[a], pos[c]), min(pos[a], pos[c])) not in stored), None)


def test_covariance_error_paths(monkeypatch):
    lib = L.load()
    # no problem set
    b = L.BundleAdjuster()
    out = np.full(36, 7.0)
    z = np.zeros(1, dtype=np.int32)
    args = lambda lam: (b._b, lam, 1, L._p(z, L._ip), L._p(z, L._ip), L._p(out, L._dp), 0, None, None, 0, None, None, None)
    assert lib.sim3opt_ba_covariances(*args(1.0)) == L.ERR_STATE
    b.close()
    # no fixed camera: the gauge makes H singular at lambda = 0 -- an error, never NaN; damped it is well posed
    P = CC.problem("cov_tracks")
    for opts in (dict(), dict(linear_solver=0)):
        b = mk(P, fixed=np.zeros(12, dtype=bool), **opts)
        with pytest.raises(L.Sim3OptError) as e:
            b.camera_covariances(0.0)
        assert e.value.code == L.ERR_STATE
        assert np.isfinite(b.camera_covariances(1.0)).all() and np.isfinite(b.point_covariances(1.0)).all()
        b.close()
    # lists at lambda = 0: a point seen once
    Pl = CC.problem("lists")
    bad = CR.point_pivot_fails(Pl, 0.0)
    assert bad
    b = mk(Pl)
    with pytest.raises(L.Sim3OptError) as e:
        b.point_covariances(0.0)
    assert e.value.code == L.ERR_STATE and f"point {bad[0]}:" in str(e.value), str(e.value)
    assert np.isfinite(b.point_covariances(1.0)).all()  # the handle still answers
    b.close()
    # ERR_ARG, outputs untouched
    b = mk(CC.problem("branches"))  # 8 separate groups of cameras: pairs across groups share nothing
    nc, npt, _ = b.dims()
    P = CC.problem("branches")
    pair = off_pattern_pair(b, P.fixed)
    assert pair is not None
    assert not (set(P.op[P.oc == pair[0]]) & set(P.op[P.oc == pair[1]]))  # no common point
    seen_by_first = int(P.op[P.oc == pair[0]][0])

    def refused(lam, cam_pairs=(), points=(), point_cams=()):
        a = np.ascontiguousarray(np.array(cam_pairs, dtype=np.int32).reshape(-1, 2))
        ca, cb = np.ascontiguousarray(a[:, 0]), np.ascontiguousarray(a[:, 1])
        pt = np.array(points, dtype=np.int32).reshape(-1)
        q = np.array(point_cams, dtype=np.int32).reshape(-1, 2)
        qp, qc = np.ascontiguousarray(q[:, 0]), np.ascontiguousarray(q[:, 1])
        cc, pp, pcb = np.full(36 * len(ca) + 1, 7.0), np.full(9 * len(pt) + 1, 7.0), np.full(18 * len(qp) + 1, 7.0)
        rc = lib.sim3opt_ba_covariances(b._b, lam, len(ca), L._p(ca, L._ip), L._p(cb, L._ip), L._p(cc, L._dp), len(pt),
                                        L._p(pt, L._ip), L._p(pp, L._dp), len(qp), L._p(qp, L._ip), L._p(qc, L._ip),
                                        L._p(pcb, L._dp))
        assert (cc == 7.0).all() and (pp == 7.0).all() and (pcb == 7.0).all()  # nothing written
        return rc

    free = 1  # (cameras 0, 3, 6, ... of branches are fixed)
    assert refused(1.0, cam_pairs=[(free, free), pair]) == L.ERR_ARG
    assert b"outside the pattern" in lib.sim3opt_ba_last_error(b._b)
    assert refused(1.0, cam_pairs=[(free, free)], point_cams=[(seen_by_first, pair[1])]) == L.ERR_ARG
    for cam in (-1, nc):
        assert refused(1.0, cam_pairs=[(free, cam)]) == L.ERR_ARG and refused(1.0, cam_pairs=[(cam, free)]) == L.ERR_ARG
        assert refused(1.0, point_cams=[(0, cam)]) == L.ERR_ARG
    for p in (-1, npt):
        assert refused(1.0, points=[0, p]) == L.ERR_ARG and refused(1.0, point_cams=[(p, free)]) == L.ERR_ARG
    for lam in (-1.0, float("nan"), float("inf")):
        assert refused(lam, cam_pairs=[(free, free)], points=[0]) == L.ERR_ARG
    assert np.isfinite(b.covariances(cam_pairs=[(free, free)], lam=1.0)[0]).all()  # still usable
    b.close()
    # linear_solver = 0 handles still answer (the context is the covariances' own), with the same bits
    P = CC.problem("cov_small")
    cam_pairs, points, pc = CC.requests(P)
    b0, b1 = mk(P, linear_solver=0), mk(P)
    assert bits(*b0.covariances(cam_pairs, points, pc, lam=0.0)) == bits(*b1.covariances(cam_pairs, points, pc, lam=0.0))
    b0.close()
    b1.close()
    # a refused plan: ERR_STATE, remembered, and the handle still optimises
    for var in ("SIM3OPT_BA_COV_MAX_PAIRS", "SIM3OPT_BA_MAX_PAIRS"):
        monkeypatch.setenv(var, "1")
        b = mk(P)
        for _ in range(2):
            with pytest.raises(L.Sim3OptError) as e:
                b.camera_covariances(1.0)
            assert e.value.code == L.ERR_STATE
        assert b.optimize(2) == 2
        monkeypatch.delenv(var)
        b.close()


def readout(b):
    return bits(b.cameras(), b.points(), np.array([b.chi2()]),
                np.array([[s[k] for k in sorted(s)] for s in b.stats()], dtype=np.float64))


@pytest.mark.parametrize("solver", [-1, 0])
def test_covariances_between_optimize_calls_change_nothing(solver):
    """optimize(3); covariances (a failing call included); optimize(3) is bit for bit optimize(3); optimize(3)"""
    P = CC.problem("cov_tracks")
    cam_pairs, points, pc = CC.requests(P)
    runs = []
    for with_calls in (False, True):
        b = mk(P, linear_solver=solver)
        assert b.optimize(3) == 3
        first = readout(b)
        if with_calls:
            cc, pp, pcb = b.covariances(cam_pairs, points, pc, lam=1e-2)
            assert np.isfinite(cc).all() and np.isfinite(pp).all() and np.isfinite(pcb).all()
            with pytest.raises(L.Sim3OptError):
                b.covariances(cam_pairs=[(2, 2)], lam=-1.0)
            with pytest.raises(L.Sim3OptError):
                b.covariances(points=[len(points)], lam=1.0)
            b.point_covariances(0.0)
        assert b.optimize(3) == 3
        runs.append((first, readout(b), bits(b.debug_reduced(1.0)["S"], b.debug_step(1.0, solver=0, pcg_max_iters=5)["dx_c"])))
        b.close()
    assert runs[0] == runs[1]


def test_a_singular_call_changes_nothing_either():
    P = CC.problem("lists")
    runs = []
    for with_calls in (False, True):
        b = mk(P)
        assert b.optimize(3) == 3
        if with_calls:
            with pytest.raises(L.Sim3OptError) as e:
                b.point_covariances(0.0)
            assert e.value.code == L.ERR_STATE
        assert b.optimize(3) == 3
        runs.append(readout(b))
        b.close()
    assert runs[0] == runs[1]


def test_device_memory_and_the_poisoned_mode():
    P = CC.problem("cov_small")
    cam_pairs, points, pc = CC.requests(P)
    L.release_device_cache()
    start = L.device_memory_in_use()
    b = mk(P)
    ref = bits(*b.covariances(cam_pairs, points, pc, lam=1e-2))
    held = L.device_memory_in_use()
    for _ in range(3):
        assert bits(*b.covariances(cam_pairs, points, pc, lam=1e-2)) == ref
        assert L.device_memory_in_use() == held
    b.close()
    assert L.device_memory_in_use() == start
    # poisoned blocks with guarded tails: the same bits, no overwritten tail
    L.debug_device_memory(True)
    try:
        b = mk(P)
        assert bits(*b.covariances(cam_pairs, points, pc, lam=1e-2)) == ref
        assert bits(*b.covariances(cam_pairs, points, pc, lam=1e-2)) == ref
        b.close()
        L.release_device_cache()
        rep = L.debug_device_memory_report()
    finally:
        L.debug_device_memory(False)
    assert rep["filled"] > 0 and rep["checked"] > 0 and rep["overwritten"] == 0, rep
