"""The batched two-view refinement on the GPU (sim3opt_ba_batch, sim3opt_amd/csrc/ba_batch.hip: one workgroup per
problem, the whole LM loop in one launch) against oracle/ba_oracle.py in BAOptimize's configuration
(kittiDetector.h:845-954): camera 0 fixed, Huber 3, lambda_0 = 50, 5 trials, 10 iterations.  The cases and their
reference runs are tests/two_view_cases.py's; tests/test_two_view_batch.py shows on the CPU that their trial counts
are stable.  Tolerances are tests/test_ba.py's for the same comparisons."""
import os
import subprocess

import numpy as np
import pytest

import two_view_cases as TC
from sim3opt_amd import lib as L

pytestmark = pytest.mark.gpu


def run_batch(cases, arrays=None, **opts):
    a = TC.batch_arrays(cases) if arrays is None else arrays
    b = L.TwoViewBatch(**opts)
    b.set_problems(**a)
    assert b.optimize() == len(cases)
    return b


def snapshot(b):
    """Everything a run returns, as arrays that can be compared bit for bit."""
    n = b.dims()[0]
    c0, c1 = b.cameras()
    st = [np.array([[s[k] for k in ("chi2_before", "chi2_after", "lambda_", "rho", "trials")] for s in b.stats(p)])
          for p in range(n)]
    chi = b.chi2()
    return dict(cam0=c0, cam1=c1, points=b.points(), stats=st, iters=b.num_iterations(),
                active_before=chi["active_before"], active_after=chi["active_after"], edge_chi2=chi["edge_chi2"],
                n_outlier_edges=chi["n_outlier_edges"], lambda_init=b.lambda_init())


def problem_of(snap, ptr, k):
    """Problem k's share of a snapshot."""
    lo, hi = int(ptr[k]), int(ptr[k + 1])
    return [snap["cam1"][k], snap["points"][lo:hi], snap["stats"][k], snap["iters"][k:k + 1],
            snap["active_before"][k:k + 1], snap["active_after"][k:k + 1], snap["edge_chi2"][lo:hi],
            snap["n_outlier_edges"][k:k + 1], snap["lambda_init"][k:k + 1]]


def same_bits(x, y):
    return all(a.shape == b.shape and a.tobytes() == b.tobytes() for a, b in zip(x, y))


_default_run = {}


def default_run():
    """The whole-run batch under default options: run once, shared; do not modify."""
    if not _default_run:
        a = TC.batch_arrays(TC.WHOLE_RUN_CASES)
        _default_run.update(arrays=a, snap=snapshot(run_batch(TC.WHOLE_RUN_CASES, a)))
    return _default_run["arrays"], _default_run["snap"]


def check_whole_run(snap, ptr, k, case, opts=()):
    """Problem k of a run against the oracle's run of `case`: the comparisons of the issue's test 2."""
    ref = TC.reference(*case, tuple(sorted(dict(opts).items())))
    cam1, pts, st, iters, ab, aa, ec, nout, _ = problem_of(snap, ptr, k)
    tr = ref["trace"]
    assert int(iters[0]) == len(tr) == len(st), (case, int(iters[0]), len(tr))
    assert [int(t) for t in st[:, 4]] == [t["trials"] for t in tr], case
    for i, t in enumerate(tr):
        assert abs(st[i, 1] - t["chi2"]) <= 1e-7 * t["chi2"], (case, i, st[i, 1], t["chi2"])
        assert abs(st[i, 2] - t["lam"]) <= 1e-5 * t["lam"], (case, i, st[i, 2], t["lam"])
    assert abs(st[0, 0] - ref["chi2_before"]) <= 1e-12 * ref["chi2_before"]
    assert TC.quat_dist(cam1[:4], ref["cam1"][:4]) < 1e-8, case
    assert np.abs(cam1[4:] - ref["cam1"][4:]).max() < 1e-7, case
    assert np.abs(pts - ref["points"]).max() < 1e-6, case
    assert abs(ab[0] - ref["active_before"]) <= 1e-7 * ref["active_before"]
    assert abs(aa[0] - ref["active_after"]) <= 1e-7 * ref["active_after"]
    # e->chi2() of every observation, each to 1e-7 relative (measured: at most 1e-9, on observations of chi2 1e-6)
    assert (np.abs(ec - ref["edge_chi2"]) <= 1e-7 * ref["edge_chi2"]).all(), case
    thr = dict(TC.DEFAULTS, **dict(opts))["outlier_chi2"]
    assert (np.abs(ref["edge_chi2"] - thr) > 1e-6 * thr).all()  # no observation on the threshold: none excluded
    assert int(nout[0]) == int((ref["edge_chi2"] > thr).sum()), case


def test_one_iteration_matches_oracle_solve():
    """One LM iteration of a ragged batch whose sizes sit around one, two and three passes of the 256-thread
    stride, the degenerate sizes 1 and 2 included: the Schur-complement step of the kernel against the oracle's
    sparse LU of the whole damped system."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    cases = TC.ONE_ITERATION_CASES
    a = TC.batch_arrays(cases)
    b = run_batch(cases, a, max_iters=1)
    snap, ptr = snapshot(b), a["point_ptr"]
    lam = TC.DEFAULTS["user_lambda_init"]
    for k, case in enumerate(cases):
        P = TC.oracle_problem(TC.make_case(*case), TC.DEFAULTS)
        H, rhs, chi = P.system()
        dx = spla.spsolve((H + lam * sp.identity(H.shape[0])).tocsc(), rhs)
        cn, pn = P.apply(P.cams, P.points, dx)
        cam1, pts, st, iters = problem_of(snap, ptr, k)[:4]
        assert int(iters[0]) == 1 and st.shape == (1, 5)
        assert abs(st[0, 0] - chi) <= 1e-12 * chi, (case, st[0, 0], chi)
        chi_new = P.chi2(cn, pn)
        assert chi_new < chi, case  # (every case's first step is a good one: the estimate moves by it)
        assert st[0, 4] == 1, case
        assert TC.quat_dist(cam1[:4], cn[1, :4]) < 1e-11, case
        assert np.abs(cam1[4:] - cn[1, 4:]).max() < 1e-10, case
        assert np.abs(pts - pn).max() < 1e-9, case
        assert abs(st[0, 1] - chi_new) <= 1e-9 * chi, (case, st[0, 1], chi_new)


def test_whole_run_matches_oracle():
    a, snap = default_run()
    for k, case in enumerate(TC.WHOLE_RUN_CASES):
        check_whole_run(snap, a["point_ptr"], k, case)
    assert (snap["lambda_init"] == 50.0).all()


def test_whole_run_on_every_quaternion_branch():
    """BRANCH_CASES: case (65, 24) in worlds moved so that camera 1 stays on the x, y, z or trace branch of Eigen's
    matrix -> quaternion rule through the whole run (tests/test_two_view_batch.py shows it for the oracle) and camera 0
    is far from the identity: the same comparisons as any whole run, and the final chi2 is the device's own for the
    base case to 1e-7 relative -- the refinement does not depend on the gauge."""
    import ba_ref as BR
    cases = TC.BRANCH_CASES + (TC.BRANCH_BASE,)
    a = TC.batch_arrays(cases)
    snap = snapshot(run_batch(cases, a))
    base = problem_of(snap, a["point_ptr"], len(cases) - 1)[2][-1, 1]
    for k, case in enumerate(TC.BRANCH_CASES):
        check_whole_run(snap, a["point_ptr"], k, case)
        want = TC.GAUGE_BRANCH[case[2]]
        assert list(BR.quat_branch(np.stack([a["cam1"][k], snap["cam1"][k]]))) == [want, want], case
        chi = problem_of(snap, a["point_ptr"], k)[2][-1, 1]
        assert abs(chi - base) <= 1e-7 * base, (case, chi, base)


def test_second_optimize_continues_from_the_first():
    """optimize() with max_iters = 4, then again with max_iters = 6 and no set_problems in between: "another call
    continues from them" (include/sim3opt.h).  Against the oracle's optimize(4) followed by optimize(6) on the same
    Problem, each restarting at lambda_0 = 50 and ni = 2 (tests/test_two_view_batch.py: that pair of traces is stable),
    with check_whole_run's tolerances for either call."""
    cases = TC.CONTINUED_CASES
    a = TC.batch_arrays(cases)
    b = L.TwoViewBatch()
    b.set_problems(**a)
    for call, iters in enumerate(TC.CONTINUED_ITERS):
        b.set_options(max_iters=iters)
        assert b.optimize() == len(cases)
        snap = snapshot(b)
        for k, case in enumerate(cases):
            ref = TC.continued_reference(*case)[call]
            cam1, pts, st, n_it, ab, aa, ec, _, lam0 = problem_of(snap, a["point_ptr"], k)
            tr = ref["trace"]
            assert int(n_it[0]) == len(tr) == iters and lam0[0] == 50.0
            assert [int(t) for t in st[:, 4]] == [t["trials"] for t in tr], (case, call)
            for i, t in enumerate(tr):
                assert abs(st[i, 1] - t["chi2"]) <= 1e-7 * t["chi2"], (case, call, i)
                assert abs(st[i, 2] - t["lam"]) <= 1e-5 * t["lam"], (case, call, i)
            tol0 = 1e-12 if call == 0 else 1e-7  # (the second call starts from the first's result, not from the input)
            assert abs(st[0, 0] - ref["chi2_before"]) <= tol0 * ref["chi2_before"]
            assert TC.quat_dist(cam1[:4], ref["cam1"][:4]) < 1e-8 and np.abs(cam1[4:] - ref["cam1"][4:]).max() < 1e-7
            assert np.abs(pts - ref["points"]).max() < 1e-6, (case, call)
            assert abs(ab[0] - ref["active_before"]) <= 1e-7 * ref["active_before"]
            assert abs(aa[0] - ref["active_after"]) <= 1e-7 * ref["active_after"]
            assert (np.abs(ec - ref["edge_chi2"]) <= 1e-7 * ref["edge_chi2"]).all(), (case, call)
    b.close()


def test_problem_whose_sums_are_not_finite_beside_healthy_ones():
    """A 12-point problem one of whose points has X_z = 0 exactly in camera 1 (two_view_cases.degenerate_case), between
    two healthy problems.  Its projection divides by zero: the robust chi2 of the start is +inf, every entry of the
    reduced system is NaN, the Cholesky reports a non-positive pivot and the trial's chi2 is DBL_MAX.
    lm_damping.hpp's statements (run on the host in tests/test_two_view_batch.py) then give rho = +inf, the failed
    trial counted as accepted with nothing to accept, lambda / 3, and no reason to stop: 10 iterations of one trial.
    The kernel returns (every loop is bounded), camera and points come back bit-identical to the start, and the
    neighbours give the bytes they give alone.  (oracle/ba_oracle.py solves the non-finite system by LU, gets a NaN
    chi2 and rejects: also 10 x 1 trial, with lambda growing instead; DESIGN.md.)"""
    import test_two_view_batch as TH
    bad = TC.degenerate_case()
    healthy = [TC.make_case(*TC.WHOLE_RUN_CASES[3]), TC.make_case(*TC.WHOLE_RUN_CASES[0])]
    a = TC.arrays_of([healthy[0], bad, healthy[1]])
    b = L.TwoViewBatch()
    b.set_problems(**a)
    start = (b.cameras()[1], b.points())
    assert b.optimize() == 3
    snap, ptr = snapshot(b), a["point_ptr"]
    for k, c in ((0, healthy[0]), (2, healthy[1])):
        one = TC.arrays_of([c])
        alone = snapshot(run_batch((None,), one))
        assert same_bits(problem_of(alone, one["point_ptr"], 0), problem_of(snap, ptr, k)), k
    cam1, pts, st, n_it = problem_of(snap, ptr, 1)[:4]
    iters, trials, lam_ratio = TH.DAMPING_INF_FAIL
    assert int(n_it[0]) == iters and [int(t) for t in st[:, 4]] == trials
    assert (st[:, 0] == np.inf).all() and (st[:, 1] == np.finfo(np.float64).max).all() and (st[:, 3] == np.inf).all()
    assert abs(st[-1, 2] - 50.0 * lam_ratio) <= 1e-14 * 50.0 * lam_ratio
    assert np.array_equal(cam1, start[0][1]) and np.array_equal(pts, start[1][int(ptr[1]):int(ptr[2])])
    b.close()


def test_problems_are_independent_of_the_batch():
    """Each problem solved alone, and the batch in reversed order: the same bits as in the batch."""
    a, snap = default_run()
    cases, ptr = TC.WHOLE_RUN_CASES, a["point_ptr"]
    for k, case in enumerate(cases):
        one = TC.batch_arrays((case,))
        alone = snapshot(run_batch((case,), one))
        assert same_bits(problem_of(alone, one["point_ptr"], 0), problem_of(snap, ptr, k)), case
    rev = TC.batch_arrays(cases[::-1])
    back = snapshot(run_batch(cases[::-1], rev))
    for k, case in enumerate(cases):
        assert same_bits(problem_of(back, rev["point_ptr"], len(cases) - 1 - k), problem_of(snap, ptr, k)), case


def test_more_workgroups_than_compute_units():
    """300 problems (30 distinct, cycled): equal problems give equal bits wherever they run; one copy of each
    matches the oracle."""
    cases = TC.MANY_CASES * 10
    a = TC.batch_arrays(cases)
    snap, ptr = snapshot(run_batch(cases, a)), a["point_ptr"]
    m = len(TC.MANY_CASES)
    for k, case in enumerate(TC.MANY_CASES):
        check_whole_run(snap, ptr, k, case)
        first = problem_of(snap, ptr, k)
        for rep in range(1, 10):
            assert same_bits(problem_of(snap, ptr, k + rep * m), first), (case, rep)


@pytest.mark.parametrize("opts", [dict(huber_delta=0.0), dict(pixel_noise=2.0), dict(user_lambda_init=0.0)],
                         ids=["no_kernel", "pixel_noise_2", "tau_rule"])
def test_options(opts):
    a, _ = default_run()
    snap = snapshot(run_batch(TC.WHOLE_RUN_CASES, a, **opts))
    for k, case in enumerate(TC.WHOLE_RUN_CASES):
        check_whole_run(snap, a["point_ptr"], k, case, tuple(opts.items()))
        if opts.get("user_lambda_init") == 0.0:  # computeLambdaInit: tau * max diag(H) over camera 1 and the points
            P = TC.oracle_problem(TC.make_case(*case), TC.merged(**opts))
            H = P.system()[0]
            want = TC.DEFAULTS["tau"] * float(np.abs(H.diagonal()[6:]).max())
            assert abs(snap["lambda_init"][k] - want) <= 1e-12 * want, (case, snap["lambda_init"][k], want)


def test_one_trial_terminates_after_one_iteration():
    a, _ = default_run()
    b = run_batch(TC.WHOLE_RUN_CASES, a, max_trials=1)
    assert list(b.num_iterations()) == [1] * len(TC.WHOLE_RUN_CASES)
    assert all(b.stats(k)[0]["trials"] == 1 for k in range(len(TC.WHOLE_RUN_CASES)))


def test_inputs_stay_and_runs_repeat():
    a, snap = default_run()
    mine = {k: np.array(v) for k, v in a.items()}
    mine["cam0"][:, 4:] = [0.02, -0.01, 0.03]  # a fixed camera that is not the identity, its quaternion not quite
    mine["cam0"][:, :4] = [0.0, 0.006, 0.0, 0.99998]  # of unit length: returned as given
    keep = {k: v.copy() for k, v in mine.items()}
    b = L.TwoViewBatch()
    b.set_problems(**mine)
    assert b.optimize() == len(TC.WHOLE_RUN_CASES)
    first = snapshot(b)
    assert first["cam0"].tobytes() == keep["cam0"].tobytes()
    assert all(mine[k].tobytes() == keep[k].tobytes() for k in mine)
    b.set_problems(**mine)
    assert b.optimize() == len(TC.WHOLE_RUN_CASES)
    again = snapshot(b)
    for k in range(len(TC.WHOLE_RUN_CASES)):
        assert same_bits(problem_of(again, mine["point_ptr"], k), problem_of(first, mine["point_ptr"], k))
    # and the identity camera 0 of the shared run came back as given
    assert snap["cam0"].tobytes() == a["cam0"].tobytes()


def test_existing_bundle_adjuster_is_unchanged_after_a_batch_run():
    """The shared arithmetic header and the device-memory cache serve both paths: after a batch run in this
    process, BundleAdjuster still reproduces the oracle on a tests/test_ba.py problem."""
    import test_ba as TB
    default_run()
    P, _ = TB.synthetic_problem(n_cams=10, n_points=350, seed=2)
    b = TB.gpu_problem(P)
    c0 = b.chi2()
    assert abs(c0 - P.chi2()) <= 1e-12 * c0
    n = b.optimize(4)
    tr = P.optimize(4)
    assert n == len(tr)
    for s, t in zip(b.stats(), tr):
        assert s["trials"] == t["trials"] and abs(s["chi2_after"] - t["chi2"]) <= 1e-6 * t["chi2"]
    assert TB.quat_dist(b.cameras()[:, :4], P.cams[:, :4]) < 1e-7
    assert np.abs(b.cameras()[:, 4:] - P.cams[:, 4:]).max() < 1e-6


def test_cxx_helper_conformance(tmp_path):
    """include/sim3opt_two_view.hpp: the whole-run cases added as BAOptimize takes them, refined by one
    optimize(), against the oracle's values this test writes to a file."""
    import test_two_view_batch as TH
    exe = TH.compile_conformance(tmp_path)
    path = str(tmp_path / "cases.txt")
    TH.write_conformance_file(path, TC.WHOLE_RUN_CASES)
    r = subprocess.run([exe, "run", path], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 failed" in r.stdout, r.stdout + r.stderr
    assert os.path.getsize(path) > 0
