"""GPU tests (-m gpu) of the batched two-view refinement's passes as operators: one LM trial of
sim3opt_amd/csrc/ba_batch.hip -- the linearisation, the point blocks and their damped inverses, Z, the sums over the
four wavefronts, the reduced 6 x 6 system and its Cholesky step, the exp-map update, the back-substitution, the
trial's chi2 and the scale term -- read out of the device (lib.TwoViewBatch.debug_trial; the read-out kernel inlines the device
functions the LM loop runs) and compared with tests/ba_ref.py in long double.  An LM loop forgives a slightly wrong g, a
wavefront's partial lost from a sum or a quaternion branch no camera visits; these tests do not:
tests/test_two_view_batch.py shows without a GPU that each such defect misses a tolerance used here by 1e4 or more.

The tolerances are tests/two_view_checks.py's (derived: gamma(k) x the expression with absolute values; measured: 32 x
|float64 restatement - long double|, floored at 4u); every test prints error / tolerance per quantity (-s), DESIGN.md
records the table.  The cases are tests/two_view_cases.py's: READOUT_CASES (every size at which the 256-thread stride, a
wavefront or the four-wavefront sum changes what runs) and BRANCH_CASES (camera 1 on every branch of Eigen's matrix ->
quaternion rule), the branch of every camera asserted here on the host."""
import ctypes

import numpy as np
import pytest

import amg_ref as R
import ba_ref as BR
import two_view_cases as TC
import two_view_checks as CK
from sim3opt_amd import lib as L
from test_gpu_two_view_batch import problem_of, same_bits, snapshot

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not R.longdouble_ok(), reason="np.longdouble has no 64-bit mantissa here")]

U = R.U
DBL_MAX = np.finfo(np.float64).max
LAM0 = TC.DEFAULTS["user_lambda_init"]
BOUNDED = ("H_pp", "b_p", "A1", "B1", "es1", "Hpp_inv", "Z", "AtA", "b_c", "ZY", "Zb", "S", "g", "maxdiag", "chi2",
           "active_chi2", "dx_c", "cam_q", "cam_t", "trial_points", "chi2_new", "scale")
POINT_KEYS = tuple(L.TwoViewBatch.TRIAL_POINT_ROWS)
PROBLEM_KEYS = tuple(L.TwoViewBatch.TRIAL_PROBLEM_ROWS)


def new_batch(cases, **opts):
    a = TC.batch_arrays(cases)
    b = L.TwoViewBatch(**opts)
    b.set_problems(**a)
    return a, b


_shared = {}


def shared(name):
    """(arrays, handle) of the read-out batch / the branch batch: made once, never optimised."""
    if name not in _shared:
        _shared[name] = new_batch(dict(sizes=TC.READOUT_CASES, branches=TC.BRANCH_CASES)[name])
    return _shared[name]


@pytest.fixture(scope="module", autouse=True)
def close_shared_handles():
    yield
    while _shared:
        _shared.popitem()[1][1].close()


def checked(what, a, b, d, lam, dx_c=None):
    """CK.ratios of the read-out d at the handle's estimate, printed; asserts every quantity within its tolerance."""
    # (the kernel computes with the normalised camera 0; the handle returns it as given)
    r = CK.ratios(d, dict(a, cam0=TC.normalised(a["cam0"])), b.cameras()[1], b.points(), lam, dx_c)
    print(f"[2v-op] {what}: error / tolerance " + ", ".join(f"{k} {r[k]:.3f}" for k in BOUNDED if k in r))
    bad = {k: r[k] for k in BOUNDED if k in r and not r[k] <= 1}
    assert not bad, (what, bad)
    return r


def share(d, ptr, k):
    """Problem k's share of a read-out, as arrays to compare bit for bit."""
    lo, hi = int(ptr[k]), int(ptr[k + 1])
    return ([np.ascontiguousarray(d[q][lo:hi]) for q in POINT_KEYS] +
            [np.ascontiguousarray(d[q][k:k + 1]) for q in PROBLEM_KEYS])


# ------------------------------------------------------------------------------------------------ bounds
@pytest.mark.parametrize("rule", ["lambda_50", "tau_maxdiag"])
def test_every_size_within_the_bounds(rule):
    """The ragged batch of READOUT_CASES (1 ... 1047 points: 193 is the first size at which wavefront 3 owns a point,
    257 / 513 / 1047 take two, three and five passes of the stride), at lambda = 50 and at computeLambdaInit's tau x
    the read-out's own maxdiag: every quantity of two_view_checks within its tolerance."""
    a, b = shared("sizes")
    n = b.dims()[0]
    lam = np.full(n, LAM0)
    if rule == "tau_maxdiag":
        lam = TC.DEFAULTS["tau"] * b.debug_trial(lam)["maxdiag"]
    d = b.debug_trial(lam)
    sizes = np.diff(a["point_ptr"])
    print(f"[2v-op] {rule}: lambda {lam.min():.3e} ... {lam.max():.3e}, fail {d['fail'].astype(int).tolist()}")
    assert not d["fail"][sizes >= 5].any()  # (one or two points leave S singular up to lambda)
    checked(rule, a, b, d, lam)


def test_maximum_diagonal_entry_held_by_the_fourth_wavefront():
    """two_view_cases.near_point_case between two other problems: the largest diagonal entry of its Hessian is the H_pp
    of point 192 -- the fourth wavefront's only point -- and more than twice the camera's largest and every other
    point's (asserted on the device's rows), so a wg_max that lost that wavefront, or a maximum over the camera alone,
    would show.  The read-out's maxdiag is that entry bit for bit, every other quantity is within its tolerance, and
    optimize() under the tau rule starts from tau x it."""
    cs = [TC.make_case(5, 13), TC.near_point_case(), TC.make_case(257, 19)]
    a = TC.arrays_of(cs)
    b = L.TwoViewBatch(user_lambda_init=0.0, max_iters=1)
    b.set_problems(**a)
    lam = np.full(3, LAM0)
    d = b.debug_trial(lam)
    lo, hi = int(a["point_ptr"][1]), int(a["point_ptr"][2])
    hpp = d["H_pp"][lo:hi][:, [0, 3, 5]].max(1)
    assert int(hpp.argmax()) == TC.NEAR_POINT[2] >= 192
    assert hpp.max() > 2 * CK.tri21(d["AtA"][1]).diagonal().max() and hpp.max() > 2 * np.delete(hpp, hpp.argmax()).max()
    assert d["maxdiag"][1] == hpp.max()
    checked("near point", a, b, d, lam)
    assert b.optimize() == 3
    assert np.array_equal(b.lambda_init(), TC.DEFAULTS["tau"] * d["maxdiag"])
    b.close()


def test_supplied_steps_on_every_branch():
    """BRANCH_CASES at lambda = 50 with the camera steps of two_view_cases.trial_steps: camera 1 starts on the x, x, y,
    y, z, z and trace branch (asserted on the device's cameras); omega = 0 and |omega| = 0.99e-5 take SE3Quat::exp's
    small-angle branch, 1.01e-5, 0.3 and pi - 1e-3 the other; carry_next / carry_prev land on the neighbouring branch.
    Every quantity within its tolerance; the Cholesky's step is reported whatever step is supplied."""
    a, b = shared("branches")
    n = b.dims()[0]
    want = np.array([TC.GAUGE_BRANCH[g] for g in TC.GAUGES])
    c0, c1 = b.cameras()
    assert np.array_equal(BR.quat_branch(c1), want)
    assert np.array_equal(c1, TC.normalised(a["cam1"]))  # (the host's normalisation, restated bit for bit)
    assert not (np.abs(c0 - [0, 0, 0, 1, 0, 0, 0]) < 0.01).all(1).any()  # camera 0 is nowhere near the identity
    assert {bool(w > 0) for w in c1[:, 3]} == {True, False}
    lam = np.full(n, LAM0)
    plain = b.debug_trial(lam)
    checked("branches, own step", a, b, plain, lam)
    landed = set()
    for name, step in TC.trial_steps(c1).items():
        d = b.debug_trial(lam, step)
        r = checked(f"branches, {name}", a, b, d, lam, step)
        assert np.array_equal(d["dx_c"], plain["dx_c"]) and not d["fail"].any()
        assert r["small"].all() if name in ("omega0", "below") else not r["small"].any(), name
        if name in ("omega0", "below", "above"):
            assert np.array_equal(r["branch"], want), name
        if name.startswith("carry"):
            assert np.array_equal(r["branch"], (want + (1 if name == "carry_next" else -1)) % 4), (name, r["branch"])
        landed |= {(int(x), int(y)) for x, y in zip(want, r["branch"])}
        assert not np.array_equal(d["cam"], plain["cam"])  # the supplied step is the one used
    assert {(x, (x + s) % 4) for x in range(4) for s in (1, 3)} <= landed


def test_zero_step_leaves_the_camera():
    """dx_c = 0 at lambda = 50: exp(0) = I exactly, so the translation comes back bit for bit and the quaternion goes
    through quat -> R -> quat and one normalisation.  With |q| = 1: an entry of R carries at most 4u, the branch's
    square root and quotients 3u more on entries <= 1, the normalisation 2u: within 16u, on every branch."""
    a, b = shared("branches")
    n = b.dims()[0]
    d = b.debug_trial(np.full(n, LAM0), np.zeros((n, 6)))
    c1 = b.cameras()[1]
    assert np.array_equal(d["cam"][:, 4:], c1[:, 4:])
    print(f"[2v-op] zero step: quaternion off by {np.abs(d['cam'][:, :4] - c1[:, :4]).max() / U:.2f} u")
    assert np.abs(d["cam"][:, :4] - c1[:, :4]).max() <= 16 * U
    assert np.abs(d["dx_c"]).min(1).max() > 0


# ------------------------------------------------------------------------------------------------ exact
def test_readout_repeats_and_does_not_depend_on_the_batch():
    """The read-out twice: the same bytes.  A problem alone, first and last in a batch: the same bytes (its rows sit at
    another offset of another stride each time)."""
    a, b = shared("sizes")
    n = b.dims()[0]
    lam = np.linspace(20.0, 80.0, n)
    d1, d2 = b.debug_trial(lam), b.debug_trial(lam)
    assert all(d1[k].tobytes() == d2[k].tobytes() for k in d1)
    for k in (5, 6, 9, 11):  # 65, 193, 257 and 1047 points
        case = TC.READOUT_CASES[k]
        ref = share(d1, a["point_ptr"], k)
        others = tuple(c for c in TC.READOUT_CASES[:6] if c != case)
        for cases, pos in (((case,), 0), ((case,) + others, 0), (others + (case,), len(others))):
            a2, b2 = new_batch(cases)
            l2 = np.full(len(cases), 33.0)
            l2[pos] = lam[k]
            assert same_bits(share(b2.debug_trial(l2), a2["point_ptr"], pos), ref), (case, len(cases), pos)
            b2.close()


def test_readout_changes_nothing():
    """optimize() after read-outs (before the first run and between two runs, with and without a supplied step, with a
    failing lambda) gives the bytes it gives without them; the estimates, the last run's results and the device memory
    in use are what they were around every read-out."""
    cases = TC.WHOLE_RUN_CASES[:4] + TC.BRANCH_CASES[:2]
    a, plain = new_batch(cases, max_iters=4)
    _, probed = new_batch(cases, max_iters=4)
    n = len(cases)

    def readouts():
        before = (probed.cameras(), probed.points(), probed.num_iterations(), L.device_memory_in_use())
        probed.debug_trial(np.full(n, 7.0))
        probed.debug_trial(np.full(n, LAM0), 0.1 * np.ones((n, 6)))
        assert probed.debug_trial(np.full(n, -1e12))["fail"].all()
        after = (probed.cameras(), probed.points(), probed.num_iterations(), L.device_memory_in_use())
        assert before[3] == after[3]
        assert all(np.array_equal(x, y) for x, y in zip(before[0] + before[1:3], after[0] + after[1:3]))

    readouts()
    with pytest.raises(L.Sim3OptError) as e:  # still no run: the read-out did not pretend one
        probed.chi2()
    assert e.value.code == L.ERR_STATE
    for _ in range(2):  # (the second optimize continues from the first)
        assert plain.optimize() == probed.optimize() == n
        s0 = snapshot(probed)
        readouts()
        s1 = snapshot(probed)
        for k in range(n):
            assert same_bits(problem_of(s0, a["point_ptr"], k), problem_of(s1, a["point_ptr"], k))
            assert same_bits(problem_of(snapshot(plain), a["point_ptr"], k), problem_of(s1, a["point_ptr"], k))
    plain.close()
    probed.close()


def test_one_trial_of_optimize_is_the_readout():
    """optimize(max_iters = 1, max_trials = 1) against the read-out at lambda_0 = 50 of the same start, bit for bit:
    chi2_before, and rho as LmDamping::update forms it from the read-out's chi2, chi2_new and scale; where the step is
    accepted (rho > 0) the camera, the points and chi2_after; where it is not, the start."""
    cases = TC.READOUT_CASES + TC.BRANCH_CASES
    a, b = new_batch(cases, max_iters=1, max_trials=1)
    n, ptr = len(cases), a["point_ptr"]
    start = (b.cameras()[1], b.points())
    d = b.debug_trial(np.full(n, LAM0))
    assert not d["fail"].any()
    assert b.optimize() == n
    cam1, pts = b.cameras()[1], b.points()
    accepted = 0
    for k in range(n):
        st, sl = b.stats(k), slice(int(ptr[k]), int(ptr[k + 1]))
        assert len(st) == 1 and st[0]["trials"] == 1
        assert st[0]["chi2_before"] == d["chi2"][k]
        rho = (d["chi2"][k] - d["chi2_new"][k]) / (d["scale"][k] + 1e-3)
        assert st[0]["rho"] == rho, (cases[k], st[0]["rho"], rho)
        if rho > 0:
            accepted += 1
            assert st[0]["chi2_after"] == d["chi2_new"][k]
            assert np.array_equal(cam1[k], d["cam"][k]) and np.array_equal(pts[sl], d["trial_points"][sl])
        else:
            assert st[0]["chi2_after"] == d["chi2"][k]
            assert np.array_equal(cam1[k], start[0][k]) and np.array_equal(pts[sl], start[1][sl])
    assert accepted >= n - 2
    b.close()


def test_negative_damping_fails_every_trial_and_nothing_else():
    """lambda = -10 x the read-out's own maxdiag: S's first pivot is lambda + (sum A_1^T A_1)_00 - (sum Z Y^T)_00 with
    the last term at most a ninth of the second and the second at most maxdiag, so it is negative: `fail` on every
    problem, the trial camera is the current one bit for bit, the trial's chi2 DBL_MAX, the scale 0.  The handle keeps working,
    and optimize() gives the bytes of a fresh handle."""
    cases = TC.READOUT_CASES[2:8] + TC.BRANCH_CASES[:3]
    a, b = new_batch(cases)
    n = len(cases)
    md = b.debug_trial(np.full(n, 1.0))["maxdiag"]
    d = b.debug_trial(-10.0 * md)
    assert d["fail"].all()
    assert (np.stack([CK.tri21(s).diagonal() for s in d["S"]])[:, 0] < 0).all()
    assert np.array_equal(d["cam"], b.cameras()[1])
    assert (d["chi2_new"] == DBL_MAX).all() and (d["scale"] == 0).all() and (d["trial_points"] == 0).all()
    again = b.debug_trial(np.full(n, LAM0))
    assert not again["fail"].any()
    _, fresh = new_batch(cases)
    assert b.optimize() == fresh.optimize() == n
    s0, s1 = snapshot(b), snapshot(fresh)
    for k in range(n):
        assert same_bits(problem_of(s0, a["point_ptr"], k), problem_of(s1, a["point_ptr"], k))
    b.close()
    fresh.close()


# ------------------------------------------------------------------------------------------------ the rejected path
def rejecting_iterations():
    """(case, iteration, trials, rho of the last trial) of every default whole run's iteration with a rejected trial."""
    out = []
    for case in TC.WHOLE_RUN_CASES:
        for i, t in enumerate(TC.reference(*case)["trace"]):
            if t["trials"] > 1:
                out.append((case, i, t["trials"], t["rho"]))
    return out


def test_rejected_trials_replayed_through_the_readout():
    """An iteration in which the oracle rejects trials (the first such of up to three cases): optimize(max_iters = k)
    reaches it, then the read-out at lambda, 2 lambda, 8 lambda, ... as LmDamping raises it.  The same H_pp and b_p are
    re-eliminated at each: every quantity within its tolerance each time, and chi_old - chi_new has the oracle's sign
    at every trial (negative until the last, then the sign of the recorded rho)."""
    todo, seen = [], set()
    for case, i, q, rho in rejecting_iterations():
        if case not in seen and len(todo) < 3:
            seen.add(case)
            todo.append((case, i, q, rho))
    assert todo
    for case, it, q, rho in todo:
        a, b = new_batch((case,), max_iters=max(it, 1))
        lam = LAM0
        if it > 0:
            assert b.optimize() == 1 and int(b.num_iterations()[0]) == it
            lam = b.stats(0)[-1]["lambda_"]
        ni = 2.0
        for j in range(q):
            d = b.debug_trial(np.array([lam]))
            assert not d["fail"][0]
            checked(f"case {case} iteration {it} trial {j} (lambda {lam:.3e})", a, b, d, np.array([lam]))
            gain = d["chi2"][0] - d["chi2_new"][0]
            assert d["scale"][0] + 1e-3 > 0
            assert np.sign(gain) == (-1.0 if j < q - 1 else np.sign(rho)), (case, it, j, gain)
            lam, ni = lam * ni, ni * 2.0
        b.close()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_handle():
    lib = L.load()
    dp = ctypes.POINTER(ctypes.c_double)
    p = lambda x: x.ctypes.data_as(dp)
    b = L.TwoViewBatch()
    one, buf = np.ones(1), np.zeros(100)
    assert lib.sim3opt_ba_batch_debug_trial(b._b, p(one), None, None, p(buf)) == L.ERR_STATE
    assert b"no problems" in lib.sim3opt_ba_batch_last_error(b._b)
    b.close()
    a, b = new_batch(((5, 13), (2, 12)))
    n, t = b.dims()
    before = (b.cameras(), b.points(), L.device_memory_in_use())
    lam, rows, prob, step = np.full(n, LAM0), np.zeros((56, t)), np.zeros((n, 100)), np.zeros((n, 6))
    f = lib.sim3opt_ba_batch_debug_trial
    assert f(b._b, None, None, p(rows), p(prob)) == L.ERR_ARG
    assert f(b._b, p(lam), None, None, None) == L.ERR_ARG
    for bad in (np.nan, np.inf, -np.inf):
        x = lam.copy()
        x[1] = bad
        assert f(b._b, p(x), None, p(rows), p(prob)) == L.ERR_ARG
        assert b"lambda" in lib.sim3opt_ba_batch_last_error(b._b)
        s = step.copy()
        s[1, 4] = bad
        assert f(b._b, p(lam), p(s), p(rows), p(prob)) == L.ERR_ARG
        assert b"step" in lib.sim3opt_ba_batch_last_error(b._b)
    assert f(None, p(lam), None, p(rows), p(prob)) == L.ERR_ARG
    after = (b.cameras(), b.points(), L.device_memory_in_use())
    assert before[2] == after[2] and np.array_equal(before[1], after[1])
    assert all(np.array_equal(x, y) for x, y in zip(before[0], after[0]))
    assert f(b._b, p(lam), None, p(rows), None) == L.OK and f(b._b, p(-lam), p(step), None, p(prob)) == L.OK
    assert np.array_equal(b.debug_trial(lam)["b_p"], np.ascontiguousarray(rows[6:9].T))
    b.close()
