"""CPU side of the batched two-view refinement (sim3opt_ba_batch, include/sim3opt.h): the cases the GPU tests
compare traces on are stable, every argument error is refused with nothing changed, the library says so when there
is no GPU, the C++ helper's conformance program passes its host part, and both builds export the new symbols."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import two_view_cases as TC
from conftest import gpu_available
from sim3opt_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH_SYMBOLS = [s for s in L.SYMBOLS if s.startswith("sim3opt_ba_batch_")]


def trials(ref):
    return [t["trials"] for t in ref["trace"]]


def test_trace_cases_are_stable_and_reject_trials():
    """Every (case, option set) the GPU tests compare whole traces on: a relative 1e-13 perturbation of the inputs
    leaves the oracle's trial counts and iteration count as they are -- so a kernel that sums in another order may
    be held to equal trial counts -- and moves its per-observation chi2 by at most 2e-8 relative.  The set exercises
    the rejection branch: some iteration takes more than one trial, some run ends early on max_trials."""
    runs = [(c, o) for o in TC.OPTION_SETS for c in TC.WHOLE_RUN_CASES] + [(c, {}) for c in TC.MANY_CASES]
    rejected = early = 0
    for case, o in runs:
        assert case[0] >= 5  # smaller problems reach chi2 = 0: their traces are rounding noise
        ref = TC.reference(*case, tuple(sorted(o.items())))
        moved = TC.run_oracle(TC.perturbed(TC.make_case(*case)), TC.merged(**o))
        assert trials(ref) == trials(moved), (case, o, trials(ref), trials(moved))
        # ... and the reference's per-observation chi2 by less than a fifth of the 1e-7 it is compared at
        rel = np.abs(moved["edge_chi2"] - ref["edge_chi2"]) / ref["edge_chi2"]
        assert rel.max() <= 2e-8, (case, o, rel.max())
        rejected += sum(t > 1 for t in trials(ref))
        early += len(ref["trace"]) < TC.DEFAULTS["max_iters"]
        # no observation sits on the outlier threshold
        thr = TC.DEFAULTS["outlier_chi2"]
        assert np.abs(ref["edge_chi2"] - thr).min() > 1e-6 * thr, (case, o)
    assert rejected >= 1 and early >= 1


def test_branch_cases_sit_on_their_branches_and_are_the_base_case():
    """BRANCH_CASES: camera 1 starts and ends on the x, x, y, y, z, z and trace branch of Eigen's matrix -> quaternion
    rule, with w of both signs, camera 0 away from the identity; the oracle takes one trial in each of its ten
    iterations, also under the 1e-13 perturbation, whose effect on every observation's chi2 stays below 2e-8; and the
    final chi2 is the base case's to 1e-14 relative: the same problem in another gauge."""
    import ba_ref as BR
    base = TC.reference(*TC.BRANCH_BASE)
    signs = set()
    for case in TC.BRANCH_CASES:
        c, ref = TC.make_case(*case), TC.reference(*case)
        want = TC.GAUGE_BRANCH[case[2]]
        assert list(BR.quat_branch(np.stack([c["cam1"], ref["cam1"]]))) == [want, want], case
        assert np.abs(c["cam0"] - [0, 0, 0, 1, 0, 0, 0]).max() > 0.5
        signs |= {(want, bool(c["cam1"][3] > 0)), (want, bool(ref["cam1"][3] > 0))}
        moved = TC.run_oracle(TC.perturbed(c), TC.DEFAULTS)
        assert trials(ref) == trials(moved) == [1] * 10, case
        assert (np.abs(moved["edge_chi2"] - ref["edge_chi2"]) <= 2e-8 * ref["edge_chi2"]).all(), case
        assert abs(ref["trace"][-1]["chi2"] - base["trace"][-1]["chi2"]) <= 1e-14 * base["trace"][-1]["chi2"], case
    assert {(b, s) for b in range(3) for s in (True, False)} <= signs and (3, True) in signs


def test_continued_runs_are_stable():
    """optimize(4) then optimize(6) without set_problems in between, each restarting at lambda_0 = 50 and ni = 2: the
    oracle's pair of traces keeps its trial counts under the 1e-13 perturbation, and its per-observation chi2 moves by
    at most 2e-8 relative after either call."""
    for case in TC.CONTINUED_CASES:
        ref = TC.continued_reference(*case)
        moved = TC.run_oracle_continued(TC.perturbed(TC.make_case(*case)), TC.DEFAULTS, TC.CONTINUED_ITERS)
        assert [len(r["trace"]) for r in ref] == list(TC.CONTINUED_ITERS), case
        for r, m in zip(ref, moved):
            assert trials(r) == trials(m), case
            assert (np.abs(m["edge_chi2"] - r["edge_chi2"]) <= 2e-8 * r["edge_chi2"]).all(), case


def test_trial_steps_reach_their_branches():
    """two_view_cases.trial_steps on the branch cases' start cameras (no device): the exp map's branch of every step and
    the quaternion branch every camera lands on, in float64 and in long double alike."""
    import ba_ref as BR
    cam1 = np.stack([TC.make_case(*c)["cam1"] for c in TC.BRANCH_CASES])
    want = np.array([TC.GAUGE_BRANCH[g] for g in TC.GAUGES])
    n = cam1.shape[0]
    for name, step in TC.trial_steps(cam1).items():
        th = np.linalg.norm(step[:, :3], axis=1)
        up = [BR.update(cam1, np.zeros((1, 3)), step, np.zeros((1, 3)), np.zeros(n, dtype=bool), dt)
              for dt in (np.float64, BR.LD)]
        assert np.array_equal(up[0]["branch"], up[1]["branch"]) and np.array_equal(up[0]["small"], up[1]["small"])
        assert np.array_equal(up[0]["small"], th < 1e-5)
        expect = dict(omega0=0.0, below=0.99e-5, above=1.01e-5, mid=0.3, near_pi=np.pi - 1e-3).get(name)
        if expect is not None:
            assert np.abs(th - expect).max() <= 1e-15 * max(expect, 1e-5), name
        if name.startswith("carry"):
            assert np.array_equal(up[0]["branch"], (want + (1 if name == "carry_next" else -1)) % 4), name


_restated = {}


def restated(mut=None, step=None):
    """The float64 restatement of the read-out (near_point_case, READOUT_CASES and BRANCH_CASES as one batch, lambda =
    50) with one seeded defect, in the layout of debug_trial, and what two_view_checks makes of it."""
    import ba_ref as BR
    import two_view_checks as CK
    if not _restated:
        a = TC.arrays_of([TC.near_point_case()] + [TC.make_case(*c) for c in TC.READOUT_CASES + TC.BRANCH_CASES])
        n = a["point_ptr"].shape[0] - 1
        s = TC.trial_steps(a["cam1"][-len(TC.BRANCH_CASES):])
        # (the other problems take the step of the first branch case)
        steps = {k: np.concatenate([np.tile(v[:1], (n - v.shape[0], 1)), v]) for k, v in s.items()}
        _restated.update(a=a, P=TC.ref_batch(a), lam=np.full(n, TC.DEFAULTS["user_lambda_init"]), steps=steps)
    a, P, lam = _restated["a"], _restated["P"], _restated["lam"]
    dx = None if step is None else _restated["steps"][step]
    d = CK.as_readout(BR.two_view_trial(P, lam, np.float64, dx_c=dx, mut=mut))
    return CK.ratios(d, a, a["cam1"], a["points"], lam, dx)


def test_restatement_passes_the_readout_checks():
    """The float64 restatement, which sums in another order than the device and inverts by LAPACK, is within every
    tolerance of tests/two_view_checks.py: the tolerances do not depend on how the sums are ordered."""
    for step in (None, "below", "carry_next"):
        r = restated(step=step)
        assert all(v <= 1 for k, v in r.items() if k not in ("branch", "small")), (step, r)


def test_exact_quantities_fail_on_any_difference():
    """What two_view_checks holds to "bit for bit" misses by an infinite factor, not by 1, as soon as it differs: the
    maximum diagonal entry moved by one ulp either way, on one problem.  And the near-point case is what it is for:
    the maximum of its problem is the H_pp of point 192, which the fourth wavefront owns, not the camera's diagonal."""
    import ba_ref as BR
    import two_view_checks as CK
    restated()
    a, P, lam = _restated["a"], _restated["P"], _restated["lam"]
    t = BR.two_view_trial(P, lam, np.float64)
    hpp = t["rows"]["H"][:TC.NEAR_POINT[0]].diagonal(0, 1, 2).max(1)
    assert int(hpp.argmax()) == TC.NEAR_POINT[2] >= 192 and t["maxdiag"][0] == hpp.max()
    assert hpp.max() > 2 * t["sums"][0]["AtA"].diagonal().max() and hpp.max() > 2 * np.delete(hpp, hpp.argmax()).max()
    d = CK.as_readout(t)
    assert CK.ratios(d, a, a["cam1"], a["points"], lam)["maxdiag"] == 0
    for k, to in ((0, np.inf), (7, 0.0)):
        bad = dict(d, maxdiag=d["maxdiag"].copy())
        bad["maxdiag"][k] = np.nextafter(bad["maxdiag"][k], to)
        assert CK.ratios(bad, a, a["cam1"], a["points"], lam)["maxdiag"] == np.inf


# defect -> (supplied step, the quantities it must move by 1e4 x their tolerance or more)
SEEDED = dict(wave3_drop=(None, ("AtA", "b_c", "ZY", "Zb", "chi2", "active_chi2", "chi2_new", "scale")),
              p256_as_0=(None, ("AtA", "b_c", "ZY", "Zb", "chi2", "chi2_new", "scale")),
              prev_offset=(None, ("AtA", "b_c", "ZY", "Zb", "chi2", "chi2_new", "scale")),
              damp_none=(None, ("Hpp_inv",)), damp_offdiag=(None, ("Hpp_inv",)), hinv_other_lambda=(None, ("Hpp_inv",)),
              no_cam0=(None, ("H_pp", "b_p")), cam0_in_AtA=(None, ("AtA", "S")),
              huber_swapped=(None, ("A1", "B1", "es1")), g_no_Zbp=(None, ("g",)), backsub_ZT=(None, ("trial_points",)),
              scale_no_cam=(None, ("scale",)), maxdiag_no_cam=(None, ("maxdiag",)),
              maxdiag_wave3=(None, ("maxdiag",)), V_half=("below", ("cam_t",)), quat_jl_swap=("mid", ("cam_q",)))


@pytest.mark.parametrize("mut", sorted(SEEDED))
def test_seeded_defect_misses_its_tolerance_by_1e4(mut):
    """Each defect an LM trace forgives (tests/ba_ref.py, TWO_VIEW_MUTATIONS), seeded into the restatement: the
    quantities it touches miss the tolerance the device is held to by a factor of 1e4 or more -- the project's rule
    for an operator test (tests/test_ba_ref.py)."""
    import ba_ref as BR
    assert sorted(SEEDED) == sorted(BR.TWO_VIEW_MUTATIONS)
    step, touched = SEEDED[mut]
    r = restated(mut, step)
    assert all(r[k] >= 1e4 for k in touched), (mut, {k: r[k] for k in touched})


def test_damping_rule_on_a_trial_that_cannot_be_evaluated(tmp_path):
    """lm_damping.hpp's own statements, compiled into a host program, on the chi2 sequences of a problem whose sums are
    not finite (tests/test_gpu_two_view_batch.py, the degenerate problem): the trial counts and the iteration count
    the kernel must report for it."""
    for got, want in ((damping_trace(tmp_path, "nan", "nan"), DAMPING_NAN),
                      (damping_trace(tmp_path, "inf", "max"), DAMPING_INF_FAIL)):
        assert got[:2] == want[:2] and abs(got[2] - want[2]) <= 1e-14 * want[2], (got, want)


# (iterations, trials of each, final lambda / lambda_0) of a run of 10 iterations x 5 trials whose current chi2 is
# always `old` and whose every trial gives `new` with scale 0.  NaN: rho is NaN, neither > 0 nor < 0: the trial is
# rejected and the iteration ends after it; rho == 0 is false, lambda stays finite (50 x 2^55): all 10 iterations run.
# +inf against DBL_MAX (the reduced system is not finite, its Cholesky fails): rho = +inf, finite chi_new: accepted,
# lambda / 3 each time.
DAMPING_NAN = (10, [1] * 10, 2.0 ** 55)
DAMPING_INF_FAIL = (10, [1] * 10, 3.0 ** -10)


def damping_trace(tmp_path, old, new):
    src, exe = str(tmp_path / "damping.cpp"), str(tmp_path / "damping")
    with open(src, "w") as f:
        f.write('#include <cfloat>\n#include <cstdio>\n#include <cstring>\n#include <limits>\n'
                '#include "lm_damping.hpp"\n'
                'static double val(const char* s) {\n'
                '  if (!std::strcmp(s, "nan")) return std::numeric_limits<double>::quiet_NaN();\n'
                '  if (!std::strcmp(s, "inf")) return std::numeric_limits<double>::infinity();\n'
                '  return DBL_MAX;\n}\n'
                'int main(int, char** v) {\n'
                '  const double chi_old = val(v[1]), chi_new = val(v[2]);\n'
                '  sim3opt::LmDamping d;\n  d.start(50.0, 1e-5, 0.0);\n  int iters = 0;\n'
                '  for (int it = 0; it < 10; ++it) {\n    double rho = 0.0, cur = chi_old;\n    int q = 0;\n'
                '    do {\n      if (d.update(cur, chi_new, 0.0, 1.0 / 3.0, 2.0 / 3.0, rho)) cur = chi_new;\n'
                '      ++q;\n    } while (rho < 0 && q < 5);\n'
                '    std::printf("%d ", q);\n    ++iters;\n    if (d.terminate(q, 5, rho)) break;\n  }\n'
                '  std::printf("\\n%d %.17g\\n", iters, d.lambda / 50.0);\n  return 0;\n}\n')
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "sim3opt_amd", "csrc"), src, "-o",
                           exe])
    out = subprocess.run([exe, old, new], capture_output=True, text=True, check=True).stdout.split("\n")
    return int(out[1].split()[0]), [int(x) for x in out[0].split()], float(out[1].split()[1])


def small_batch():
    a = TC.batch_arrays(((5, 13), (1, 11), (2, 12)))
    b = L.TwoViewBatch()
    b.set_problems(**a)
    return a, b


def state(b):
    return b.dims(), b.cameras(), b.points()


def same_state(x, y):
    return x[0] == y[0] and np.array_equal(x[1][0], y[1][0]) and np.array_equal(x[1][1], y[1][1]) and \
        np.array_equal(x[2], y[2])


def test_defaults_are_the_detectors():
    o = L.BaBatchOptions()
    L.load().sim3opt_ba_batch_options_default(ctypes.byref(o))
    got = {k: getattr(o, k) for k, _ in L.BaBatchOptions._fields_}
    assert got == dict(TC.DEFAULTS, device=-1)


def test_set_problems_keeps_the_callers_numbers():
    a, b = small_batch()
    assert b.dims() == (3, 8)
    c0, c1 = b.cameras()
    assert np.array_equal(c0, a["cam0"]) and np.abs(c1 - a["cam1"]).max() < 1e-15  # (cam1: normalised)
    assert np.array_equal(b.points(), a["points"])
    with pytest.raises(L.Sim3OptError) as e:
        b.chi2()
    assert e.value.code == L.ERR_STATE
    assert list(b.num_iterations()) == [0, 0, 0] and b.stats(0) == []


@pytest.mark.parametrize("what", ["no_problem", "empty_problem", "not_monotone", "ptr0", "nan_point", "inf_uv0",
                                  "inf_uv1", "nan_cam0", "nan_cam1", "zero_quaternion", "focal"])
def test_set_problems_refuses_and_changes_nothing(what):
    a, b = small_batch()
    before = state(b)
    bad = {k: np.array(v) for k, v in a.items()}
    kw = {}
    if what == "no_problem":
        bad["point_ptr"] = np.array([0], dtype=np.int32)
        bad["cam0"], bad["cam1"] = bad["cam0"][:0], bad["cam1"][:0]
    elif what == "empty_problem":
        bad["point_ptr"] = np.array([0, 5, 5, 8], dtype=np.int32)
    elif what == "not_monotone":
        bad["point_ptr"] = np.array([0, 6, 5, 8], dtype=np.int32)
    elif what == "ptr0":
        bad["point_ptr"] = np.array([1, 5, 6, 8], dtype=np.int32)
    elif what == "nan_point":
        bad["points"][7, 1] = np.nan
    elif what == "inf_uv0":
        bad["uv0"][0, 0] = np.inf
    elif what == "inf_uv1":
        bad["uv1"][7, 1] = -np.inf
    elif what == "nan_cam0":
        bad["cam0"][2, 6] = np.nan
    elif what == "nan_cam1":
        bad["cam1"][1, 0] = np.nan
    elif what == "zero_quaternion":
        bad["cam1"][0, :4] = 0.0
    elif what == "focal":
        kw["focal"] = 0.0
    with pytest.raises(L.Sim3OptError) as e:
        b.set_problems(**bad, **kw)
    assert e.value.code == L.ERR_ARG and "ba_batch_set_problems" in str(e.value)
    assert same_state(before, state(b))


@pytest.mark.parametrize("kw", [dict(max_iters=0), dict(max_trials=0), dict(pixel_noise=0.0), dict(pixel_noise=-1.0),
                                dict(pixel_noise=float("nan")), dict(tau=0.0), dict(huber_delta=-1.0),
                                dict(user_lambda_init=float("inf"))])
def test_set_options_refuses_and_changes_nothing(kw):
    a, b = small_batch()
    before = state(b)
    with pytest.raises(L.Sim3OptError) as e:
        b.set_options(**kw)
    assert e.value.code == L.ERR_ARG
    assert same_state(before, state(b))
    b.set_options(max_iters=3)  # a good value is still taken
    assert same_state(before, state(b))


def test_optimize_without_problems_is_a_state_error():
    b = L.TwoViewBatch()
    with pytest.raises(L.Sim3OptError) as e:
        b.optimize()
    assert e.value.code == L.ERR_STATE


def test_fails_loudly_without_gpu():
    if gpu_available():
        pytest.skip("GPU present: covered by the gpu tests")
    a, b = small_batch()
    before = state(b)
    with pytest.raises(L.Sim3OptError) as e:
        b.optimize()
    assert e.value.code == L.ERR_NO_DEVICE and "no usable HIP device" in str(e.value)
    assert same_state(before, state(b))


def compile_conformance(tmp_path):
    exe = str(tmp_path / "two_view_conformance")
    libdir = os.path.join(ROOT, "sim3opt_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "two_view_conformance.cpp"), "-L" + libdir,
                           "-lsim3opt", "-Wl,-rpath," + libdir, "-o", exe])
    return exe


def write_conformance_file(path, cases):
    """The candidates of `cases` as BAOptimize takes them, each followed by the oracle's run of it."""
    with open(path, "w") as f:
        w = lambda *v: f.write(" ".join(repr(float(x)) if not isinstance(x, (int, np.integer)) else str(x)
                                        for x in v) + "\n")
        w(len(cases), TC.FOCAL, TC.CX, TC.CY)
        for c in cases:
            case, ref = TC.make_case(*c), TC.reference(*c)
            n = case["points"].shape[0]
            w(n, len(ref["trace"]))
            w(*TC.BO.quat_to_R(case["cam1"][:4]).ravel())
            w(*case["cam1"][4:])
            for i in range(n):
                w(*case["points"][i], *case["uv0"][i], *case["uv1"][i])
            w(*[int(t["trials"]) for t in ref["trace"]])
            w(*[t["chi2"] for t in ref["trace"]])
            w(*ref["cam1"][:4])
            w(*ref["cam1"][4:])
            for i in range(n):
                w(*ref["points"][i])
            w(int((ref["edge_chi2"] > TC.DEFAULTS["outlier_chi2"]).sum()))


def test_conformance_host_part(tmp_path):
    """include/sim3opt_two_view.hpp compiles -Werror without Eigen or OpenCV; its add() / optimize() refusals and
    the C-ABI's leave everything as it was."""
    exe = compile_conformance(tmp_path)
    r = subprocess.run([exe, "host"], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 failed" in r.stdout, r.stdout + r.stderr


def test_conformance_fails_loudly_without_gpu(tmp_path):
    if gpu_available():
        pytest.skip("GPU present: covered by the gpu tests")
    exe = compile_conformance(tmp_path)
    path = str(tmp_path / "cases.txt")
    write_conformance_file(path, TC.WHOLE_RUN_CASES[:2])
    r = subprocess.run([exe, "run", path], capture_output=True, text=True)
    assert r.returncode == 3 and "no usable HIP device" in r.stderr, r.stdout + r.stderr


def test_both_builds_export_the_batch_symbols(tmp_path):
    """The Makefile's library and build.py's: ba_batch.hip is in the one list of translation units both read."""
    assert len(BATCH_SYMBOLS) == 15 and "sim3opt_ba_batch_debug_trial" in BATCH_SYMBOLS
    out = str(tmp_path / "libsim3opt.so")
    subprocess.check_call(["make", "-C", ROOT, "LIB=" + out, out], stdout=subprocess.DEVNULL)
    from sim3opt_amd import build as B
    for path in (out, B.LIB):
        lib = ctypes.CDLL(path)
        for name in BATCH_SYMBOLS:
            assert hasattr(lib, name), (path, name)
