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
    assert len(BATCH_SYMBOLS) == 14
    out = str(tmp_path / "libsim3opt.so")
    subprocess.check_call(["make", "-C", ROOT, "LIB=" + out, out], stdout=subprocess.DEVNULL)
    from sim3opt_amd import build as B
    for path in (out, B.LIB):
        lib = ctypes.CDLL(path)
        for name in BATCH_SYMBOLS:
            assert hasattr(lib, name), (path, name)
