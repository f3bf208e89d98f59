"""CPU side of the batched PnP RANSAC (sim3opt_pnp_batch, include/sim3opt.h): the conditions the comparisons of
tests/test_gpu_pnp_batch.py rest on hold for every case and option set it uses (tests/pnp_cases.py), the restatement
(tests/pnp_ref.py) finds the planted truth and notices seeded one-line defects, the kernel's per-hypothesis
arithmetic (sim3opt_amd/csrc/pnp_math.hpp), compiled for the host, agrees with the restatement's other P3P, the host
helper and every argument check work without a GPU, and the library says so when there is none."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pnp_cases as PC
import pnp_ref as PR
from conftest import gpu_available
from oracle import ba_oracle as BO
from sim3opt_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THR2 = PC.OPTS["reproj_error"] ** 2
# Largest deviation of the reference's final pose from the planted truth over SIZE_CASES, measured: 9.24e-4 rad (the
# 5-point problem; 3.2e-4 rad from 63 points on) and 9.72e-3 m (the 4-point problem; 4.5e-3 m from 63 points on).
# Asserted: twice that.
TRUTH_ROT, TRUTH_T = 2 * 9.24e-4, 2 * 9.72e-3
# ... and of the pose after the two-view refinement that starts from it (oracle/ba_oracle.py in BAOptimize's
# configuration on the PnP inliers, CONFORMANCE_CASES), measured: 8.47e-4 rad and 6.49e-2 m -- the length of the
# translation is a gauge of a two-view problem with free points, held by the start alone.  Asserted: twice that.
REFINED_ROT, REFINED_T = 2 * 8.47e-4, 2 * 6.49e-2
CONFORMANCE_CASES = PC.SIZE_CASES[2:9]
PNP_SYMBOLS = [s for s in L.SYMBOLS if s.startswith("sim3opt_pnp_batch_")]


def off_threshold(e2):
    e2 = e2[np.isfinite(e2)]
    return bool((np.abs(e2 - THR2) > 1e-9 * THR2).all())


@pytest.mark.parametrize("case,items", PC.RUNS, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else None)
def test_conditions_of_the_gpu_comparisons(case, items):
    """Threshold margin, conditioning, a best hypothesis that cannot be mistaken, a stable refit."""
    ref, well = PC.reference(*case, items), PC.conditioning(*case, items)
    hyp, best, opts = ref["hyp"], ref["best"], PC.merged(items)
    H = opts["iterations"]
    # no (valid hypothesis, point) within 1e-9 relative of the threshold (the nearest seen: 5.6e-5); none left out
    assert off_threshold(hyp["e2"]), (case, items)
    # ... nor at the final pose, whose mask is compared
    assert off_threshold(PC.reference_scores(PC.make_case(*case), ref["pose"][None])[2])
    # at most 5 of 100 hypotheses are ill-conditioned
    assert (~well).sum() <= 5 * H // 100, (case, items, int((~well).sum()))
    assert hyp["valid"].sum() >= max(1, H // 2)
    # the best hypothesis is well-conditioned, and every other one has a smaller count, or an equal count and a cost
    # more than 1e-6 relative larger (an ill-conditioned one: a smaller count even at twice the threshold)
    assert best >= 0 and well[best] and hyp["valid"][best], (case, items)
    with np.errstate(invalid="ignore"):
        count2 = ((hyp["z"] > 0) & (hyp["e2"] <= 4.0 * THR2)).sum(1)
    for h in np.where(hyp["valid"])[0]:
        if h == best:
            continue
        if not well[h]:
            assert count2[h] < hyp["count"][best], (case, items, h)
        elif hyp["count"][h] == hyp["count"][best]:
            gap = hyp["cost"][h] - hyp["cost"][best]
            if case[0] >= 63:
                assert gap > 1e-6 * hyp["cost"][best], (case, items, h, gap)
            elif not gap > 1e-6 * hyp["cost"][best]:
                # exact fits of the same points tie in cost to rounding: then they are the same pose
                assert np.abs(hyp["R"][h] - hyp["R"][best]).max() < 1e-9, (case, items, h)
                assert np.abs(hyp["t"][h] - hyp["t"][best]).max() < 1e-9, (case, items, h)
        else:
            assert hyp["count"][h] < hyp["count"][best]
    # a relative 1e-13 on the inputs: the same best hypothesis, inliers and trial counts, and a final pose within a
    # fifth of the 1e-8 / 1e-7 it is compared at
    moved = PC.run_reference(PC.perturbed(PC.make_case(*case), 1e-13), opts)
    if case[0] >= 63:
        assert moved["best"] == best
    assert np.array_equal(moved["mask"], ref["mask"]) and moved["status"] == ref["status"]
    if ref["refit"] is not None:
        assert moved["refit"]["trials"] == ref["refit"]["trials"], (case, items)
    assert PC.quat_dist(moved["pose"][:4], ref["pose"][:4]) < 2e-9, (case, items)
    assert np.abs(moved["pose"][4:] - ref["pose"][4:]).max() < 2e-8, (case, items)


def test_supplied_poses_are_off_the_threshold():
    """The scoring operator's poses (truth, the reference's hypotheses, a pose with points behind the camera)."""
    behind = 0
    for case in PC.SIZE_CASES:
        _, _, e2, z = PC.reference_scores(PC.make_case(*case), PC.score_poses(*case))
        assert off_threshold(e2), case
        behind += int((z[-1] <= 0).sum())
    assert behind > 0


@pytest.mark.parametrize("case,keep,far", PC.REFIT_RUNS, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_refit_operator_runs_are_stable(case, keep, far):
    ref = PC.reference_refit(case, keep, far)
    pose, mask = PC.refit_input(case, keep, far)
    assert mask.sum() == (6 if keep else PC.reference(*case)["hyp"]["count"][PC.reference(*case)["best"]])
    c = PC.perturbed(PC.make_case(*case), 1e-13)
    rng = np.random.default_rng(5)
    moved = PR.refit(pose * (1.0 + 1e-13 * rng.uniform(-1, 1, 7)), c["points"], c["uv1"], mask, PC.FOCAL, PC.CX, PC.CY,
                     PC.OPTS)
    assert moved["trials"] == ref["trials"], (case, keep)
    assert len(ref["trials"]) >= 2 and ref["chi2_after"] < ref["chi2_before"]
    assert (max(ref["trials"]) > 1) == far  # (the far start exercises the rejection branch)
    assert PC.quat_dist(moved["pose"][:4], ref["pose"][:4]) < 2e-9
    assert np.abs(moved["pose"][4:] - ref["pose"][4:]).max() < 2e-8


def test_reference_finds_the_planted_truth():
    """Largest deviations measured over SIZE_CASES: 9.24e-4 rad (the 5-point problem) and 9.72e-3 m (the 4-point
    problem); from 63 points on 3.2e-4 rad and 4.5e-3 m.  Asserted: twice the measured values."""
    worst = [0.0, 0.0]
    for case in PC.SIZE_CASES:
        ref, c = PC.reference(*case), PC.make_case(*case)
        rot = PC.rot_dist(ref["pose"][:4], c["cam1_true"][:4])
        dt = float(np.abs(ref["pose"][4:] - c["cam1_true"][4:]).max())
        print(f"truth {case}: {rot:.3e} rad, {dt:.3e} m")
        worst = [max(worst[0], rot), max(worst[1], dt)]
        assert rot <= TRUTH_ROT and dt <= TRUTH_T, (case, rot, dt)
        if case[0] >= 63:  # the inliers are the points that were not moved, give or take the noise's tail
            assert (ref["mask"] != ~c["outlier"]).sum() <= 0.03 * case[0], case
    print(f"truth: worst {worst[0]:.3e} rad, {worst[1]:.3e} m")
    assert worst[0] > TRUTH_ROT / 4 and worst[1] > TRUTH_T / 4  # (the bound is twice the measurement, not more)


def test_sampler_is_the_stated_one():
    assert PR.splitmix64(0) == 0xE220A8397B1DCDAF  # the published first output of SplitMix64 seeded with 0
    for n in (4, 5, 9, 1153):
        for h in range(300):
            s = PR.sample(0, h, n)
            assert len(set(s)) == 4 and min(s) >= 0 and max(s) < n
    assert [sorted(PR.sample(7, h, 4)) for h in range(20)] == [[0, 1, 2, 3]] * 20
    first = np.array([PR.sample(0, h, 1000)[0] for h in range(4000)])
    assert abs(first.mean() - 499.5) < 15  # uniform


def test_reference_notices_seeded_defects():
    case = (65, 5)
    c, ref = PC.make_case(*case), PC.reference(*case)
    # a sampler off by one in the skip rule repeats an index
    assert any(len(set(PR.sample(0, h, 5, "sampler_skip"))) < 4 for h in range(100))
    # '<' for '<=' at the threshold: a point exactly 3 px off, and the depth test: a point behind the camera that
    # projects onto its pixel
    X = np.array([[3.0, 0.0, 1.0], [0.0, 0.0, -5.0], [0.5, 0.0, 1.0]])
    uv = np.zeros((3, 2))
    uv[2, 0] = 0.5
    I, z = np.eye(3), np.zeros(3)
    assert list(PR.inliers(I, z, X, uv, 1.0, 0.0, 0.0, 3.0)[0]) == [True, False, True]
    assert list(PR.inliers(I, z, X, uv, 1.0, 0.0, 0.0, 3.0, "strict_threshold")[0]) == [False, False, True]
    assert list(PR.inliers(I, z, X, uv, 1.0, 0.0, 0.0, 3.0, "no_depth_test")[0]) == [True, True, True]
    # taking the first P3P solution instead of the one the fourth point chooses
    bad = PR.hypotheses(c["points"], c["uv1"], PC.FOCAL, PC.CX, PC.CY, PC.OPTS, "first_solution")
    differs = np.where(np.abs(bad["R"] - ref["hyp"]["R"]).reshape(100, -1).max(1) > 1e-6)[0]
    assert len(differs) >= 5
    assert (bad["count"][differs] <= ref["hyp"]["count"][differs]).all()
    assert (bad["count"][differs] < ref["hyp"]["count"][differs]).any()
    # a tie-break that ignores the cost
    tie = dict(valid=np.array([True, True, True]), count=np.array([5, 7, 7]), cost=np.array([0.1, 2.0, 1.0]))
    assert PR.best_hypothesis(tie) == 2 and PR.best_hypothesis(tie, "tie_ignores_cost") == 1
    # a refit over all points instead of the inliers is drawn off by the gross outliers
    off = PC.run_reference(c, PC.OPTS, "refit_all_points")
    assert PC.rot_dist(off["pose"][:4], c["cam1_true"][:4]) > 4 * PC.rot_dist(ref["pose"][:4], c["cam1_true"][:4])


def test_reference_p3p_reproduces_an_exact_pose():
    """Noise-free pixels: one of the P3P solutions is the planted pose, to rounding times conditioning."""
    rng = np.random.default_rng(3)
    c = PC.make_case(65, 5)
    R, t = BO.quat_to_R(c["cam1_true"][:4]), c["cam1_true"][4:]
    uv = PC._project(R, t, c["points"])
    for _ in range(20):
        s = rng.choice(65, 4, replace=False)
        ok, Rh, th, ns = PR.hypothesis(c["points"][s], uv[s], PC.FOCAL, PC.CX, PC.CY)
        assert ok and 1 <= ns <= 4
        assert np.abs(Rh - R).max() < 1e-7 and np.abs(th - t).max() < 1e-6


def compile_cxx(tmp_path, name, flags=(), link=True):
    exe = str(tmp_path / name)
    libdir = os.path.join(ROOT, "sim3opt_amd")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cxx", name + ".cpp")]
    if link:
        cmd += ["-L" + libdir, "-lsim3opt", "-Wl,-rpath," + libdir]
    subprocess.check_call(cmd + ["-o", exe])
    return exe


def compile_conformance(tmp_path):
    return compile_cxx(tmp_path, "pnp_conformance")


def conformance_uv0(c):
    """camera 0's pixels of case c: the points' projections with 0.5 px noise"""
    rng = np.random.default_rng(5000 + c[1])
    return PC._project(np.eye(3), np.zeros(3), PC.make_case(*c)["points"]) + 0.5 * rng.standard_normal((c[0], 2))


def write_conformance_file(path, cases):
    """The candidates of `cases` as the detector has them, each followed by the planted pose of camera 1; the bound
    of test_refinement_from_the_reference_pose_finds_the_truth in the first line."""
    with open(path, "w") as f:
        w = lambda *v: f.write(" ".join(repr(float(x)) if not isinstance(x, (int, np.integer)) else str(x)
                                        for x in v) + "\n")
        w(len(cases), PC.FOCAL, PC.CX, PC.CY, REFINED_ROT, REFINED_T)
        for c in cases:
            case, uv0 = PC.make_case(*c), conformance_uv0(c)
            w(c[0])
            for i in range(c[0]):
                w(*case["points"][i], *uv0[i], *case["uv1"][i])
            w(*case["cam1_true"])


def test_refinement_from_the_reference_pose_finds_the_truth():
    """What tests/cxx/pnp_conformance.cpp does on the device, through the two restatements: pnp_ref's pose and inliers
    into oracle/ba_oracle.py in BAOptimize's configuration.  Largest deviations of the refined pose from the planted
    truth over CONFORMANCE_CASES, measured: 8.47e-4 rad (65 points) and 6.49e-2 m (64 points).  Asserted: twice that."""
    import two_view_cases as TC
    worst = [0.0, 0.0]
    for c in CONFORMANCE_CASES:
        case, ref, uv0 = PC.make_case(*c), PC.reference(*c), conformance_uv0(c)
        m = ref["mask"]
        out = TC.run_oracle(dict(cam0=np.array([0.0, 0, 0, 1, 0, 0, 0]), cam1=ref["pose"], points=case["points"][m],
                                 uv0=uv0[m], uv1=case["uv1"][m]), TC.DEFAULTS)
        rot = PC.rot_dist(out["cam1"][:4], case["cam1_true"][:4])
        dt = float(np.abs(out["cam1"][4:] - case["cam1_true"][4:]).max())
        print(f"refined {c}: {rot:.3e} rad, {dt:.3e} m")
        worst = [max(worst[0], rot), max(worst[1], dt)]
    assert worst[0] <= REFINED_ROT and worst[1] <= REFINED_T, worst
    assert worst[0] > REFINED_ROT / 4 and worst[1] > REFINED_T / 4


def test_kernel_arithmetic_on_the_host_matches_the_reference(tmp_path):
    """sim3opt_amd/csrc/pnp_math.hpp (sampler, closed-form quartic, P3P, the fourth point's choice), the statements the
    kernel runs, compiled for the host: the same samples; for well-conditioned hypotheses the same validity and
    solution count and R, t within 1e-6 of the restatement's other formulation (measured: 8e-9)."""
    exe = compile_cxx(tmp_path, "pnp_math_driver", flags=("-O2", "-Wno-unknown-pragmas"), link=False)
    for case in PC.SIZE_CASES:
        c, hyp, well = PC.make_case(*case), PC.reference(*case)["hyp"], PC.conditioning(*case)
        path = str(tmp_path / "case.txt")
        with open(path, "w") as f:
            f.write(f"{PC.FOCAL!r} {PC.CX!r} {PC.CY!r} 0 100 {case[0]}\n")
            for p, u in zip(c["points"], c["uv1"]):
                f.write(" ".join(repr(float(x)) for x in (*p, *u)) + "\n")
        out = np.array([[float(x) for x in ln.split()] for ln in
                        subprocess.check_output([exe, path], text=True).splitlines()])
        assert np.array_equal(out[:, :4], hyp["sample"]), case
        assert np.isfinite(out).all()
        assert np.array_equal(out[well, 4].astype(bool), hyp["valid"][well]), case
        assert np.array_equal(out[well, 5].astype(int), hyp["n_solutions"][well]), case
        use = well & hyp["valid"]
        dR = np.abs(out[use, 6:15].reshape(-1, 3, 3) - hyp["R"][use]).max()
        dt = (np.abs(out[use, 15:18] - hyp["t"][use]).max(1) / np.maximum(1, np.linalg.norm(hyp["t"][use], axis=1))).max()
        assert dR < 1e-6 and dt < 1e-6, (case, dR, dt)


def test_median_depth_ratio():
    """sim3opt_median_depth_ratio (host) against numpy.sort, even and odd counts; its refusals."""
    rng = np.random.default_rng(11)
    sizes = [1, 2, 9, 10, 219, 1047]
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    d0, d1 = rng.uniform(4, 60, ptr[-1]), rng.uniform(4, 60, ptr[-1])
    got = L.median_depth_ratio(ptr, d0, d1)
    assert np.array_equal(got, PR.median_depth_ratio(ptr, d0, d1))
    assert got[0] == d1[0] / d0[0] and got[1] == max(d1[1:3]) / max(d0[1:3])  # index floor(0.5 n): the upper median
    for bad in (np.array([0, 3, 3], dtype=np.int32), np.array([1, 3, 5], dtype=np.int32)):
        with pytest.raises(L.Sim3OptError) as e:
            L.median_depth_ratio(bad, d0, d1)
        assert e.value.code == L.ERR_ARG
    d0[2] = np.nan
    with pytest.raises(L.Sim3OptError):
        L.median_depth_ratio(ptr, d0, d1)


def test_defaults_are_the_detectors():
    o = L.PnpBatchOptions()
    L.load().sim3opt_pnp_batch_options_default(ctypes.byref(o))
    got = {k: getattr(o, k) for k, _ in L.PnpBatchOptions._fields_}
    assert got == dict(PR.DEFAULTS, device=-1)
    assert len(PNP_SYMBOLS) == 14


def small_batch():
    a = PC.batch_arrays(((5, 27), (4, 1)))
    a = dict(a, point_ptr=np.array([0, 5, 8, 9], dtype=np.int32))  # 5, 3 and 1 points
    b = L.PnpBatch()
    b.set_problems(**a)
    return a, b


@pytest.mark.parametrize("what", ["no_problem", "empty_problem", "not_monotone", "ptr0", "nan_point", "inf_uv1", "focal"])
def test_set_problems_refuses_and_changes_nothing(what):
    a, b = small_batch()
    assert b.dims() == (3, 9)  # (problems of 1-3 points are accepted: they end with status 1)
    bad = {k: np.array(v) for k, v in a.items()}
    kw = {}
    if what == "no_problem":
        bad["point_ptr"] = np.array([0], dtype=np.int32)
    elif what == "empty_problem":
        bad["point_ptr"] = np.array([0, 5, 5, 9], dtype=np.int32)
    elif what == "not_monotone":
        bad["point_ptr"] = np.array([0, 6, 5, 9], dtype=np.int32)
    elif what == "ptr0":
        bad["point_ptr"] = np.array([1, 5, 6, 9], dtype=np.int32)
    elif what == "nan_point":
        bad["points"][7, 1] = np.nan
    elif what == "inf_uv1":
        bad["uv1"][8, 1] = -np.inf
    elif what == "focal":
        kw["focal"] = 0.0
    with pytest.raises(L.Sim3OptError) as e:
        b.set_problems(**bad, **kw)
    assert e.value.code == L.ERR_ARG and "pnp_batch_set_problems" in str(e.value)
    assert b.dims() == (3, 9)


@pytest.mark.parametrize("kw", [dict(iterations=0), dict(iterations=4097), dict(reproj_error=0.0),
                                dict(reproj_error=float("inf")), dict(min_points=3), dict(min_inliers=-1),
                                dict(refine_iters=-1), dict(max_trials=0), dict(tau=0.0), dict(tau=float("nan"))])
def test_set_options_refuses_and_changes_nothing(kw):
    _, b = small_batch()
    before = b.options()
    with pytest.raises(L.Sim3OptError) as e:
        b.set_options(**kw)
    assert e.value.code == L.ERR_ARG
    assert b.options() == before and b.dims() == (3, 9)
    b.set_options(iterations=4096, refine_iters=0, seed=2 ** 64 - 1)  # the ends of the ranges are taken
    assert b.options()["seed"] == 2 ** 64 - 1


def test_state_errors_before_a_solve():
    _, b = small_batch()
    for call in (b.poses, b.inliers, b.summary, lambda: b.debug_hypotheses(0)):
        with pytest.raises(L.Sim3OptError) as e:
            call()
        assert e.value.code == L.ERR_STATE
    with pytest.raises(L.Sim3OptError) as e:
        L.PnpBatch().solve()
    assert e.value.code == L.ERR_STATE


def test_fails_loudly_without_gpu():
    if gpu_available():
        pytest.skip("GPU present: covered by the gpu tests")
    _, b = small_batch()
    for call in (b.solve, lambda: b.debug_score(np.tile([0.0, 0, 0, 1, 0, 0, 0], (3, 1, 1))),
                 lambda: b.debug_refine(np.tile([0.0, 0, 0, 1, 0, 0, 0], (3, 1)), np.ones(9, dtype=np.uint8))):
        with pytest.raises(L.Sim3OptError) as e:
            call()
        assert e.value.code == L.ERR_NO_DEVICE and "no usable HIP device" in str(e.value)
    assert b.dims() == (3, 9)


def test_conformance_host_part(tmp_path):
    """include/sim3opt_pnp.hpp compiles -Werror beside sim3opt_two_view.hpp without Eigen or OpenCV; its add() / solve()
    refusals and the C-ABI's leave everything as it was; the median depth ratio."""
    exe = compile_conformance(tmp_path)
    r = subprocess.run([exe, "host"], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 failed" in r.stdout, r.stdout + r.stderr


def test_conformance_fails_loudly_without_gpu(tmp_path):
    if gpu_available():
        pytest.skip("GPU present: covered by the gpu tests")
    exe = compile_conformance(tmp_path)
    path = str(tmp_path / "candidates.txt")
    write_conformance_file(path, CONFORMANCE_CASES[:2])
    r = subprocess.run([exe, "run", path], capture_output=True, text=True)
    assert r.returncode == 3 and "no usable HIP device" in r.stderr, r.stdout + r.stderr
