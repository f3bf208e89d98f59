"""CPU side of the batched essential-matrix RANSAC (sim3opt_essential_batch, include/sim3opt.h): the conditions the
comparisons of tests/test_gpu_essential_batch.py rest on hold for every case and option set it uses
(tests/essential_cases.py), the restatement (tests/essential_ref.py) finds the planted truth and notices seeded
one-line defects, the kernel's per-hypothesis arithmetic (sim3opt_amd/csrc/essential_math.hpp), compiled for the host
with the address and undefined-behaviour sanitizers, agrees with the restatement's other solver, every argument check
works without a GPU, and the library says so when there is none.

E_LIMIT, the bound on |E_host -+ E_restatement| (entries of matrices of Frobenius norm 1) on well-conditioned
hypotheses, here and on the GPU: the host build's worst deviation measured over every run of essential_cases.RUNS is
9.46e-11 (median 1.4e-14, 99th percentile 2.7e-11); 32 times that is 3.0e-9, which is tighter than 100 x the 1e-10
conditioning threshold, so the limit is that floor, 1e-8.  It is set against the restatement, never the device.
Known limit of the kernel's solver, inside RUNS and asserted as such (essential_cases.KNOWN_FEWER_SOLUTIONS): where two
solutions nearly coincide in the coordinate its polynomial is in, the root pair can come out complex -- case (65, 5)
under sampler seed 4242, hypothesis 33 (counted from 0), well-conditioned by the restatement, gives two real solutions
for the restatement's four (one such hypothesis in about 3000 looked at); its chosen E is the restatement's all the same.

Largest deviation of the restatement's pose from the planted truth over SIZE_CASES, measured: from nine points on
1.886e-3 rad in the rotation and 3.318e-2 rad in the direction of t (both the 257-point problem); the six-point
problem, an exact fit of noisy pixels that the translation's direction hangs on weakly, 2.540e-2 rad and 6.291e-1 rad.
Asserted: twice that, each class against its own measurement."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import essential_cases as EC
import essential_ref as ER
from conftest import gpu_available
from sim3opt_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_MEASURED = 9.46e-11
E_LIMIT = max(32 * E_MEASURED, 100 * 1e-10)
TRUTH_ROT, TRUTH_DIR = 2 * 1.886e-3, 2 * 3.318e-2
TRUTH_ROT_6, TRUTH_DIR_6 = 2 * 2.540e-2, 2 * 6.291e-1
ESS_SYMBOLS = [s for s in L.SYMBOLS if s.startswith("sim3opt_essential_batch_")]
RUN_IDS = lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else None


def thr2_of(opts):
    thr = opts["threshold"] / EC.FOCAL
    return thr * thr


def off(values, at):
    """no finite value within 1e-9 relative of `at` (at = 0: within 1e-9)"""
    v = values[np.isfinite(values)]
    return bool((np.abs(v - at) > 1e-9 * at).all()) if at else bool((np.abs(v) > 1e-9).all())


def check_conditions(case, items):
    """Threshold margin, conditioning, valid share, a best hypothesis and a vote that cannot be mistaken."""
    ref, well, opts = EC.reference(*case, items), EC.conditioning(*case, items), EC.merged(items)
    hyp, best, H, thr2 = ref["hyp"], ref["best"], opts["iterations"], thr2_of(opts)
    # no (valid hypothesis, point) within 1e-9 relative of the threshold; the final E is the best hypothesis's
    assert off(hyp["e2"][hyp["valid"]], thr2), (case, items)
    # at most 5 of 100 hypotheses are ill-conditioned; at least half are valid
    assert (~well).sum() <= max(5 * H // 100, 0), (case, items, int((~well).sum()))
    assert hyp["valid"].sum() >= max(1, H // 2), (case, items)
    # the best hypothesis is well-conditioned, and every other one has a smaller count, or an equal count and a cost
    # more than 1e-6 relative larger, or is the same E to 1e-9 (an ill-conditioned one: a smaller count even at
    # twice the threshold)
    assert best >= 0 and well[best] and hyp["valid"][best], (case, items)
    with np.errstate(invalid="ignore"):
        count2 = (hyp["e2"] <= 4.0 * thr2).sum(1)
    same = EC.same_up_to_sign(hyp["E"], np.broadcast_to(hyp["E"][best], hyp["E"].shape)) < 1e-9
    for h in np.where(hyp["valid"])[0]:
        if h == best or same[h]:
            continue
        if not well[h]:
            assert count2[h] < hyp["count"][best], (case, items, h)
        elif hyp["count"][h] == hyp["count"][best]:
            assert hyp["cost"][h] - hyp["cost"][best] > 1e-6 * hyp["cost"][best], (case, items, h)
        else:
            assert hyp["count"][h] < hyp["count"][best], (case, items, h)
    # the vote: no depth of an inlier within 1e-9 relative of 0 or of distance_threshold; the winner has at least
    # twice the runner-up's votes
    rec = ref["rec"]
    z = rec["z"][:, ref["mask_hypothesis"]]
    assert off(z, 0.0) and off(z, opts["distance_threshold"]), (case, items)
    votes = np.sort(rec["votes"])[::-1]
    assert votes[0] >= 2 * votes[1] and votes[0] > 0, (case, items, rec["votes"])
    assert ref["status"] == ER.OK


@pytest.mark.parametrize("case,items", EC.RUNS, ids=RUN_IDS)
def test_conditions_of_the_gpu_comparisons(case, items):
    check_conditions(case, items)


def test_supplied_matrices_are_off_the_threshold():
    """The scoring operator's matrices (truth, the reference's hypotheses, a zero row) and the pose operator's."""
    vanishing = 0
    for case in EC.SIZE_CASES:
        _, _, e2 = EC.reference_scores(EC.make_case(*case), EC.score_matrices(*case))
        assert off(e2, thr2_of(EC.OPTS)), case
        vanishing += int((~np.isfinite(e2[-1])).sum() + (e2[-1] > 1.0).sum())
    winners = []
    for p in EC.pose_problems():
        rec = EC.reference_pose(p)
        z = rec["z"][:, p["mask"]]
        assert off(z, 0.0) and off(z, EC.OPTS["distance_threshold"])
        winners.append((rec["winner"], int(rec["votes"].max())))
    assert sorted(w for w, _ in winners[:4]) == [0, 1, 2, 3] and all(v > 30 for _, v in winners[:4])
    assert winners[4] == (0, 0)  # nothing votes in the far scene: candidate 0 by the tie rule


def pose_error(ref, c):
    cosang = float(np.clip(np.dot(ref["t"], c["t_true"]), -1.0, 1.0))
    return EC.rot_angle(ref["R"], c["R_true"]), float(np.arccos(cosang))


def test_reference_finds_the_planted_truth():
    worst = [0.0, 0.0]
    for case in EC.SIZE_CASES:
        ref, c = EC.reference(*case), EC.make_case(*case)
        rot, ang = pose_error(ref, c)
        print(f"truth {case}: {rot:.3e} rad, direction {ang:.3e} rad")
        if case[0] < 9:
            assert TRUTH_ROT_6 / 4 < rot <= TRUTH_ROT_6 and TRUTH_DIR_6 / 4 < ang <= TRUTH_DIR_6, (case, rot, ang)
            continue
        worst = [max(worst[0], rot), max(worst[1], ang)]
        assert rot <= TRUTH_ROT and ang <= TRUTH_DIR, (case, rot, ang)
        assert abs(np.linalg.norm(ref["t"]) - 1.0) < 1e-12 and abs(np.linalg.norm(ref["E"]) - 1.0) < 1e-12
        if case[0] >= 63:  # the inliers are the points that were not moved, give or take the noise's tail and depth
            assert (ref["mask_hypothesis"] != ~c["outlier"]).sum() <= 0.06 * case[0], case
    print(f"truth: worst {worst[0]:.3e} rad, {worst[1]:.3e} rad")
    assert worst[0] > TRUTH_ROT / 4 and worst[1] > TRUTH_DIR / 4  # (the bound is twice the measurement, not more)


def test_sampler_is_the_stated_one():
    assert ER.splitmix64(0) == 0xE220A8397B1DCDAF  # the published first output of SplitMix64 seeded with 0
    for n in (6, 7, 9, 1073):
        for h in range(300):
            s = ER.sample(0, h, n)
            assert len(set(s)) == 6 and min(s) >= 0 and max(s) < n
    assert [sorted(ER.sample(7, h, 6)) for h in range(20)] == [[0, 1, 2, 3, 4, 5]] * 20
    first = np.array([ER.sample(0, h, 1000)[0] for h in range(4000)])
    assert abs(first.mean() - 499.5) < 15  # uniform


def test_reference_notices_seeded_defects():
    """Nine one-line defects, each changing an output a test asserts."""
    case = (65, 5)
    c, ref = EC.make_case(*case), EC.reference(*case)
    x0, x1 = ER.normalise(c["uv0"], EC.FOCAL, EC.CX, EC.CY), ER.normalise(c["uv1"], EC.FOCAL, EC.CX, EC.CY)
    good, rot0 = ref["hyp"], pose_error(ref, c)[0]
    # 1 draws not stepped over earlier picks: a repeated index
    assert any(len(set(ER.sample(0, h, 7, "sampler_skip"))) < 6 for h in range(100))
    # 2 E for E^T: the truth no longer explains the points
    Et = EC.true_essential(c)
    n_true = int((ER.sampson(Et, x0, x1) <= thr2_of(EC.OPTS)).sum())
    assert n_true >= 40 and int((ER.sampson(Et, x0, x1, "E_transposed") <= thr2_of(EC.OPTS)).sum()) < n_true // 2
    # 3 Sampson's denominator without the E^T x1 terms: other errors, and another cost of the best hypothesis
    half = ER.sampson(Et, x0, x1, "sampson_half_denominator")
    full = ER.sampson(Et, x0, x1)
    assert (half > full).all() and half[full <= thr2_of(EC.OPTS)].sum() > 1.5 * full[full <= thr2_of(EC.OPTS)].sum()
    # 4 the trace term with factor 1 instead of 2: the solutions are no essential matrices, and fit nothing
    bad = ER.hypotheses(c["uv0"], c["uv1"], EC.FOCAL, EC.CX, EC.CY, EC.OPTS, "trace_factor_1")
    assert bad["count"].max() < good["count"].max() and bad["count"].sum() < good["count"].sum() // 2
    # 5 the sixth point ignored: other solutions chosen, never better ones
    bad = ER.hypotheses(c["uv0"], c["uv1"], EC.FOCAL, EC.CX, EC.CY, EC.OPTS, "ignore_sixth")
    differs = EC.same_up_to_sign(bad["E"], good["E"]) > 1e-6
    assert differs.sum() >= 20 and bad["count"][differs].sum() < good["count"][differs].sum()
    # 6 the threshold not divided by focal: every point an inlier
    bad = EC.run_reference(c, EC.OPTS, "threshold_not_normalised")
    assert bad["hyp"]["count"].max() == case[0] and pose_error(bad, c)[0] > 2 * rot0
    # 7 t for -t in candidates 2 and 3: the winner of this case, candidate 2, is lost
    assert ref["rec"]["winner"] == 2
    bad = EC.run_reference(c, EC.OPTS, "t_sign_23")
    assert bad["rec"]["votes"][2] < ref["rec"]["votes"][2] // 2
    # 8 votes not limited by distance_threshold: the far scene votes
    far = EC.pose_problems()[4]
    assert EC.reference_pose(far)["votes"].max() == 0 and EC.reference_pose(far, defect="no_distance_threshold")["votes"].max() == 40
    # 9 a tie-break that ignores the cost
    tie = dict(valid=np.array([True, True, True]), count=np.array([5, 7, 7]), cost=np.array([0.1, 2.0, 1.0]))
    assert ER.best_hypothesis(tie) == 2 and ER.best_hypothesis(tie, "tie_ignores_cost") == 1


def test_reference_solver_reproduces_an_exact_pose():
    """Noise-free pixels: one of the five-point solutions is the planted E, and the sixth point chooses it."""
    c = EC.make_case(65, 5)
    uv0 = EC.project(np.eye(3), np.zeros(3), c["points"])
    uv1 = EC.project(c["R_true"], c["t_true"] * c["scale"], c["points"])
    hyp = ER.hypotheses(uv0, uv1, EC.FOCAL, EC.CX, EC.CY, dict(EC.OPTS, iterations=20))
    assert hyp["valid"].all()
    d = EC.same_up_to_sign(hyp["E"], np.broadcast_to(EC.true_essential(c), hyp["E"].shape))
    assert d.max() < 1e-7, d.max()
    rec = ER.recover_pose(hyp["E"][0], ER.normalise(uv0, EC.FOCAL, EC.CX, EC.CY), ER.normalise(uv1, EC.FOCAL, EC.CX, EC.CY),
                          np.ones(65, dtype=bool), 50.0)
    R, t = rec["candidates"][rec["winner"]]
    assert EC.rot_angle(R, c["R_true"]) < 1e-6 and np.abs(t - c["t_true"]).max() < 1e-6
    for k, (Rk, tk) in enumerate(rec["candidates"]):  # the candidates are what the header says they are
        sign = 1.0 if k in (0, 2) else -1.0
        tt = rec["candidates"][k % 2][1]
        assert (sign * hyp["E"][0] * (ER.skew(tt) @ Rk)).sum() > 0.99 / np.sqrt(2) and abs(np.linalg.det(Rk) - 1) < 1e-12


def compile_cxx(tmp_path, name, flags=(), link=True):
    exe = str(tmp_path / name)
    libdir = os.path.join(ROOT, "sim3opt_amd")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cxx", name + ".cpp")]
    if link:
        cmd += ["-L" + libdir, "-lsim3opt", "-Wl,-rpath," + libdir]
    subprocess.check_call(cmd + ["-o", exe])
    return exe


def points_text(c):
    return "".join(" ".join(repr(float(x)) for x in (*a, *b)) + "\n" for a, b in zip(c["uv0"], c["uv1"]))


def run_driver(exe, mode, text):
    out = subprocess.run([exe, mode], input=text, capture_output=True, text=True)
    assert out.returncode == 0 and not out.stderr, out.stderr  # (a sanitizer report lands in stderr)
    return np.array([[float(x) for x in ln.split()] for ln in out.stdout.splitlines()])


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """tests/cxx/essential_math_driver.cpp: a stand-alone program under the address and undefined-behaviour sanitizers"""
    return compile_cxx(tmp_path_factory.mktemp("essential"), "essential_math_driver",
                       flags=("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                              "-Wno-unknown-pragmas"), link=False)


def test_kernel_arithmetic_on_the_host_matches_the_reference(driver):
    """sim3opt_amd/csrc/essential_math.hpp (sampler, five-point method, the sixth point's choice), the statements the
    kernel runs, compiled for the host: the same samples in every run; on well-conditioned hypotheses the same
    validity, the same number of real solutions and the chosen E within E_LIMIT of the restatement's other solver."""
    worst = 0.0
    for case, items in EC.RUNS:
        c, o = EC.make_case(*case), EC.merged(items)
        hyp, well = EC.reference(*case, items)["hyp"], EC.conditioning(*case, items)
        head = f"{EC.FOCAL!r} {EC.CX!r} {EC.CY!r} {o['seed']} {o['iterations']} {case[0]}\n"
        out = run_driver(driver, "hyp", head + points_text(c))
        assert np.array_equal(out[:, :6], hyp["sample"]), (case, items)
        assert np.isfinite(out).all()
        assert np.array_equal(out[well, 6].astype(bool), hyp["valid"][well]), (case, items)
        exact = EC.exact_count_mask(case, items, well)
        assert np.array_equal(out[exact, 7].astype(int), hyp["n_solutions"][exact]), (case, items)
        for h in EC.KNOWN_FEWER_SOLUTIONS.get((case, items), ()):  # the known limit: named, and no more than that
            assert well[h] and hyp["valid"][h] and 1 <= out[h, 7] <= hyp["n_solutions"][h], (case, items, h)
        E = out[:, 8:17].reshape(-1, 3, 3)
        norm = np.sqrt((E ** 2).sum(axis=(1, 2)))
        assert (np.abs(norm[out[:, 6] == 1] - 1.0) < 1e-14).all() and (norm[out[:, 6] == 0] == 0).all()
        use = well & hyp["valid"]
        d = EC.same_up_to_sign(E, hyp["E"])[use].max()
        worst = max(worst, d)
        assert d < E_LIMIT, (case, items, d)
    print(f"host build against the restatement: worst |dE| {worst:.3e}")
    assert worst > E_MEASURED / 32  # (the limit rests on a measurement of this code, not of something more exact)


def test_scoring_and_pose_arithmetic_on_the_host(driver):
    """ess_sampson gives the restatement's bits per point, so counts are equal and costs differ by the order of their
    sums only; ess_candidates and ess_votes give the restatement's candidates to 1e-12 and its votes."""
    for case in EC.SIZE_CASES[:5]:
        c, Es = EC.make_case(*case), EC.score_matrices(*case)
        head = f"{EC.FOCAL!r} {EC.CX!r} {EC.CY!r} {EC.OPTS['threshold']!r} {case[0]} {len(Es)}\n"
        body = "".join(" ".join(repr(float(x)) for x in E.reshape(9)) + "\n" for E in Es)
        out = subprocess.run([driver, "score"], input=head + points_text(c) + body, capture_output=True, text=True)
        assert out.returncode == 0 and not out.stderr, out.stderr
        rows = [[float(x) for x in ln.split()] for ln in out.stdout.splitlines()]
        rc, rs, e2 = EC.reference_scores(c, Es)
        for k, row in enumerate(rows):
            assert int(row[0]) == rc[k], (case, k)
            assert abs(row[1] - rs[k]) <= 4 * np.finfo(float).eps * max(rc[k], 1) * rs[k], (case, k)
            got = np.array(row[2:])
            assert np.array_equal(np.isfinite(got), np.isfinite(e2[k])), (case, k)
            assert np.array_equal(got[np.isfinite(got)], e2[k][np.isfinite(got)]), (case, k)  # the same bits
    for p in EC.pose_problems():
        rec, n = EC.reference_pose(p), int(p["mask"].sum())
        c = dict(uv0=p["uv0"][p["mask"]], uv1=p["uv1"][p["mask"]])
        head = f"{EC.FOCAL!r} {EC.CX!r} {EC.CY!r} {EC.OPTS['distance_threshold']!r} {n} 1\n"
        out = run_driver(driver, "pose", head + points_text(c) + " ".join(repr(float(x)) for x in p["E"].reshape(9)) + "\n")[0]
        assert out[0] == 1
        for k, (R, t) in enumerate(rec["candidates"]):
            assert np.abs(ER.quat_to_R(out[1 + 7 * k:5 + 7 * k]) - R).max() < 1e-12
            assert np.abs(out[5 + 7 * k:8 + 7 * k] - t).max() < 1e-12
        assert np.array_equal(out[29:33].astype(int), rec["votes"])


def test_defaults_are_the_detectors():
    o = L.EssentialBatchOptions()
    L.load().sim3opt_essential_batch_options_default(ctypes.byref(o))
    got = {k: getattr(o, k) for k, _ in L.EssentialBatchOptions._fields_}
    assert got == dict(ER.DEFAULTS, device=-1)
    assert len(ESS_SYMBOLS) == 15
    assert L.load().sim3opt_version() == 130


def small_batch():
    a = EC.batch_arrays(((9, 1), (6, 5)))
    a = dict(a, point_ptr=np.array([0, 9, 12, 15], dtype=np.int32))  # 9, 3 and 3 points
    b = L.EssentialBatch()
    b.set_problems(**a)
    return a, b


@pytest.mark.parametrize("what", ["no_problem", "empty_problem", "not_monotone", "ptr0", "nan_uv0", "inf_uv1", "focal",
                                  "nan_cx"])
def test_set_problems_refuses_and_changes_nothing(what):
    a, b = small_batch()
    assert b.dims() == (3, 15)  # (problems of fewer than min_points points are accepted: they end with status 1)
    bad = {k: np.array(v) for k, v in a.items()}
    kw = {}
    if what == "no_problem":
        bad["point_ptr"] = np.array([0], dtype=np.int32)
    elif what == "empty_problem":
        bad["point_ptr"] = np.array([0, 9, 9, 15], dtype=np.int32)
    elif what == "not_monotone":
        bad["point_ptr"] = np.array([0, 10, 9, 15], dtype=np.int32)
    elif what == "ptr0":
        bad["point_ptr"] = np.array([1, 9, 12, 15], dtype=np.int32)
    elif what == "nan_uv0":
        bad["uv0"][7, 1] = np.nan
    elif what == "inf_uv1":
        bad["uv1"][14, 0] = -np.inf
    elif what == "focal":
        kw["focal"] = 0.0
    elif what == "nan_cx":
        kw["cx"] = float("nan")
    with pytest.raises(L.Sim3OptError) as e:
        b.set_problems(**bad, **kw)
    assert e.value.code == L.ERR_ARG and "essential_batch_set_problems" in str(e.value)
    assert b.dims() == (3, 15)


@pytest.mark.parametrize("kw", [dict(iterations=0), dict(iterations=4097), dict(threshold=0.0),
                                dict(threshold=float("inf")), dict(distance_threshold=0.0),
                                dict(distance_threshold=float("nan")), dict(min_points=5)])
def test_set_options_refuses_and_changes_nothing(kw):
    _, b = small_batch()
    before = b.options()
    with pytest.raises(L.Sim3OptError) as e:
        b.set_options(**kw)
    assert e.value.code == L.ERR_ARG and "value out of range" in str(e.value)
    assert b.options() == before and b.dims() == (3, 15)
    b.set_options(iterations=4096, min_points=6, seed=2 ** 64 - 1)  # the ends of the ranges are taken
    assert b.options()["seed"] == 2 ** 64 - 1 and b.tiles() == (EC.LDS_POINTS, EC.CHUNK)


def test_state_and_argument_errors_before_a_solve():
    _, b = small_batch()
    for call in (b.poses, b.essentials, b.inliers, b.summary, lambda: b.debug_hypotheses(0)):
        with pytest.raises(L.Sim3OptError) as e:
            call()
        assert e.value.code == L.ERR_STATE
    with pytest.raises(L.Sim3OptError) as e:
        L.EssentialBatch().solve()
    assert e.value.code == L.ERR_STATE and "no problems set" in str(e.value)
    lib, nul = L.load(), None
    assert lib.sim3opt_essential_batch_debug_score(b._b, 0, nul, nul, nul) == L.ERR_ARG
    assert lib.sim3opt_essential_batch_debug_pose(b._b, nul, nul, nul, nul, nul, nul) == L.ERR_ARG
    assert lib.sim3opt_essential_batch_get_poses(b._b, nul) == L.ERR_ARG
    assert lib.sim3opt_essential_batch_get_essentials(b._b, nul) == L.ERR_ARG
    assert lib.sim3opt_essential_batch_get_inliers(b._b, nul, nul) == L.ERR_ARG
    assert lib.sim3opt_essential_batch_solve(nul) == L.ERR_ARG and lib.sim3opt_essential_batch_dims(nul, nul, nul, nul) == L.ERR_ARG
    nan_E = np.full((3, 1, 3, 3), np.nan)
    with pytest.raises(L.Sim3OptError) as e:
        b.debug_score(nan_E)
    assert e.value.code == L.ERR_ARG and "non-finite matrix" in str(e.value)
    with pytest.raises(L.Sim3OptError) as e:
        b.debug_pose(nan_E, np.ones(15, dtype=np.uint8))
    assert e.value.code == L.ERR_ARG and "non-finite matrix" in str(e.value)
    with pytest.raises(ValueError):
        b.debug_pose(np.zeros((2, 3, 3)), np.ones(15, dtype=np.uint8))


def test_fails_loudly_without_gpu():
    if gpu_available():
        pytest.skip("GPU present: covered by the gpu tests")
    _, b = small_batch()
    E = np.tile(np.eye(3), (3, 1, 1, 1))
    for call in (b.solve, lambda: b.debug_score(E), lambda: b.debug_pose(E, np.ones(15, dtype=np.uint8))):
        with pytest.raises(L.Sim3OptError) as e:
            call()
        assert e.value.code == L.ERR_NO_DEVICE and "no usable HIP device" in str(e.value)
    assert b.dims() == (3, 15)


CONFORMANCE_CASES = EC.SIZE_CASES[2:8]


def compile_conformance(tmp_path):
    return compile_cxx(tmp_path, "essential_conformance")


def write_conformance_file(path, cases):
    """The candidates of `cases` as the detector has them (points1, points2), each followed by the planted rotation
    and unit translation; the hypothesis count of OPTS and the bounds of test_reference_finds_the_planted_truth in the
    first line (the device's pose is within 1e-7 of the restatement's, which the bounds are twice the measurement of)."""
    with open(path, "w") as f:
        w = lambda *v: f.write(" ".join(repr(float(x)) if not isinstance(x, (int, np.integer)) else str(x)
                                        for x in v) + "\n")
        w(len(cases), EC.FOCAL, EC.CX, EC.CY, EC.OPTS["iterations"], TRUTH_ROT, TRUTH_DIR)
        for c in cases:
            case = EC.make_case(*c)
            w(c[0])
            for a, b in zip(case["uv0"], case["uv1"]):
                w(*a, *b)
            w(*case["R_true"].reshape(9), *case["t_true"])


def test_conformance_host_part(tmp_path):
    """include/sim3opt_essential.hpp compiles -Werror beside sim3opt_pnp.hpp without Eigen or OpenCV; its add() / solve()
    refusals and the C-ABI's leave everything as it was."""
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
