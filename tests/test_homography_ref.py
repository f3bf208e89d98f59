"""CPU side of the batched homography stage (sim3opt_homography_batch, include/sim3opt.h): the conditions the
comparisons of tests/test_gpu_homography_batch.py rest on hold for every case and option set it uses
(tests/homography_cases.py), the restatement (tests/homography_ref.py) reaches both branches of the choice and every
status, finds the planted truth and notices seeded one-line defects, the kernel's arithmetic
(sim3opt_amd/csrc/homography_math.hpp), compiled for the host with the address and undefined-behaviour sanitizers,
agrees with the restatement, every argument check works without a GPU, and the library says so when there is none.

The limits, each measured from the host build of homography_math.hpp against the restatement over every run of
homography_cases.RUNS (2401 well-conditioned hypotheses, 19 solves), never against the device; each is 32 times the
worst deviation, floored by 100 x the 1e-10 conditioning threshold as the essential stage's E_LIMIT is:
  H_LIMIT      |H_host -+ H_restatement| of a hypothesis (Frobenius norm 1): worst 7.74e-13, median 2.3e-15, 99th
               percentile 8.5e-14 -> the floor, 1e-8
  SIGMA_LIMIT  |sigma^2_host - sigma^2_restatement| / sigma^2 of a round: worst 1.05e-10, median 1.2e-12, 99th percentile
               1.05e-10 -> the floor, 1e-8
  REFINED_LIMIT |H_host - H_restatement| after a round: worst 5.36e-11 -> the floor, 1e-8
  POSE_LIMIT   |R_host - R_restatement| (worst 3.2e-15) and |t_host - t_restatement| / |t| (worst 8.67e-11, median
               1.1e-12, 99th percentile 8.0e-11) -> the floor, 1e-8

The planted truth.  A plane alone leaves two Faugeras-Lustman solutions that explain the pixels equally; in every
listed scene both pass both visibility tests (dRatio = 1), and the Sampson sums that then decide differ by the noise
only: the reference's choice is the planted pose in about half the scenes.  That is the reference's behaviour, kept.
What is asserted: the planted pose is one of the two kept, within twice the largest deviation measured over SIZE_CASES
from 63 points on -- rotation 3.04e-3 rad, direction of t 2.92e-2 rad, plane normal 9.00e-2 rad, all three the scene
with repeated matches, which has the fewest distinct inliers; the ten-point case, an
estimate from ten noisy pixels, 5.85e-3, 7.56e-2 and 2.28e-2 rad -- and that where the second visibility test does
decide (the wide scenes) the chosen one is the planted one."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import homography_cases as HC
import homography_ref as HR
from conftest import gpu_available
from sim3opt_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR = 100 * 1e-10
H_MEASURED, SIGMA_MEASURED, REFINED_MEASURED, POSE_MEASURED = 7.74e-13, 1.05e-10, 5.36e-11, 8.67e-11
H_LIMIT = max(32 * H_MEASURED, FLOOR)
SIGMA_LIMIT = max(32 * SIGMA_MEASURED, FLOOR)
REFINED_LIMIT = max(32 * REFINED_MEASURED, FLOOR)
POSE_LIMIT = max(32 * POSE_MEASURED, FLOOR)
TRUTH_ROT, TRUTH_DIR, TRUTH_NORMAL = 2 * 3.04e-3, 2 * 2.92e-2, 2 * 9.00e-2
TRUTH_ROT_10, TRUTH_DIR_10, TRUTH_NORMAL_10 = 2 * 5.85e-3, 2 * 7.56e-2, 2 * 2.28e-2
MARGIN = 1e-9  # no compared quantity lies within this, relative, of the value it is tested against
HOM_SYMBOLS = [s for s in L.SYMBOLS if s.startswith("sim3opt_homography_batch_")]
RUN_IDS = lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else None


def off(values, at, rel=MARGIN):
    """no finite value within rel relative of `at` (at = 0: within rel)"""
    v = np.asarray(values, dtype=float)
    v = v[np.isfinite(v)]
    return bool((np.abs(v - at) > rel * at).all()) if at else bool((np.abs(v) > rel).all())


def check_choice(ch, what):
    """the conditions on a decomposition and its choice: distinct singular values, signed columns, visibility, dRatio,
    Sampson sums"""
    assert ch["status"] == HR.OK, what
    assert off(ch["vis_first"], 0.0) and off(ch["vis_second"], 0.0), what
    assert abs(ch["ratio"] - 0.9) > 1e-6, what
    if ch["ambiguous"]:
        assert abs(ch["sampson"][0] - ch["sampson"][1]) > 1e-6 * ch["sampson"].max(), (what, ch["sampson"])


def check_svd(H, what):
    U, d, V = HR.signed_svd(H)
    assert (d[0] - d[1]) > 1e-6 * d[0] and (d[1] - d[2]) > 1e-6 * d[0], (what, d)
    mags = np.sort(np.abs(V), axis=0)
    assert (mags[2] - mags[1] > 1e-6).all(), (what, V)  # which component leads a column of V is beyond doubt


def check_conditions(case, items):
    ref, opts = HC.reference(case, items), HC.merged(items)
    hyp, best, max2 = ref["hyp"], ref["best"], opts["max_pixel_error"] ** 2
    c = HC.make_case(*case)
    x0, x1 = HC.normalised(c)
    assert ref["status"] == HR.OK and best >= 0 and hyp["valid"][best] and HC.conditioning(case, items)[best]
    # the best hypothesis is unique in cost, or its twins are the same matrix
    same = HC.same_up_to_sign(hyp["H"], np.broadcast_to(hyp["H"][best], hyp["H"].shape)) < 1e-9
    for h in np.where(hyp["valid"])[0]:
        if h != best and not same[h]:
            assert hyp["cost"][h] - hyp["cost"][best] > 1e-6 * hyp["cost"][best], (case, items, h)
    assert not same[:best].any()  # (a twin before it would be the best: the smallest index)
    # no point within the margin of the inlier threshold; at least four inliers
    assert off(hyp["e2"][best], max2) and ref["n_inliers"] >= 4, (case, items)
    # no inlier's error within the margin of a round's sigma^2
    Hs = [ref["H_mlesac"]] + list(ref["refine"]["H"])
    for r, s2 in enumerate(ref["refine"]["sigma2"]):
        e2, _ = HR.sq_error(Hs[r], x0[ref["mask"]], x1[ref["mask"]], HC.FOCAL)
        assert off(e2, s2) and np.isfinite(e2).all(), (case, items, r)
    check_svd(ref["H_refined"], (case, items))
    check_choice(ref, (case, items))


@pytest.mark.parametrize("case,items", HC.RUNS, ids=RUN_IDS)
def test_conditions_of_the_gpu_comparisons(case, items):
    check_conditions(case, items)


def test_supplied_matrices_are_off_the_cap():
    """The scoring operator's matrices (the planted H, the reference's hypotheses, the identity): no squared error
    within the margin of max_pixel_error^2, and all of them finite."""
    for case in HC.SIZE_CASES:
        x0, x1 = HC.normalised(HC.make_case(*case))
        e2, _ = HR.sq_error(HC.score_matrices(case), x0, x1, HC.FOCAL)
        assert np.isfinite(e2).all() and off(e2, HC.OPTS["max_pixel_error"] ** 2), case


def test_listed_runs_cover_the_shapes():
    """even and odd inlier counts, tied errors, both sides of every size at which the kernel takes another path"""
    m = [HC.reference(c, i)["n_inliers"] for c, i in HC.RUNS]
    assert any(k % 2 == 0 for k in m) and any(k % 2 == 1 for k in m)
    dup = HC.reference((66, 2, "dup"))
    e2 = dup["hyp"]["e2"][dup["best"]][dup["mask"]]
    assert len(np.unique(e2)) < len(e2)  # the median is taken among ties
    assert not dup["hyp"]["valid"].all()  # ... and a sample with a repeated match is refused
    n = {c[0] for c, _ in HC.RUNS}
    assert {10, 63, 64, 65, 255, 256, 257, HC.LDS_POINTS - 1, HC.LDS_POINTS, HC.LDS_POINTS + 1} <= n
    h = {HC.merged(i)["iterations"] for _, i in HC.RUNS}
    assert {1, HC.CHUNK - 1, HC.CHUNK, HC.CHUNK + 1, 2 * HC.CHUNK + 1, 300} <= h
    assert HR.DEFAULTS["iterations"] == 300


def test_both_branches_and_every_status_are_reached():
    """The listed scenes all take the ambiguity branch (whole solves); dRatio < 0.9 is reached by the wide scenes through
    the restatement's equivalent of the decomposition operator.  FEW_POINTS, NO_HYPOTHESIS and NO_INLIERS are whole
    solves; DEGENERATE is the identity through the operator.  NO_INLIERS needs a threshold whose square is zero: a valid
    hypothesis fits its own four points, so at any threshold worth the name it has four inliers."""
    assert all(HC.reference(c, i)["ambiguous"] for c, i in HC.RUNS)
    probs = HC.supplied_problems()
    chs = [HC.reference_choice(p) for p in probs]
    nu, na = 2 * len(HC.WIDE_UNAMBIGUOUS), 2 * len(HC.WIDE_AMBIGUOUS)
    for p, ch in zip(probs[:-1], chs[:-1]):
        check_svd(p["H"], "supplied")
        check_choice(ch, "supplied")
    assert [ch["ambiguous"] for ch in chs[:-1]] == [False] * nu + [True] * (na + 2)
    assert all(ch["ratio"] < 0.9 - 1e-3 for ch in chs[:nu]) and all(ch["ratio"] > 0.9 + 1e-3 for ch in chs[nu:-1])
    for k, seed in enumerate(HC.WIDE_UNAMBIGUOUS):  # where the visibility decides, it decides for the planted pose
        w = HC.wide_scene(seed)
        rot, ang, nor = HC.truth_errors(chs[2 * k]["R"], chs[2 * k]["t"], chs[2 * k]["n"], w)
        assert rot < 1e-6 and ang < 1e-6 and nor < 1e-6, (seed, rot, ang, nor)
    assert chs[-1] == dict(status=HR.DEGENERATE)
    lines, same, nine = HC.degenerate_problems()
    run = lambda p, **kw: HR.solve(p[0], p[1], HC.FOCAL, HC.CX, HC.CY, dict(HC.OPTS, **kw))
    assert run(nine)["status"] == HR.FEW_POINTS
    for p in (lines, same):
        r = run(p)
        assert r["status"] == HR.NO_HYPOTHESIS and not r["hyp"]["valid"].any()
    r = run(HC.scattered_problem(), max_pixel_error=HC.NO_INLIERS_ERROR)
    assert r["status"] == HR.NO_INLIERS and r["n_inliers"] == 0 and r["best"] == 0 and r["cost"] == 0.0
    assert run(HC.scattered_problem())["n_inliers"] >= 4


def kept_truth_errors(ref, c):
    """the planted pose against each of the two decompositions kept: the smaller deviations, and whether the chosen one
    is that one"""
    errs = [HC.truth_errors(ref["decompositions"][k]["R"], ref["decompositions"][k]["t"], ref["decompositions"][k]["n"], c)
            for k in ref["two"]]
    k = int(np.argmin([e[1] for e in errs]))
    return errs[k], ref["two"][k] == ref["choice"]


def test_reference_finds_the_planted_truth():
    worst, chosen = np.zeros(3), []
    for case in HC.SIZE_CASES:
        ref, c = HC.reference(case), HC.make_case(*case)
        e, is_chosen = kept_truth_errors(ref, c)
        chosen.append(is_chosen)
        print(f"truth {case}: rotation {e[0]:.3e} rad, direction {e[1]:.3e} rad, normal {e[2]:.3e} rad, chosen {is_chosen}")
        if case[0] < 63:
            assert TRUTH_ROT_10 / 4 < e[0] <= TRUTH_ROT_10 and TRUTH_DIR_10 / 4 < e[1] <= TRUTH_DIR_10 and \
                TRUTH_NORMAL_10 / 4 < e[2] <= TRUTH_NORMAL_10, (case, e)
            continue
        worst = np.maximum(worst, e)
        assert e[0] <= TRUTH_ROT and e[1] <= TRUTH_DIR and e[2] <= TRUTH_NORMAL, (case, e)
        assert abs(np.linalg.norm(ref["H_mlesac"]) - 1.0) < 1e-12
        # the inliers are the points that were not moved, give or take the noise's tail
        assert (ref["mask"] != ~c["outlier"]).sum() <= 0.06 * case[0], case
    print(f"truth: worst {worst}")
    assert (worst > np.array([TRUTH_ROT, TRUTH_DIR, TRUTH_NORMAL]) / 4).all()  # (twice the measurement, not more)
    assert any(chosen) and not all(chosen)  # Sampson's tie-break on a plane is decided by the noise


def test_sampler_is_the_stated_one():
    assert HR.splitmix64(0) == 0xE220A8397B1DCDAF  # the published first output of SplitMix64 seeded with 0
    for n in (4, 5, 10, 1073):
        for h in range(300):
            s = HR.sample(0, h, n)
            assert len(set(s)) == 4 and min(s) >= 0 and max(s) < n
    first = np.array([HR.sample(0, h, 1000)[0] for h in range(4000)])
    assert abs(first.mean() - 499.5) < 15  # uniform


def test_sign_of_h_does_not_matter():
    """H and -H: the same pose, the same counts, the chosen decomposition the mirrored one."""
    for p in HC.supplied_problems()[:-1]:
        a, b = HC.reference_choice(p), HC.reference_choice(dict(p, H=-p["H"]))
        assert np.abs(a["R"] - b["R"]).max() < 1e-12 and np.abs(a["t"] - b["t"]).max() < 1e-12
        assert b["choice"] == HC.mirror_index(a["choice"]) and a["ambiguous"] == b["ambiguous"]
        assert np.array_equal(b["counts_first"], a["counts_first"][[HC.mirror_index(k) for k in range(8)]])
        assert sorted(a["counts_second"]) == sorted(b["counts_second"])
        assert np.abs(np.sort(a["sampson"]) - np.sort(b["sampson"])).max() <= 1e-9 * a["sampson"].max()
    case = (65, 1)
    c, ref = HC.make_case(*case), HC.reference(case)
    x0, x1 = HC.normalised(c)
    neg = HR.refine(-ref["H_mlesac"], x0, x1, HC.FOCAL, ref["mask"], 5, 25.0)
    assert np.abs(neg["H"] + ref["refine"]["H"]).max() < 1e-12 and np.allclose(neg["sigma2"], ref["refine"]["sigma2"], rtol=1e-10)


def test_reference_notices_seeded_defects():
    """Eight one-line defects, each changing an output a test asserts."""
    case = (65, 1)
    c, ref = HC.make_case(*case), HC.reference(case)
    x0, x1 = HC.normalised(c)
    # 1 <= for < in the inlier test
    e2 = np.array([24.0, 25.0, 26.0])
    assert HR.inliers_of(e2, 25.0).tolist() == [True, False, False] and HR.inliers_of(e2, 25.0, "inlier_le").sum() == 2
    # 2 rank ceil(m / 2) - 1 for floor(m / 2): another sigma^2 for an even m
    e = np.array([4.0, 1.0, 3.0, 2.0])
    assert HR.sigma_squared(e) == pytest.approx((4.6851 * 1.4826 * 3.5) ** 2 * 3.0, rel=1e-12)
    assert HR.sigma_squared(e, "median_rank") < 0.7 * HR.sigma_squared(e)
    odd = np.append(e, 5.0)
    assert HR.sigma_squared(odd) == HR.sigma_squared(odd, "median_rank")  # (odd m: the same element)
    # 3 the inlier set recomputed between rounds: points come in once H is refined, and sigma^2 moves
    tight = ((255, 2), HC.opt_items(max_pixel_error=2.0))  # (a listed run: at 2 px the refined H admits more points)
    kept = HC.reference(*tight)
    bad = HC.run_reference(HC.make_case(*tight[0]), HC.merged(tight[1]), "inliers_recomputed")
    d = np.abs(bad["refine"]["sigma2"] - kept["refine"]["sigma2"]) / kept["refine"]["sigma2"]
    assert d[0] < 1e-12 and d[1:].max() > 100 * SIGMA_LIMIT, d
    # 4 the prior dropped: the system is singular along H itself
    bad = HR.refine(ref["H_mlesac"], x0, x1, HC.FOCAL, ref["mask"], 1, 25.0, "no_prior")["H"][0]
    good = ref["refine"]["H"][0]
    assert not np.isfinite(bad).all() or abs(np.linalg.norm(bad) - np.linalg.norm(good)) > 1e-3
    # 5 d^2 for d in the decomposition: a rotation far from the planted one
    good_rot = kept_truth_errors(ref, c)[0][0]
    bad = HR.choose(ref["H_refined"], x0, x1, ref["mask"], 25.0, "d_squared")
    rots = [HC.rot_angle(bad["decompositions"][k]["R"], c["R_true"]) for k in bad["two"]]
    assert good_rot <= TRUTH_ROT and min(rots) > 2 * TRUTH_ROT
    # 6 the sign in Eq. 14: t points elsewhere
    w = HC.wide_scene(0)
    p = dict(uv0=w["uv0"], uv1=w["uv1"], H=w["H"], mask=np.ones(80, dtype=bool))
    good, bad = HC.reference_choice(p), HC.reference_choice(p, defect="eq14_sign")
    assert good["choice"] == bad["choice"] < 4 and HC.angle(good["t"], w["t_true"]) < 1e-6 < 0.1 < HC.angle(bad["t"], w["t_true"])
    # 7 the sort's tie rule: the four of equal first count in another order
    bad = HR.choose(ref["H_refined"], x0, x1, ref["mask"], 25.0, "tie_rule")
    assert ref["kept"].tolist() == sorted(ref["kept"]) and bad["kept"].tolist() == sorted(ref["kept"])[::-1]
    # 8 the Sampson cap: it binds once max_pixel_error is small (the sums are in camera-plane units)
    good, bad = HC.reference_choice(HC.cap_problem(), HC.CAP_ERROR), HC.reference_choice(HC.cap_problem(), HC.CAP_ERROR, "sampson_cap")
    assert good["ambiguous"] and (bad["sampson"] > 1.5 * good["sampson"]).all()


def compile_cxx(tmp_path, name, flags=(), link=True):
    exe = str(tmp_path / name)
    libdir = os.path.join(ROOT, "sim3opt_amd")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cxx", name + ".cpp")]
    if link:
        cmd += ["-L" + libdir, "-lsim3opt", "-Wl,-rpath," + libdir]
    subprocess.check_call(cmd + ["-o", exe])
    return exe


def points_text(uv0, uv1):
    return "".join(" ".join(repr(float(x)) for x in (*a, *b)) + "\n" for a, b in zip(uv0, uv1))


def run_driver(exe, mode, text):
    out = subprocess.run([exe, mode], input=text, capture_output=True, text=True)
    assert out.returncode == 0 and not out.stderr, out.stderr  # (a sanitizer report lands in stderr)
    return [[float(x) for x in ln.split()] for ln in out.stdout.splitlines()]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """tests/cxx/homography_math_driver.cpp: a stand-alone program under the address and undefined-behaviour sanitizers"""
    return compile_cxx(tmp_path_factory.mktemp("homography"), "homography_math_driver",
                       flags=("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                              "-Wno-unknown-pragmas"), link=False)


def head_of(o, n):
    return f"{HC.FOCAL!r} {HC.CX!r} {HC.CY!r} {o['seed']} {o['iterations']} {n}"


def driver_hypotheses(exe, case, items):
    """the host build's hypotheses of a run: (sample (H, 4), valid (H,), H (H, 3, 3), cost (H,))"""
    c, o = HC.make_case(*case), HC.merged(items)
    rows = np.array(run_driver(exe, "hyp", head_of(o, case[0]) + "\n" + points_text(c["uv0"], c["uv1"])))
    return rows[:, :4].astype(int), rows[:, 4].astype(bool), rows[:, 5:14].reshape(-1, 3, 3), rows[:, 14]


def parse_choice(rows):
    """the driver's choice lines -> dict as homography_ref.choose's"""
    if int(rows[0][0]) != HR.OK:
        return dict(status=int(rows[0][0]))
    dec = np.array(rows[1:9])
    return dict(status=HR.OK, dec=dec, counts_first=np.array(rows[9], dtype=int), kept=np.array(rows[10], dtype=int),
                counts_second=np.array(rows[11], dtype=int), choice=int(rows[12][0]), ambiguous=bool(rows[12][1]),
                sampson=np.array(rows[12][2:]), pose=np.array(rows[13]))


def compare_choice(got, ref, what):
    """counts, kept, choice and branch exactly; the eight decompositions, the Sampson sums and the pose within
    POSE_LIMIT; returns the largest deviations of (R, t / |t|)"""
    assert got["status"] == ref["status"] == HR.OK, what
    for k in ("counts_first", "kept", "counts_second"):
        assert np.array_equal(got[k], ref[k]), (what, k, got[k], ref[k])
    assert got["choice"] == ref["choice"] and got["ambiguous"] == ref["ambiguous"], what
    for k, o in enumerate(ref["decompositions"]):
        scale = np.linalg.norm(o["t"])
        assert np.abs(got["dec"][k][:9].reshape(3, 3) - o["R"]).max() < POSE_LIMIT, (what, k)
        assert np.abs(got["dec"][k][9:12] - o["t"]).max() < POSE_LIMIT * scale, (what, k)
        assert np.abs(got["dec"][k][12:15] - o["n"]).max() < POSE_LIMIT and abs(got["dec"][k][15] - o["d"]) < POSE_LIMIT
    if ref["ambiguous"]:
        assert np.abs(got["sampson"] - ref["sampson"]).max() < 1e-6 * ref["sampson"].max(), what
    else:
        assert (got["sampson"] == 0).all()
    dR = np.abs(HR.quat_to_R(got["pose"][:4]) - ref["R"]).max()
    dt = np.abs(got["pose"][4:] - ref["t"]).max() / np.linalg.norm(ref["t"])
    assert dR < POSE_LIMIT and dt < POSE_LIMIT, (what, dR, dt)
    return dR, dt


def test_hypotheses_on_the_host_match_the_reference(driver):
    """The sampler and the four-point homography, the statements the kernel runs, compiled for the host: the same samples
    in every run; on well-conditioned hypotheses the same validity and H within H_LIMIT of the SVD null vector; an
    invalid hypothesis is the identity; the MLESAC cost within the summation bound."""
    dev = []
    for case, items in HC.RUNS:
        hyp, well = HC.reference(case, items)["hyp"], HC.conditioning(case, items)
        smp, valid, H, cost = driver_hypotheses(driver, case, items)
        assert np.array_equal(smp, hyp["sample"]) and np.isfinite(H).all(), (case, items)
        assert np.array_equal(valid[well], hyp["valid"][well]), (case, items)
        assert (H[~valid] == np.eye(3)).all() and (np.abs(np.linalg.norm(H[valid], axis=(1, 2)) - 1.0) < 1e-14).all()
        use = well & hyp["valid"]
        d = HC.same_up_to_sign(H, hyp["H"])[use]
        dev += list(d)
        assert d.max() < H_LIMIT, (case, items, d.max())
        if HC.merged(items)["max_pixel_error"] == 5.0:
            assert (np.abs(cost - hyp["cost"])[use] <= 1e-9 * hyp["cost"][use]).all(), (case, items)
    dev = np.array(dev)
    print(f"host build against the restatement, {len(dev)} hypotheses: worst |dH| {dev.max():.3e}, median "
          f"{np.median(dev):.3e}, 99th percentile {np.percentile(dev, 99):.3e}")
    assert dev.max() > H_MEASURED / 32  # (the limit rests on a measurement of this code, not of something more exact)


def test_whole_solves_on_the_host_match_the_reference(driver):
    """Error, inlier set, refinement rounds, decomposition and choice of homography_math.hpp on the host against the
    restatement over every listed run: best hypothesis, mask, counts, choice and branch exactly; sigma^2, H of every
    round and the pose within their limits."""
    worst = np.zeros(4)
    for case, items in HC.RUNS:
        c, o, ref = HC.make_case(*case), HC.merged(items), HC.reference(case, items)
        x0, x1 = HC.normalised(c)
        rows = run_driver(driver, "solve", head_of(o, case[0]) + f" {o['max_pixel_error']!r} {o['refine_rounds']}\n" +
                          points_text(c["uv0"], c["uv1"]))
        assert int(rows[0][0]) == ref["best"] and int(rows[0][2]) == ref["n_inliers"], (case, items)
        assert abs(rows[0][1] - ref["cost"]) <= 1e-9 * ref["cost"]
        assert np.array_equal(np.array(rows[1], dtype=int).astype(bool), ref["mask"]), (case, items)
        Hm = np.array(rows[2]).reshape(3, 3)
        sgn = 1.0 if (Hm * ref["H_mlesac"]).sum() > 0 else -1.0  # (the null vector's sign is open)
        assert np.abs(Hm - sgn * ref["H_mlesac"]).max() < H_LIMIT
        R = o["refine_rounds"]
        rr = np.array(rows[3:3 + R])
        ds = (np.abs(rr[:, 0] - ref["refine"]["sigma2"]) / ref["refine"]["sigma2"]).max()
        dh = np.abs(rr[:, 1:].reshape(-1, 3, 3) - sgn * ref["refine"]["H"]).max()
        assert ds < SIGMA_LIMIT and dh < REFINED_LIMIT, (case, items, ds, dh)
        exp = ref if sgn > 0 else HR.choose(-ref["H_refined"], x0, x1, ref["mask"], o["max_pixel_error"] ** 2)
        dR, dt = compare_choice(parse_choice(rows[3 + R:]), exp, (case, items))
        worst = np.maximum(worst, [ds, dh, dR, dt])
    print(f"host build against the restatement: worst sigma^2 {worst[0]:.3e} (relative), refined H {worst[1]:.3e}, "
          f"R {worst[2]:.3e}, t {worst[3]:.3e} (relative)")
    assert worst[0] > SIGMA_MEASURED / 32 and worst[1] > REFINED_MEASURED / 32 and worst[3] > POSE_MEASURED / 32


def test_decomposition_on_the_host_matches_the_reference(driver):
    """Both branches, both signs of H and the exactly degenerate identity through the host build."""
    for k, p in enumerate(HC.supplied_problems()):
        text = f"{HC.FOCAL!r} {HC.CX!r} {HC.CY!r} 0 0 {len(p['uv0'])} 5.0 0\n" + points_text(p["uv0"], p["uv1"]) + \
            " ".join(repr(float(x)) for x in p["H"].reshape(9)) + "\n" + " ".join(str(int(x)) for x in p["mask"]) + "\n"
        got, ref = parse_choice(run_driver(driver, "decompose", text)), HC.reference_choice(p)
        if ref["status"] == HR.DEGENERATE:
            assert got == dict(status=HR.DEGENERATE) and k == len(HC.supplied_problems()) - 1
        else:
            compare_choice(got, ref, k)


def test_defaults_are_the_references():
    o = L.HomographyBatchOptions()
    L.load().sim3opt_homography_batch_options_default(ctypes.byref(o))
    got = {k: getattr(o, k) for k, _ in L.HomographyBatchOptions._fields_}
    assert got == dict(HR.DEFAULTS, device=-1)
    assert len(HOM_SYMBOLS) == 16
    assert (L.HOMOGRAPHY_OK, L.HOMOGRAPHY_FEW_POINTS, L.HOMOGRAPHY_NO_HYPOTHESIS, L.HOMOGRAPHY_NO_INLIERS,
            L.HOMOGRAPHY_DEGENERATE) == (HR.OK, HR.FEW_POINTS, HR.NO_HYPOTHESIS, HR.NO_INLIERS, HR.DEGENERATE)


def small_batch():
    a = HC.batch_arrays(((10, 1),))
    a = dict(point_ptr=np.array([0, 9, 12, 15], dtype=np.int32), uv0=np.tile(a["uv0"], (2, 1))[:15],
             uv1=np.tile(a["uv1"], (2, 1))[:15])  # 9, 3 and 3 points
    b = L.HomographyBatch()
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
    assert e.value.code == L.ERR_ARG and "homography_batch_set_problems" in str(e.value)
    assert b.dims() == (3, 15)


@pytest.mark.parametrize("kw", [dict(iterations=0), dict(iterations=4097), dict(max_pixel_error=0.0),
                                dict(max_pixel_error=float("inf")), dict(max_pixel_error=float("nan")),
                                dict(refine_rounds=-1), dict(refine_rounds=9), dict(min_points=3)])
def test_set_options_refuses_and_changes_nothing(kw):
    _, b = small_batch()
    before = b.options()
    with pytest.raises(L.Sim3OptError) as e:
        b.set_options(**kw)
    assert e.value.code == L.ERR_ARG and "value out of range" in str(e.value)
    assert b.options() == before and b.dims() == (3, 15)
    b.set_options(iterations=4096, min_points=4, refine_rounds=8, seed=2 ** 64 - 1)  # the ends of the ranges are taken
    assert b.options()["seed"] == 2 ** 64 - 1 and b.tiles() == (HC.LDS_POINTS, HC.CHUNK)
    b.set_options(refine_rounds=0)
    assert b.options()["refine_rounds"] == 0


def test_state_and_argument_errors_before_a_solve():
    _, b = small_batch()
    for call in (b.poses, b.homographies, b.inliers, b.summary, lambda: b.debug_hypotheses(0)):
        with pytest.raises(L.Sim3OptError) as e:
            call()
        assert e.value.code == L.ERR_STATE
    with pytest.raises(L.Sim3OptError) as e:
        L.HomographyBatch().solve()
    assert e.value.code == L.ERR_STATE and "no problems set" in str(e.value)
    lib, nul = L.load(), None
    assert lib.sim3opt_homography_batch_debug_score(b._b, 0, nul, nul, nul) == L.ERR_ARG
    assert lib.sim3opt_homography_batch_debug_refine(b._b, nul, nul, nul, nul) == L.ERR_ARG
    assert lib.sim3opt_homography_batch_debug_decompose(b._b, nul, nul, nul, nul, nul, nul, nul, nul, nul, nul, nul) == L.ERR_ARG
    assert lib.sim3opt_homography_batch_get_poses(b._b, nul) == L.ERR_ARG
    assert lib.sim3opt_homography_batch_get_homographies(b._b, nul, nul) == L.ERR_ARG
    assert lib.sim3opt_homography_batch_get_inliers(b._b, nul, nul) == L.ERR_ARG
    assert lib.sim3opt_homography_batch_solve(nul) == L.ERR_ARG and lib.sim3opt_homography_batch_dims(nul, nul, nul, nul) == L.ERR_ARG
    nan_H = np.full((3, 1, 3, 3), np.nan)
    ones = np.ones(15, dtype=np.uint8)
    for call in (lambda: b.debug_score(nan_H), lambda: b.debug_refine(nan_H, ones), lambda: b.debug_decompose(nan_H, ones)):
        with pytest.raises(L.Sim3OptError) as e:
            call()
        assert e.value.code == L.ERR_ARG and "non-finite matrix" in str(e.value)
    with pytest.raises(ValueError):
        b.debug_refine(np.zeros((2, 3, 3)), ones)
    with pytest.raises(ValueError):
        b.debug_decompose(np.zeros((3, 3, 3)), ones[:14])


def test_fails_loudly_without_gpu():
    if gpu_available():
        pytest.skip("GPU present: covered by the gpu tests")
    _, b = small_batch()
    H = np.tile(np.eye(3), (3, 1, 1, 1))
    ones = np.ones(15, dtype=np.uint8)
    for call in (b.solve, lambda: b.debug_score(H), lambda: b.debug_refine(H, ones), lambda: b.debug_decompose(H, ones)):
        with pytest.raises(L.Sim3OptError) as e:
            call()
        assert e.value.code == L.ERR_NO_DEVICE and "no usable HIP device" in str(e.value)
    assert b.dims() == (3, 15)


# the listed cases in which the restatement's choice is the planted pose (test_reference_finds_the_planted_truth prints
# which): the device's pose is within POSE_LIMIT of the restatement's, which the bounds are twice the measurement of
CONFORMANCE_CASES = ((63, 1), (255, 1), (256, 1), (257, 1), (1071, 1), (1073, 1))


def compile_conformance(tmp_path):
    return compile_cxx(tmp_path, "homography_conformance")


def write_conformance_file(path, cases):
    """The candidates of `cases` as the detector has them (points1, points2), each followed by the planted rotation
    and unit translation; the hypothesis count of OPTS and the bounds of test_reference_finds_the_planted_truth in the
    first line."""
    with open(path, "w") as f:
        w = lambda *v: f.write(" ".join(repr(float(x)) if not isinstance(x, (int, np.integer)) else str(x)
                                        for x in v) + "\n")
        w(len(cases), HC.FOCAL, HC.CX, HC.CY, HC.OPTS["iterations"], TRUTH_ROT, TRUTH_DIR)
        for c in cases:
            case = HC.make_case(*c)
            w(c[0])
            for a, b in zip(case["uv0"], case["uv1"]):
                w(*a, *b)
            w(*case["R_true"].reshape(9), *case["t_true"])


def test_conformance_cases_are_those_the_choice_gets_right():
    for c in CONFORMANCE_CASES:
        assert kept_truth_errors(HC.reference(c), HC.make_case(*c))[1], c


def test_conformance_host_part(tmp_path):
    """include/sim3opt_homography.hpp compiles -Werror beside sim3opt_essential.hpp without Eigen, OpenCV or TooN; its
    add() / solve() refusals and the C-ABI's leave everything as it was."""
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
