"""The batched homography stage on the GPU (sim3opt_homography_batch, sim3opt_amd/csrc/homography_batch.hip: one
workgroup per problem; MLESAC hypotheses, inliers, refinement rounds, decomposition and choice in one launch) against
tests/homography_ref.py, an independent restatement with other linear algebra.  PARITY UNPINNED (the reference cannot
be built here): what is compared is the restatement and planted truth.  The cases and their reference runs are
tests/homography_cases.py's; tests/test_homography_ref.py shows on the CPU that the conditions these comparisons rest on
hold for them, and sets the limits from the host build of the kernel's arithmetic against the restatement.  Real inputs, the KITTI 00 keyframes, run in
tests/test_gpu_real_keyframes.py."""
import subprocess

import numpy as np
import pytest

import homography_cases as HC
import homography_ref as HR
import test_homography_ref as TH
from sim3opt_amd import lib as L

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
HYP_FIELDS = ("sample", "n_solutions", "valid", "H", "count", "cost")
SUMMARY_FIELDS = ("n_inliers", "status", "best_hypothesis", "cost_hypothesis", "sigma2", "counts_first", "kept",
                  "counts_second", "choice", "ambiguous", "sampson")


def run_batch(cases, arrays=None, **opts):
    a = HC.batch_arrays(cases) if arrays is None else arrays
    b = L.HomographyBatch(**dict(dict(iterations=HC.OPTS["iterations"]), **opts))
    b.set_problems(**a)
    b.solve()
    return b


def snapshot(b):
    """Everything a solve returns, the hypotheses' read-out included, as arrays that can be compared bit for bit."""
    n = b.dims()[0]
    mask, _ = b.inliers()
    hm, hr = b.homographies()
    hyp = [b.debug_hypotheses(k) for k in range(n)]
    return dict(poses=b.poses(), H_mlesac=hm, H_refined=hr, mask=mask, hyp=hyp, **b.summary())


def problem_of(snap, ptr, k):
    """Problem k's share of a snapshot."""
    lo, hi = int(ptr[k]), int(ptr[k + 1])
    return [snap["poses"][k], snap["H_mlesac"][k], snap["H_refined"][k], snap["mask"][lo:hi]] + \
        [snap[f][k:k + 1] for f in SUMMARY_FIELDS] + [snap["hyp"][k][f] for f in HYP_FIELDS]


def same_bits(x, y):
    return all(a.shape == b.shape and a.tobytes() == b.tobytes() for a, b in zip(x, y))


_default_run = {}


def default_run():
    """SIZE_CASES as one batch under OPTS: solved once, shared; do not modify."""
    if not _default_run:
        a = HC.batch_arrays(HC.SIZE_CASES)
        b = run_batch(HC.SIZE_CASES, a)
        _default_run.update(arrays=a, batch=b, snap=snapshot(b))
    return _default_run["arrays"], _default_run["batch"], _default_run["snap"]


def expected_choice(ref, H_dev, c, opts):
    """The restatement's choice for the sign the device's H came out with (the null vector's sign is open, and with -H
    the decompositions change places, include/sim3opt.h): (sign, choice dict)"""
    sgn = 1.0 if (H_dev * ref["H_mlesac"]).sum() > 0 else -1.0
    if sgn > 0:
        return sgn, ref
    x0, x1 = HC.normalised(c)
    return sgn, HR.choose(-ref["H_refined"], x0, x1, ref["mask"], opts["max_pixel_error"] ** 2)


def check_choice(got, k, exp, what):
    """Problem k of a summary or of the decomposition operator against the restatement's choice: counts, kept, choice and
    branch exactly, the Sampson sums to 1e-6, the pose within POSE_LIMIT"""
    for f in ("counts_first", "kept", "counts_second"):
        assert np.array_equal(got[f][k], exp[f]), (what, f, got[f][k], exp[f])
    assert got["choice"][k] == exp["choice"] and bool(got["ambiguous"][k]) == exp["ambiguous"], what
    if exp["ambiguous"]:
        assert np.abs(got["sampson"][k] - exp["sampson"]).max() < 1e-6 * exp["sampson"].max(), what
    else:
        assert (got["sampson"][k] == 0).all(), what
    pose = got["poses"][k] if "poses" in got else got["pose"][k]
    dR = np.abs(HR.quat_to_R(pose[:4]) - exp["R"]).max()
    dt = np.abs(pose[4:] - exp["t"]).max() / np.linalg.norm(exp["t"])
    assert dR < TH.POSE_LIMIT and dt < TH.POSE_LIMIT, (what, dR, dt)
    assert abs(np.linalg.norm(pose[:4]) - 1.0) < 1e-14
    return dR, dt


def check_whole_solve(snap, ptr, k, case, items=()):
    """Problem k of a solve against homography_ref's run of `case`: status, best hypothesis (or its twin), inlier count
    and mask, counts, choice and branch exactly; both H, sigma^2 and the pose within their limits; the planted truth
    within its bounds."""
    ref, opts, c = HC.reference(case, items), HC.merged(items), HC.make_case(*case)
    lo, hi = int(ptr[k]), int(ptr[k + 1])
    hyp, best = ref["hyp"], ref["best"]
    assert snap["status"][k] == ref["status"] == HR.OK, (case, items)
    twins = (HC.same_up_to_sign(hyp["H"], np.broadcast_to(hyp["H"][best], hyp["H"].shape)) < 1e-9) & hyp["valid"]
    assert twins[best] and twins[snap["best_hypothesis"][k]], (case, items, snap["best_hypothesis"][k], best)
    assert abs(snap["cost_hypothesis"][k] - ref["cost"]) <= 1e-9 * ref["cost"], (case, items)
    assert snap["n_inliers"][k] == ref["n_inliers"] and np.array_equal(snap["mask"][lo:hi].astype(bool), ref["mask"]), (case, items)
    Hm, Hr = snap["H_mlesac"][k], snap["H_refined"][k]
    assert np.array_equal(Hm, snap["hyp"][k]["H"][snap["best_hypothesis"][k]])
    sgn, exp = expected_choice(ref, Hm, c, opts)
    dm, dr = np.abs(Hm - sgn * ref["H_mlesac"]).max(), np.abs(Hr - sgn * ref["H_refined"]).max()
    ds = (np.abs(snap["sigma2"][k] - ref["refine"]["sigma2"]) / ref["refine"]["sigma2"]).max()
    assert dm < TH.H_LIMIT and dr < TH.REFINED_LIMIT and ds < TH.SIGMA_LIMIT, (case, items, dm, dr, ds)
    dR, dt = check_choice(snap, k, exp, (case, items))
    print(f"whole solve {case} {dict(items)}: |dHm| {dm:.3e}, |dHr| {dr:.3e}, sigma^2 {ds:.3e}, |dR| {dR:.3e}, |dt| {dt:.3e}")
    # the planted pose is one of the two kept (tests/test_homography_ref.py), within the bounds measured there
    pose = snap["poses"][k]
    e, chosen = TH.kept_truth_errors(exp, c)
    lim = (TH.TRUTH_ROT, TH.TRUTH_DIR) if case[0] >= 63 else (TH.TRUTH_ROT_10, TH.TRUTH_DIR_10)
    assert e[0] <= lim[0] and e[1] <= lim[1], (case, items, e)
    if chosen:
        assert HC.rot_angle(HR.quat_to_R(pose[:4]), c["R_true"]) <= lim[0] and HC.angle(pose[4:], c["t_true"]) <= lim[1]


def test_scoring_operator():
    """sim3opt_homography_batch_debug_score at every point count on the planted H, every hypothesis of the reference and
    the identity: every count is the problem's point count, the costs are the restatement's within the summation bound
    (the per-point errors are the same operations in the same order; only the order of the sum differs).  The
    read-out leaves the last results as they were."""
    a, b, snap = default_run()
    Hs = np.stack([HC.score_matrices(c) for c in HC.SIZE_CASES])
    n = len(HC.SIZE_CASES)
    before = sum((problem_of(snap, a["point_ptr"], k) for k in range(n)), [])
    count, cost = b.debug_score(Hs)
    assert same_bits(before, sum((problem_of(snapshot(b), a["point_ptr"], k) for k in range(n)), []))
    assert np.isfinite(cost).all()
    for k, case in enumerate(HC.SIZE_CASES):
        x0, x1 = HC.normalised(HC.make_case(*case))
        e2, _ = HR.sq_error(Hs[k], x0, x1, HC.FOCAL)
        # (tests/test_homography_ref.py: no e2 of these matrices lies at the cap, where rounding could take either side)
        want, _ = HR.mlesac_cost(e2, 25.0)
        assert (count[k] == case[0]).all(), case
        assert (np.abs(cost[k] - want) <= 4 * EPS * case[0] * want).all(), (case, np.abs(cost[k] - want).max())
        if case[0] >= 63:  # the planted H costs less than any hypothesis from four noisy points, far less than the identity
            assert cost[k, 0] < cost[k, 1:-1].min() * 1.5 and cost[k, 0] < 0.5 * cost[k, -1], case


def test_hypotheses():
    """sim3opt_homography_batch_debug_hypotheses against the restatement's: the same sample for every h; on
    well-conditioned hypotheses the same validity and H within H_LIMIT up to sign; an invalid hypothesis is the
    identity with count and cost zero; count and cost of every valid one are the restatement's scoring."""
    _, _, snap = default_run()
    for k, case in enumerate(HC.SIZE_CASES):
        ref, dev, well = HC.reference(case)["hyp"], snap["hyp"][k], HC.conditioning(case)
        valid = dev["valid"].astype(bool)
        assert np.array_equal(dev["sample"], ref["sample"]), case
        assert np.isfinite(dev["H"]).all() and np.isfinite(dev["cost"]).all()
        assert np.array_equal(valid[well], ref["valid"][well]) and np.array_equal(dev["n_solutions"], dev["valid"]), case
        assert (dev["H"][~valid] == np.eye(3)).all() and (dev["count"][~valid] == 0).all() and (dev["cost"][~valid] == 0).all()
        assert (dev["count"][valid] == case[0]).all(), case
        use = well & ref["valid"]
        assert HC.same_up_to_sign(dev["H"], ref["H"])[use].max() < TH.H_LIMIT, case
        assert (np.abs(dev["cost"] - ref["cost"])[use] <= 1e-9 * ref["cost"][use]).all(), case
    assert not snap["hyp"][len(HC.SIZE_CASES) - 1]["valid"].all()  # (the repeated matches: some samples are refused)


def test_hypotheses_have_the_host_builds_bits(tmp_path):
    """The stage is compiled without fused multiply-add so that a hypothesis has on the device the bits it has in the
    host build of homography_math.hpp (tests/cxx/homography_math_driver.cpp): sample, validity and every entry of H are
    compared bit for bit over every listed run."""
    exe = TH.compile_cxx(tmp_path, "homography_math_driver", flags=("-O2", "-Wno-unknown-pragmas"), link=False)
    for case, items in HC.RUNS:
        dev = run_batch((case,), **dict(items)).debug_hypotheses(0)
        smp, valid, H, _ = TH.driver_hypotheses(exe, case, items)
        assert np.array_equal(dev["sample"], smp) and np.array_equal(dev["valid"].astype(bool), valid), (case, items)
        assert dev["H"].tobytes() == np.ascontiguousarray(H).tobytes(), (case, items)


def test_degenerate_samples_are_invalid_and_leave_no_nan():
    """Collinear and repeated points: every sample is refused, the hypotheses read as the identity, the problem ends
    with NO_HYPOTHESIS and finite results; a healthy problem with repeated matches refuses exactly the samples that
    hold a repeat."""
    lines, same, _ = HC.degenerate_problems()
    dup = HC.make_case(66, 2, "dup")
    a = HC.arrays_of([lines, same, (dup["uv0"], dup["uv1"])])
    b = run_batch(None, a)
    s = snapshot(b)
    assert s["status"].tolist() == [HR.NO_HYPOTHESIS, HR.NO_HYPOTHESIS, HR.OK]
    for k in range(2):
        h = s["hyp"][k]
        assert not h["valid"].any() and (h["H"] == np.eye(3)).all() and (h["cost"] == 0).all()
        assert (s["poses"][k] == [0, 0, 0, 1, 0, 0, 0]).all() and (s["H_mlesac"][k] == 0).all()
    assert (s["mask"][:24] == 0).all() and all(np.isfinite(s[f]).all() for f in ("poses", "H_mlesac", "H_refined", "sigma2"))
    h = s["hyp"][2]
    pairs = {(k, k + 1) for k in range(0, 65, 4)}
    repeat = np.array([any((i, j) in pairs for i in smp for j in smp) for smp in h["sample"]])
    assert repeat.any() and np.array_equal(~h["valid"].astype(bool), repeat)


def refine_problems():
    """what the refinement operator is given: every size case with the restatement's MLESAC H and inliers (even and
    odd m, around the wavefront, the stride and the staging cap, tied errors), and the planted H on a listed case's true
    inliers"""
    probs = [(c, HC.reference(c)["H_mlesac"], HC.reference(c)["mask"]) for c in HC.SIZE_CASES]
    c = (257, 1)
    probs.append((c, HC.true_homography(HC.make_case(*c)), ~HC.make_case(*c)["outlier"]))
    return probs


def test_refinement_operator():
    """sim3opt_homography_batch_debug_refine: sigma^2 and H after every round against the restatement's rounds from the
    same H on the same set.  A set of fewer than four points gives zeros."""
    probs = refine_problems()
    a = HC.batch_arrays([p[0] for p in probs])
    b = L.HomographyBatch()
    b.set_problems(**a)
    out = b.debug_refine(np.stack([p[1] for p in probs]), np.concatenate([p[2] for p in probs]))
    ms = set()
    for k, (case, H, mask) in enumerate(probs):
        x0, x1 = HC.normalised(HC.make_case(*case))
        ref = HR.refine(H, x0, x1, HC.FOCAL, mask, 5, 25.0)
        ds = (np.abs(out["sigma2"][k] - ref["sigma2"]) / ref["sigma2"]).max()
        dh = np.abs(out["H"][k] - ref["H"]).max()
        print(f"refinement {case}: m {int(mask.sum())}, sigma^2 {ds:.3e}, |dH| {dh:.3e}")
        assert ds < TH.SIGMA_LIMIT and dh < TH.REFINED_LIMIT, (case, ds, dh)
        ms.add(int(mask.sum()) % 2)
    assert ms == {0, 1}
    few = np.concatenate([p[2] for p in probs])
    few[:10] = [1, 1, 1] + [0] * 7
    out = b.debug_refine(np.stack([p[1] for p in probs]), few)
    assert (out["sigma2"][0] == 0).all() and (out["H"][0] == 0).all() and (out["sigma2"][1] > 0).all()
    b.set_options(refine_rounds=2)
    two = b.debug_refine(np.stack([p[1] for p in probs]), np.concatenate([p[2] for p in probs]))
    assert two["H"].shape == (len(probs), 2, 3, 3) and two["sigma2"].shape == (len(probs), 2)


def test_decomposition_operator():
    """sim3opt_homography_batch_debug_decompose on the wide scenes of both branches under both signs of H, two listed
    cases and the identity: the eight decompositions, both rounds of counts, the four kept, the choice, the branch and
    the Sampson sums against the restatement; H and -H give the same pose; the identity is DEGENERATE."""
    probs = HC.supplied_problems()
    a = HC.arrays_of([(p["uv0"], p["uv1"]) for p in probs])
    b = L.HomographyBatch()
    b.set_problems(**a)
    got = b.debug_decompose(np.stack([p["H"] for p in probs]), np.concatenate([p["mask"] for p in probs]))
    branches = set()
    for k, p in enumerate(probs[:-1]):
        ref = HC.reference_choice(p)
        assert got["status"][k] == HR.OK
        check_choice(got, k, ref, k)
        for j, o in enumerate(ref["decompositions"]):
            scale = np.linalg.norm(o["t"])
            assert np.abs(got["R"][k, j] - o["R"]).max() < TH.POSE_LIMIT and np.abs(got["t"][k, j] - o["t"]).max() < TH.POSE_LIMIT * scale
            assert np.abs(got["normal"][k, j] - o["n"]).max() < TH.POSE_LIMIT and abs(got["d"][k, j] - o["d"]) < TH.POSE_LIMIT
        branches.add(bool(got["ambiguous"][k]))
    assert branches == {False, True}
    for k in range(0, 2 * len(HC.WIDE_UNAMBIGUOUS + HC.WIDE_AMBIGUOUS), 2):  # H, then -H
        assert np.abs(got["pose"][k] - got["pose"][k + 1]).max() < 1e-12, k
        assert got["choice"][k + 1] == HC.mirror_index(got["choice"][k]) and got["ambiguous"][k] == got["ambiguous"][k + 1]
        assert np.array_equal(got["counts_first"][k + 1], got["counts_first"][k][[HC.mirror_index(j) for j in range(8)]])
    last = len(probs) - 1
    assert got["status"][last] == HR.DEGENERATE and (got["pose"][last] == [0, 0, 0, 1, 0, 0, 0]).all()
    assert (got["R"][last] == 0).all() and np.isfinite(got["pose"]).all()
    # the Sampson cap binds at a small max_pixel_error (the sums are in camera-plane units)
    p = HC.cap_problem()
    c = L.HomographyBatch(max_pixel_error=HC.CAP_ERROR)
    c.set_problems(**HC.arrays_of([(p["uv0"], p["uv1"])]))
    got = c.debug_decompose(p["H"], p["mask"])
    ref, uncapped = HC.reference_choice(p, HC.CAP_ERROR), HC.reference_choice(p, HC.CAP_ERROR, "sampson_cap")
    check_choice(got, 0, ref, "cap")
    assert (uncapped["sampson"] > 1.5 * got["sampson"][0]).all()


def test_whole_solve_matches_reference():
    """Every size case in one batch under OPTS."""
    a, _, snap = default_run()
    for k, case in enumerate(HC.SIZE_CASES):
        check_whole_solve(snap, a["point_ptr"], k, case)


@pytest.mark.parametrize("case,items", HC.RUNS[len(HC.SIZE_CASES):], ids=TH.RUN_IDS)
def test_whole_solve_options(case, items):
    """The other listed runs: the hypothesis counts around the chunk and the default 300, another sampler seed, another
    max_pixel_error."""
    a = HC.batch_arrays((case,))
    snap = snapshot(run_batch((case,), a, **dict(items)))
    check_whole_solve(snap, a["point_ptr"], 0, case, items)
    assert len(snap["hyp"][0]["valid"]) == HC.merged(items)["iterations"]


def test_statuses_beside_healthy_problems():
    """FEW_POINTS and NO_HYPOTHESIS beside healthy problems in one batch: each ends with its own status, the healthy ones
    with the bits they have alone.  NO_INLIERS needs a max_pixel_error whose square is zero (a valid hypothesis fits its
    own four points), so it is a batch of its own; DEGENERATE beside healthy matrices is test_decomposition_operator."""
    lines, same, nine = HC.degenerate_problems()
    c0, c1 = HC.make_case(65, 1), HC.make_case(257, 1)
    a = HC.arrays_of([nine, (c0["uv0"], c0["uv1"]), lines, (c1["uv0"], c1["uv1"]), same])
    b = run_batch(None, a)
    s = snapshot(b)
    assert s["status"].tolist() == [HR.FEW_POINTS, HR.OK, HR.NO_HYPOTHESIS, HR.OK, HR.NO_HYPOTHESIS]
    assert s["best_hypothesis"].tolist()[0::2] == [-1, -1, -1] and (s["n_inliers"][0::2] == 0).all()
    assert (s["hyp"][0]["H"] == 0).all() and (s["hyp"][0]["sample"] == 0).all()  # (nothing ran)
    for k, case in ((1, (65, 1)), (3, (257, 1))):
        one = HC.batch_arrays((case,))
        alone = snapshot(run_batch((case,), one))
        assert same_bits(problem_of(alone, one["point_ptr"], 0), problem_of(s, a["point_ptr"], k)), case
        check_whole_solve(s, a["point_ptr"], k, case)
    z = run_batch(None, HC.arrays_of([HC.scattered_problem(), (c0["uv0"], c0["uv1"])]), max_pixel_error=HC.NO_INLIERS_ERROR)
    s = snapshot(z)
    assert s["status"].tolist() == [HR.NO_INLIERS] * 2 and (s["n_inliers"] == 0).all() and (s["mask"] == 0).all()
    assert (s["cost_hypothesis"] == 0).all() and (s["best_hypothesis"] == 0).all()  # every cost ties at zero: the first
    assert np.array_equal(s["H_mlesac"], s["H_refined"]) and (np.abs(np.linalg.norm(s["H_mlesac"], axis=(1, 2)) - 1) < 1e-14).all()


def test_problems_are_independent_of_the_batch():
    """A problem alone, first, last and among others: the same bits everywhere.  Two solves of one handle give the same
    bits; another seed, other samples."""
    a, b, snap = default_run()
    cases, ptr = HC.SIZE_CASES, a["point_ptr"]
    for k in (0, 4, len(cases) - 2):
        one = HC.batch_arrays((cases[k],))
        alone = snapshot(run_batch((cases[k],), one))
        assert same_bits(problem_of(alone, one["point_ptr"], 0), problem_of(snap, ptr, k)), cases[k]
    rev = HC.batch_arrays(cases[::-1])
    back = snapshot(run_batch(cases[::-1], rev))
    for k, case in enumerate(cases):
        assert same_bits(problem_of(back, rev["point_ptr"], len(cases) - 1 - k), problem_of(snap, ptr, k)), case
    many = tuple(cases[k % 7] for k in range(300))  # more workgroups than compute units
    am = HC.batch_arrays(many)
    sm = snapshot(run_batch(many, am, iterations=17))
    for k in range(7, 300):
        assert same_bits(problem_of(sm, am["point_ptr"], k), problem_of(sm, am["point_ptr"], k % 7)), k
    b.solve()
    again = snapshot(b)
    for k, case in enumerate(cases):
        assert same_bits(problem_of(again, ptr, k), problem_of(snap, ptr, k)), case
    other = snapshot(run_batch(cases, a, seed=777))
    want = np.array([HR.sample(777, h, cases[4][0]) for h in range(HC.OPTS["iterations"])])
    assert np.array_equal(other["hyp"][4]["sample"], want) and not np.array_equal(want, snap["hyp"][4]["sample"])


def test_memory_and_errors():
    """sim3opt_device_memory_in_use is constant across solves and the four read-outs and back at its start after
    close(); the handle holds nine blocks (the frame's eight and the squared errors of problems too large for LDS); after
    a change of size, and of options.device, it solves again to the same bytes; read-outs and refused calls leave the last
    results bit for bit."""
    start = L.device_memory_in_use()
    cases = (HC.SIZE_CASES[3], HC.SIZE_CASES[9], HC.SIZE_CASES[4])  # (one of them beyond the staging cap)
    a = HC.batch_arrays(cases)
    b = L.HomographyBatch(iterations=HC.OPTS["iterations"])
    b.set_problems(**a)
    assert b.solve() == 3
    held = L.device_memory_in_use()
    assert held[1] > start[1] and held[0] - start[0] == 9
    first = snapshot(b)
    flat = lambda s: sum((problem_of(s, a["point_ptr"], k) for k in range(3)), [])
    b.solve()
    assert L.device_memory_in_use() == held
    b.debug_hypotheses(1)
    b.debug_score(np.stack([HC.score_matrices(c) for c in cases]))
    b.debug_refine(first["H_mlesac"], first["mask"])
    b.debug_decompose(first["H_refined"], first["mask"])
    assert L.device_memory_in_use() == held
    assert same_bits(flat(snapshot(b)), flat(first))  # the read-outs left the results as they were
    for kw in (dict(iterations=0), dict(max_pixel_error=0.0), dict(refine_rounds=9), dict(min_points=3)):
        with pytest.raises(L.Sim3OptError) as e:
            b.set_options(**kw)
        assert e.value.code == L.ERR_ARG and "homography_batch_set_options: value out of range" in str(e.value), kw
    bad = {k: np.array(v) for k, v in a.items()}
    bad["uv1"][5, 1] = np.nan
    with pytest.raises(L.Sim3OptError) as e:
        b.set_problems(**bad)
    assert e.value.code == L.ERR_ARG and "non-finite observation" in str(e.value)
    with pytest.raises(L.Sim3OptError) as e:
        b.debug_hypotheses(3)
    assert e.value.code == L.ERR_ARG and "no such problem" in str(e.value)
    assert same_bits(flat(snapshot(b)), flat(first)) and L.device_memory_in_use() == held
    # another size and back (the first use after it a read-out, not a solve), another device setting and back
    b.set_problems(**HC.batch_arrays(cases[:2]))
    b.debug_refine(first["H_mlesac"][:2], first["mask"][:int(a["point_ptr"][2])])
    assert b.solve() == 2 and L.device_memory_in_use()[0] == held[0] and L.device_memory_in_use()[1] < held[1]
    b.set_problems(**a)
    b.solve()
    assert L.device_memory_in_use() == held and same_bits(flat(snapshot(b)), flat(first))
    b.set_options(iterations=HC.OPTS["iterations"], device=0)
    assert L.device_memory_in_use()[0] == start[0]  # the blocks went with the device setting
    b.solve()
    assert L.device_memory_in_use() == held and same_bits(flat(snapshot(b)), flat(first))
    b.close()
    assert L.device_memory_in_use() == start


def test_match_batch_arrays_are_accepted_as_they_are():
    """MatchBatch's match_ptr, uv0 and uv1 go into set_problems unchanged (the frame's set_problems)."""
    import match_cases as MC

    c = MC.ratio()
    M = L.MatchBatch(**c["options"])
    M.set_frames(**MC.frame_arrays(c["frames"]), **c["intr"])
    M.set_pairs(c["pairs"])
    M.solve()
    mt, ptr = M.matches(), np.unique(M.match_ptr())  # (pairs without a match own no rows: the arrays stay as they are)
    assert len(ptr) > 10 and ptr[0] == 0
    b = L.HomographyBatch(iterations=HC.OPTS["iterations"], min_points=4)
    b.set_problems(ptr, mt["uv0"], mt["uv1"], c["intr"]["focal"], c["intr"]["cx"], c["intr"]["cy"])
    assert b.dims() == (len(ptr) - 1, int(ptr[-1]))
    b.solve()
    s, (mask, cnt) = b.summary(), b.inliers()
    assert set(s["status"].tolist()) <= {HR.OK, HR.FEW_POINTS, HR.NO_HYPOTHESIS, HR.NO_INLIERS, HR.DEGENERATE}
    assert np.array_equal(cnt, np.add.reduceat(mask.astype(np.int32), ptr[:-1])) and np.isfinite(b.poses()).all()


def test_cxx_conformance(tmp_path):
    """tests/cxx/homography_conformance.cpp: HomographyBatch's rotations and unit translations are within the bounds
    tests/test_homography_ref.py measured, through the restatement, of the planted truth; good() holds; its inlier count
    is its mask's."""
    exe = TH.compile_conformance(tmp_path)
    path = str(tmp_path / "candidates.txt")
    TH.write_conformance_file(path, TH.CONFORMANCE_CASES)
    r = subprocess.run([exe, "run", path], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 failed" in r.stdout, r.stdout + r.stderr
