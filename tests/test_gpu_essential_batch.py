"""The batched essential-matrix RANSAC on the GPU (sim3opt_essential_batch, sim3opt_amd/csrc/essential_batch.hip: one
workgroup per problem; hypotheses, scoring, pose candidates and vote in one launch) against tests/essential_ref.py,
an independent restatement with another five-point solver.  PARITY UNPINNED (the reference stores no inputs of its
cv::findEssentialMat runs): what is compared is the restatement and planted truth.  The cases and their reference runs
are tests/essential_cases.py's; tests/test_essential_ref.py shows on the CPU that the conditions these comparisons rest
on hold for them, and sets E_LIMIT from the host build of the kernel's arithmetic against the restatement.  Real inputs, the KITTI 00 keyframes, run in
tests/test_gpu_real_keyframes.py."""
import subprocess

import numpy as np
import pytest

import essential_cases as EC
import essential_ref as ER
import test_essential_ref as TE
from sim3opt_amd import lib as L

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
HYP_FIELDS = ("sample", "n_solutions", "valid", "E", "count", "cost")
SUMMARY_FIELDS = ("n_inliers", "status", "best_hypothesis", "n_inliers_hypothesis", "cost_hypothesis", "winner",
                  "votes_winner", "votes")


def run_batch(cases, arrays=None, **opts):
    a = EC.batch_arrays(cases) if arrays is None else arrays
    b = L.EssentialBatch(**dict(dict(iterations=100, min_points=6), **opts))
    b.set_problems(**a)
    b.solve()
    return b


def snapshot(b):
    """Everything a solve returns, the hypotheses' read-out included, as arrays that can be compared bit for bit."""
    n = b.dims()[0]
    mask, cnt = b.inliers()
    hyp = [b.debug_hypotheses(k) for k in range(n)]
    return dict(poses=b.poses(), essentials=b.essentials(), mask=mask, n_inliers=cnt, hyp=hyp, **b.summary())


def problem_of(snap, ptr, k):
    """Problem k's share of a snapshot."""
    lo, hi = int(ptr[k]), int(ptr[k + 1])
    return [snap["poses"][k], snap["essentials"][k], snap["mask"][lo:hi]] + [snap[f][k:k + 1] for f in SUMMARY_FIELDS] + \
        [snap["hyp"][k][f] for f in HYP_FIELDS]


def same_bits(x, y):
    return all(a.shape == b.shape and a.tobytes() == b.tobytes() for a, b in zip(x, y))


_default_run = {}


def default_run():
    """SIZE_CASES as one batch under OPTS: solved once, shared; do not modify."""
    if not _default_run:
        a = EC.batch_arrays(EC.SIZE_CASES)
        b = run_batch(EC.SIZE_CASES, a)
        _default_run.update(arrays=a, batch=b, snap=snapshot(b))
    return _default_run["arrays"], _default_run["batch"], _default_run["snap"]


def check_whole_solve(snap, ptr, k, case, items=()):
    """Problem k of a solve against essential_ref's run of `case`: status, best hypothesis, counts, masks and winner
    exactly; E up to sign, the quaternion up to sign and t within E_LIMIT."""
    ref = EC.reference(*case, items)
    lo, hi = int(ptr[k]), int(ptr[k + 1])
    hyp, best = ref["hyp"], ref["best"]
    assert snap["status"][k] == ref["status"] == 0, (case, items)
    # the index exactly, but for hypotheses the CPU conditions found to be the best one's E to 1e-9 with its count: made
    # of the same points, they tie with it in cost to rounding (the six- and nine-point problems have such)
    twins = (EC.same_up_to_sign(hyp["E"], np.broadcast_to(hyp["E"][best], hyp["E"].shape)) < 1e-9) & hyp["valid"] & \
        (hyp["count"] == hyp["count"][best])
    assert twins[best] and (case[0] < 63 or twins.sum() == 1), (case, items)
    assert twins[snap["best_hypothesis"][k]], (case, items, snap["best_hypothesis"][k], best)
    assert snap["n_inliers_hypothesis"][k] == hyp["count"][best], (case, items)
    want = hyp["cost"][best]
    assert abs(snap["cost_hypothesis"][k] - want) <= 1e-6 * want, (case, items, snap["cost_hypothesis"][k], want)
    # E is a solution up to its sign, and the two solvers need not choose the same one; with -E the candidates 0 <-> 1
    # and 2 <-> 3 change places (include/sim3opt.h), so the restatement's votes are read through that exchange
    E, pose = snap["essentials"][k], snap["poses"][k]
    flipped = np.abs(E - ref["E"]).max() > np.abs(E + ref["E"]).max()
    perm = np.array([1, 0, 3, 2]) if flipped else np.arange(4)
    assert np.abs(E - (-1.0 if flipped else 1.0) * ref["E"]).max() < TE.E_LIMIT, (case, items)
    assert np.array_equal(E, snap["hyp"][k]["E"][snap["best_hypothesis"][k]])
    assert np.array_equal(snap["votes"][k], ref["rec"]["votes"][perm]), (case, items, snap["votes"][k], ref["rec"]["votes"])
    assert snap["winner"][k] == perm[ref["rec"]["winner"]], (case, items)
    assert snap["votes_winner"][k] == snap["n_inliers"][k] == ref["n_inliers"], (case, items)
    assert np.array_equal(snap["mask"][lo:hi].astype(bool), ref["mask"]), (case, items)
    dq = min(np.abs(pose[:4] - ref["pose"][:4]).max(), np.abs(pose[:4] + ref["pose"][:4]).max())
    dt = np.abs(pose[4:] - ref["t"]).max()
    print(f"whole solve {case} {dict(items)}: |dq| {dq:.3e}, |dt| {dt:.3e}")
    assert dq < TE.E_LIMIT and dt < TE.E_LIMIT, (case, items, dq, dt)
    assert abs(np.linalg.norm(pose[4:]) - 1.0) < 1e-14 and abs(np.linalg.norm(pose[:4]) - 1.0) < 1e-14


def test_scoring_operator():
    """sim3opt_essential_batch_debug_score at every point count on the truth, every hypothesis of the reference and an
    E with a zero row: counts equal the reference's, costs within a few ulp x count (the per-point errors are the
    same bits; only the order of the sum differs).  The read-out leaves the last results as they were."""
    a, b, _ = default_run()
    Es = np.stack([EC.score_matrices(*c) for c in EC.SIZE_CASES])
    n = len(EC.SIZE_CASES)
    before = sum((problem_of(snapshot(b), a["point_ptr"], k) for k in range(n)), [])
    count, cost = b.debug_score(Es)
    assert same_bits(before, sum((problem_of(snapshot(b), a["point_ptr"], k) for k in range(n)), []))
    assert np.isfinite(cost).all()
    for k, case in enumerate(EC.SIZE_CASES):
        rc, rs, _ = EC.reference_scores(EC.make_case(*case), Es[k])
        assert np.array_equal(count[k], rc), (case, np.where(count[k] != rc))
        assert (np.abs(cost[k] - rs) <= 4 * EPS * np.maximum(rc, 1) * rs).all(), (case, np.abs(cost[k] - rs).max())
        if case[0] >= 63:
            assert count[k, 0] >= 0.6 * case[0]  # the truth: nearly every point that is no gross outlier


def test_hypotheses():
    """sim3opt_essential_batch_debug_hypotheses against the restatement's hypotheses: the same sample for every h; on
    well-conditioned hypotheses validity and the number of real solutions equal and E within E_LIMIT up to sign;
    count and cost of every hypothesis are the reference's scoring of the device's own E, exactly."""
    a, b, snap = default_run()
    worst = 0.0
    for k, case in enumerate(EC.SIZE_CASES):
        ref, dev, well = EC.reference(*case)["hyp"], snap["hyp"][k], EC.conditioning(*case)
        assert np.array_equal(dev["sample"], ref["sample"]), case
        assert np.isfinite(dev["E"]).all() and np.isfinite(dev["cost"]).all()
        assert np.array_equal(dev["valid"][well].astype(bool), ref["valid"][well]), case
        assert not EC.KNOWN_FEWER_SOLUTIONS.get((case, ()))  # (none of these runs is excused anything)
        assert np.array_equal(dev["n_solutions"][well], ref["n_solutions"][well]), case
        use = well & ref["valid"]
        d = EC.same_up_to_sign(dev["E"], ref["E"])[use].max()
        print(f"hypotheses {case}: max |dE| {d:.3e}")
        worst = max(worst, d)
        assert d < TE.E_LIMIT, (case, d)
        v = dev["valid"].astype(bool)
        rc, rs, e2 = EC.reference_scores(EC.make_case(*case), dev["E"][v])
        assert TE.off(e2, TE.thr2_of(EC.OPTS)), case  # (no point on the threshold for these matrices either)
        assert np.array_equal(dev["count"][v], rc), case
        assert (np.abs(dev["cost"][v] - rs) <= 4 * EPS * np.maximum(rc, 1) * rs).all(), case
        assert (dev["count"][~v] == 0).all() and (dev["cost"][~v] == 0).all() and (dev["E"][~v] == 0).all()
    print(f"hypotheses: worst |dE| {worst:.3e}")


def test_degenerate_samples_are_invalid_and_leave_no_nan():
    """A healthy problem in which point 1 repeats point 0: every hypothesis whose six sample points hold both is
    invalid, be the repeat among the five or the sixth.  Twelve pixels on a line in both views, and twelve times the same pixel pair: status 2, or valid
    matrices, and nothing that is not finite."""
    a = EC.arrays_of(EC.degenerate_problems())
    s = snapshot(run_batch(None, a))
    for f in ("poses", "essentials", "cost_hypothesis"):
        assert np.isfinite(s[f]).all(), f
    for h in s["hyp"]:
        assert np.isfinite(h["E"]).all() and np.isfinite(h["cost"]).all()
        norm = np.sqrt((h["E"] ** 2).sum(axis=(1, 2)))
        assert (np.abs(norm[h["valid"] == 1] - 1.0) < 1e-14).all() and (norm[h["valid"] == 0] == 0).all()
    h0 = s["hyp"][0]
    both = np.array([{0, 1} <= set(row[:5]) for row in h0["sample"]])
    assert both.any() and not h0["valid"][both].any()
    assert s["status"][0] == 0 and h0["valid"].sum() > 80
    h3 = s["hyp"][3]  # eight points: the repeat is among the five, or it is the sixth point, or it is not drawn
    both = np.array([{0, 1} <= set(row[:5]) for row in h3["sample"]])
    sixth = np.array([{0, 1} <= set(row) for row in h3["sample"]]) & ~both
    assert both.any() and sixth.any() and not h3["valid"][both | sixth].any()
    ref3 = ER.hypotheses(*EC.degenerate_problems()[3], EC.FOCAL, EC.CX, EC.CY, EC.OPTS)
    assert np.array_equal(h3["sample"], ref3["sample"]) and not ref3["valid"][both | sixth].any()
    clean = ~(both | sixth)
    assert clean.any() and h3["valid"][clean].sum() >= 0.8 * clean.sum() and s["status"][3] == 0
    ident = np.array([0.0, 0, 0, 1, 0, 0, 0])
    assert s["status"][2] == L.ESSENTIAL_NO_HYPOTHESIS and not s["hyp"][2]["valid"].any()
    for k in (1, 2):
        assert s["status"][k] in (0, 2, 3)
        if s["status"][k] == L.ESSENTIAL_NO_HYPOTHESIS:
            assert np.array_equal(s["poses"][k], ident) and not s["essentials"][k].any() and s["n_inliers"][k] == 0
            assert s["best_hypothesis"][k] == -1 and not s["mask"][a["point_ptr"][k]:a["point_ptr"][k + 1]].any()


def test_pose_operator():
    """sim3opt_essential_batch_debug_pose on the planted E under both signs and both orders of the views, so that
    each candidate index wins once, and on a scene whose points all lie beyond distance_threshold: the candidates
    within 1e-12 of the restatement's SVD, the votes, the winner and the narrowed mask exactly."""
    probs = EC.pose_problems()
    a = EC.arrays_of([(p["uv0"], p["uv1"]) for p in probs])
    b = L.EssentialBatch()
    b.set_problems(**a)
    out = b.debug_pose(np.stack([p["E"] for p in probs]), np.concatenate([p["mask"] for p in probs]))
    winners = []
    for k, p in enumerate(probs):
        rec = EC.reference_pose(p)
        lo, hi = a["point_ptr"][k], a["point_ptr"][k + 1]
        for c, (R, t) in enumerate(rec["candidates"]):
            assert np.abs(ER.quat_to_R(out["candidates"][k, c, :4]) - R).max() < 1e-12, (k, c)
            assert np.abs(out["candidates"][k, c, 4:] - t).max() < 1e-12, (k, c)
        assert np.array_equal(out["votes"][k], rec["votes"]) and out["winner"][k] == rec["winner"], k
        assert np.array_equal(out["mask"][lo:hi].astype(bool), rec["mask"]), k
        winners.append(int(out["winner"][k]))
        if k < 4:  # the winner is the planted pose
            q = out["candidates"][k, out["winner"][k]]
            assert EC.rot_angle(ER.quat_to_R(q[:4]), p["R_true"]) < 1e-10 and np.abs(q[4:] - p["t_true"]).max() < 1e-10
    assert sorted(winners[:4]) == [0, 1, 2, 3]
    assert winners[4] == 0 and not out["votes"][4].any() and not out["mask"][a["point_ptr"][4]:].any()  # status 3's case
    with pytest.raises(L.Sim3OptError) as e:  # the read-out solved nothing
        b.poses()
    assert e.value.code == L.ERR_STATE


def test_whole_solve_matches_reference():
    a, b, snap = default_run()
    for k, case in enumerate(EC.SIZE_CASES):
        check_whole_solve(snap, a["point_ptr"], k, case)
    assert b.tiles() == (EC.LDS_POINTS, EC.CHUNK)


@pytest.mark.parametrize("items", sorted(set(i for _, i in EC.RUNS if i)), ids=lambda i: "-".join(f"{k}{v}" for k, v in i))
def test_whole_solve_options(items):
    """Other hypothesis counts (one, around the chunk of 16, two chunks + 1, once the default 1000), another seed,
    other thresholds."""
    cases = [c for c, i in EC.RUNS if i == items]
    a = EC.batch_arrays(cases)
    snap = snapshot(run_batch(cases, a, **dict(items)))
    for k, case in enumerate(cases):
        check_whole_solve(snap, a["point_ptr"], k, case, items)


def status_batch():
    healthy = (EC.SIZE_CASES[4], EC.SIZE_CASES[6])
    few, far = EC.make_case(*EC.SIZE_CASES[2]), EC.far_scene()
    same = EC.degenerate_problems()[2]
    parts = [(few["uv0"][:3], few["uv1"][:3]), (EC.make_case(*healthy[0])["uv0"], EC.make_case(*healthy[0])["uv1"]),
             (few["uv0"][:8], few["uv1"][:8]), same, (EC.make_case(*healthy[1])["uv0"], EC.make_case(*healthy[1])["uv1"]),
             (far["uv0"], far["uv1"])]
    return healthy, EC.arrays_of(parts)


def test_statuses_beside_healthy_problems():
    """One ragged batch under the default min_points = 9: 3 and 8 points end with status 1, twelve identical pixel
    pairs with status 2, the far scene with status 3 (E returned, candidate 0, no inlier left); the healthy problems
    between them give the bits they give alone."""
    healthy, a = status_batch()
    alone = [snapshot(run_batch((c,), min_points=9)) for c in healthy]
    b = L.EssentialBatch(iterations=100)
    b.set_problems(**a)
    assert b.solve() == 2
    s = snapshot(b)
    assert list(s["status"]) == [1, 0, 1, 2, 0, 3]
    ident = np.array([0.0, 0, 0, 1, 0, 0, 0])
    for k in (0, 2, 3):
        assert np.array_equal(s["poses"][k], ident) and s["n_inliers"][k] == 0 and not s["essentials"][k].any()
        assert s["best_hypothesis"][k] == -1
    assert not s["hyp"][0]["valid"].any() and not s["hyp"][0]["sample"].any()  # nothing run
    assert s["winner"][5] == 0 and not s["votes"][5].any() and s["n_inliers"][5] == 0
    assert abs(np.linalg.norm(s["essentials"][5]) - 1.0) < 1e-14 and s["n_inliers_hypothesis"][5] == 40
    assert not s["mask"][a["point_ptr"][5]:].any() and abs(np.linalg.norm(s["poses"][5][4:]) - 1.0) < 1e-14
    assert np.isfinite(s["poses"]).all() and np.isfinite(s["essentials"]).all()
    for j, k in enumerate((1, 4)):
        assert same_bits(problem_of(s, a["point_ptr"], k), problem_of(alone[j], [0, healthy[j][0]], 0)), healthy[j]


def test_problems_are_independent_of_the_batch():
    """A problem alone, first, last and among others: the same bits everywhere.  Two solves of one handle give the
    same bits; another seed, other samples."""
    a, b, snap = default_run()
    cases, ptr = EC.SIZE_CASES, a["point_ptr"]
    for k in (0, 4, len(cases) - 1):
        one = EC.batch_arrays((cases[k],))
        alone = snapshot(run_batch((cases[k],), one))
        assert same_bits(problem_of(alone, one["point_ptr"], 0), problem_of(snap, ptr, k)), cases[k]
    rev = EC.batch_arrays(cases[::-1])
    back = snapshot(run_batch(cases[::-1], rev))
    for k, case in enumerate(cases):
        assert same_bits(problem_of(back, rev["point_ptr"], len(cases) - 1 - k), problem_of(snap, ptr, k)), case
    many = tuple(cases[k % 8] for k in range(300))  # more workgroups than compute units
    am = EC.batch_arrays(many)
    sm = snapshot(run_batch(many, am, iterations=17))
    for k in range(8, 300):
        assert same_bits(problem_of(sm, am["point_ptr"], k), problem_of(sm, am["point_ptr"], k % 8)), k
    b.solve()
    again = snapshot(b)
    for k, case in enumerate(cases):
        assert same_bits(problem_of(again, ptr, k), problem_of(snap, ptr, k)), case
    other = snapshot(run_batch(cases, a, seed=777))
    want = np.array([ER.sample(777, h, cases[4][0]) for h in range(100)])
    assert np.array_equal(other["hyp"][4]["sample"], want) and not np.array_equal(want, snap["hyp"][4]["sample"])


def test_memory_and_errors():
    """sim3opt_device_memory_in_use is constant across solves and the three read-outs and back at its start after
    close(); the handle holds eight blocks; after a change of size, and of options.device, it solves again to the same
    bytes; read-outs and refused calls leave the last results bit for bit; the refusals say what they refuse."""
    start = L.device_memory_in_use()
    cases = EC.SIZE_CASES[2:5]
    a = EC.batch_arrays(cases)
    b = L.EssentialBatch(iterations=100, min_points=6)
    b.set_problems(**a)
    for call in (b.poses, b.essentials, b.inliers, b.summary, lambda: b.debug_hypotheses(0)):
        with pytest.raises(L.Sim3OptError) as e:
            call()
        assert e.value.code == L.ERR_STATE
    assert b.solve() == 3
    held = L.device_memory_in_use()
    assert held[1] > start[1] and held[0] - start[0] == 8  # ptr, pixels, three per hypothesis, two per problem, mask
    first = snapshot(b)
    flat = lambda s: sum((problem_of(s, a["point_ptr"], k) for k in range(3)), [])
    b.solve()
    assert L.device_memory_in_use() == held
    b.debug_hypotheses(1)
    b.debug_score(np.stack([EC.score_matrices(*c) for c in cases]))
    assert L.device_memory_in_use() == held
    b.debug_pose(first["essentials"], first["mask"])
    assert L.device_memory_in_use() == held
    assert same_bits(flat(snapshot(b)), flat(first))  # the read-outs left the results as they were
    for kw in (dict(iterations=0), dict(iterations=4097), dict(threshold=0.0), dict(threshold=float("nan")),
               dict(distance_threshold=-1.0), dict(min_points=5)):
        with pytest.raises(L.Sim3OptError) as e:
            b.set_options(**kw)
        assert e.value.code == L.ERR_ARG and "essential_batch_set_options: value out of range" in str(e.value), kw
    bad = {k: np.array(v) for k, v in a.items()}
    bad["uv1"][5, 1] = np.nan
    with pytest.raises(L.Sim3OptError) as e:
        b.set_problems(**bad)
    assert e.value.code == L.ERR_ARG and "non-finite observation" in str(e.value)
    with pytest.raises(L.Sim3OptError) as e:
        b.debug_hypotheses(3)
    assert e.value.code == L.ERR_ARG and "no such problem" in str(e.value)
    assert same_bits(flat(snapshot(b)), flat(first)) and b.options()["min_points"] == 6
    # another size and back, another device setting and back: the same bytes held, the same bits
    b.set_problems(**EC.batch_arrays(cases[:2]))
    assert b.solve() == 2 and L.device_memory_in_use()[0] == held[0] and L.device_memory_in_use()[1] < held[1]
    b.set_problems(**a)
    b.solve()
    assert L.device_memory_in_use() == held and same_bits(flat(snapshot(b)), flat(first))
    b.set_options(iterations=100, min_points=6, device=0)
    assert L.device_memory_in_use()[0] == start[0]  # the blocks went with the device setting
    with pytest.raises(L.Sim3OptError) as e:
        b.set_options(iterations=100, min_points=6, device=4096)
        b.solve()
    assert e.value.code == L.ERR_ARG and "device ordinal out of range" in str(e.value)
    b.set_options(iterations=100, min_points=6, device=0)
    b.solve()
    assert L.device_memory_in_use() == held and same_bits(flat(snapshot(b)), flat(first))
    b.close()
    assert L.device_memory_in_use() == start


def test_cxx_conformance(tmp_path):
    """tests/cxx/essential_conformance.cpp: EssentialBatch's rotations and translation directions are within the bound
    tests/test_essential_ref.py measured, through the restatement, of the planted truth; its inlier count is its mask's."""
    exe = TE.compile_conformance(tmp_path)
    path = str(tmp_path / "candidates.txt")
    TE.write_conformance_file(path, TE.CONFORMANCE_CASES)
    r = subprocess.run([exe, "run", path], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 failed" in r.stdout, r.stdout + r.stderr


HOST_RUNS = tuple((c, ()) for c in EC.SIZE_CASES[:6]) + (((65, 5), EC.opt_items(seed=4242)),)


def test_hypotheses_have_the_host_builds_bits(tmp_path):
    """The stage is compiled without fused multiply-add so that a hypothesis has on the device the bits it has in the
    host build of essential_math.hpp (tests/cxx/essential_math_driver.cpp): sample, validity, number of real solutions
    and every entry of E are compared bit for bit, also for the run with the known limit, where the device, like the
    host build, finds fewer solutions than the restatement and the same E."""
    exe = TE.compile_cxx(tmp_path, "essential_math_driver", flags=("-O2", "-Wno-unknown-pragmas"), link=False)
    for case, items in HOST_RUNS:
        c, o = EC.make_case(*case), EC.merged(items)
        a = EC.batch_arrays((case,))
        dev = run_batch((case,), a, **dict(items)).debug_hypotheses(0)
        head = f"{EC.FOCAL!r} {EC.CX!r} {EC.CY!r} {o['seed']} {o['iterations']} {case[0]}\n"
        host = TE.run_driver(exe, "hyp", head + TE.points_text(c))
        assert np.array_equal(dev["sample"], host[:, :6].astype(np.int32)), (case, items)
        assert np.array_equal(dev["valid"], host[:, 6].astype(np.int32)), (case, items)
        assert np.array_equal(dev["n_solutions"], host[:, 7].astype(np.int32)), (case, items)
        assert dev["E"].reshape(-1, 9).tobytes() == np.ascontiguousarray(host[:, 8:17]).tobytes(), (case, items)
        ref, well = EC.reference(*case, items)["hyp"], EC.conditioning(*case, items)
        exact = EC.exact_count_mask(case, items, well)
        assert np.array_equal(dev["n_solutions"][exact], ref["n_solutions"][exact]), (case, items)
        for h in EC.KNOWN_FEWER_SOLUTIONS.get((case, items), ()):
            assert well[h] and dev["valid"][h] == 1 and 1 <= dev["n_solutions"][h] <= ref["n_solutions"][h], (case, items, h)
        use = well & ref["valid"]
        assert EC.same_up_to_sign(dev["E"], ref["E"])[use].max() < TE.E_LIMIT, (case, items)
