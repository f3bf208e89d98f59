"""The loop-candidate stages on the GPU on real inputs: the first 45 PTAM keyframes of KITTI 00 (tests/real_cases.py),
the pixels as stored.  PnpBatch, EssentialBatch, HomographyBatch and Sim3Batch each solve the 86 keyframe pairs as one
ragged batch; every problem is compared with its restatement's run by the rule the stage's own GPU test applies to a
whole solve (imported, not repeated here) and with the pose PTAM stored at twice the margin
tests/test_real_keyframes_ref.py measured for the restatement.  The hypothesis and scoring read-outs run through the
stages' own tests on six of the problems; TwoViewBatch, MatchBatch and TrackBatch follow, the last against the host
restatement byte for byte and against the point ids, a truth no restatement had a hand in; then the chain, once.

A problem real_cases.LISTED names (none at the time of writing) is left out of the index and mask equalities only.
The homography rule is the stock one up to the planted-plane bounds, which have no meaning for scenes that are no
planes: in their place stands the nearer of the two kept decompositions against PTAM's pose."""
import numpy as np
import pytest

import ba_ref as BR
import essential_cases as EC
import homography_cases as HC
import homography_ref as HR
import match_cases as MC
import match_ref as MR
import pnp_cases as PC
import real_cases as RC
import sim3_batch_cases as SC
import test_gpu_essential_batch as GE
import test_gpu_homography_batch as GH
import test_gpu_pnp_batch as GP
import test_gpu_sim3_batch as GS
import test_gpu_two_view_batch as GT
import test_homography_ref as TH
import test_real_keyframes_ref as RR
import test_sim3_batch_ref as TS
import track_ref as TR
from oracle import ba_oracle as BO
from sim3opt_amd import lib as L

pytestmark = pytest.mark.gpu
SIX = RC.six()
HANDLE = dict(pnp=L.PnpBatch, essential=L.EssentialBatch, homography=L.HomographyBatch, sim3=L.Sim3Batch)
SNAPSHOT = dict(pnp=GP.snapshot, essential=GE.snapshot, homography=GH.snapshot, sim3=GS.snapshot)
_solved = {}


def solved(stage):
    """The 86 problems as one batch of `stage`'s handle under real_cases.OPTIONS: solved once, shared; do not modify."""
    if stage not in _solved:
        a = RC.batch_arrays(stage)
        b = HANDLE[stage](device=0, **RC.OPTIONS[stage])
        b.set_problems(**a)
        assert b.solve() == len(RC.pair_problems())
        _solved[stage] = (a, b, SNAPSHOT[stage](b))
    return _solved[stage]


def ratio(worst, what, value, bound):
    print(f"{what}: {value:.3e} of {bound:.3e}")
    worst[what] = max(worst.get(what, 0.0), value / bound)
    assert value <= bound, (what, value, bound)


def report(stage, worst):
    print(f"{stage}: worst deviation / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


# ---- the RANSAC handles on the 86 problems ----------------------------------------------------------------------------
def test_pnp_batch():
    a, _, snap = solved("pnp")
    worst = {}
    for k, p in enumerate(RC.pair_problems()):
        if not RC.listed("pnp", k):
            GP.check_whole_solve(snap, a["point_ptr"], k, RC.key("pnp", k), RC.ITEMS["pnp"])
        d = RC.pose7_deviation(snap["poses"][k], p)
        ratio(worst, "rotation", d[0], 2 * RR.PNP_ROT)
        ratio(worst, "|dt| / |t|", d[1], 2 * RR.PNP_DT)
    report("PnP", worst)


def test_essential_batch():
    a, _, snap = solved("essential")
    worst = {}
    for k, p in enumerate(RC.pair_problems()):
        if not RC.listed("essential", k):
            GE.check_whole_solve(snap, a["point_ptr"], k, RC.key("essential", k), RC.ITEMS["essential"])
        d = RC.pose7_deviation(snap["poses"][k], p)
        ratio(worst, "rotation", d[0], 2 * RR.ESSENTIAL_ROT)
        ratio(worst, "direction of t", d[2], 2 * RR.ESSENTIAL_DIR)
    report("essential", worst)


def check_homography(snap, ptr, k, case, items, equalities=True):
    """test_gpu_homography_batch.check_whole_solve up to its planted-plane bounds, with its own expected_choice and
    check_choice"""
    ref, opts, c = HC.reference(case, items), HC.merged(items), HC.make_case(*case)
    lo, hi = int(ptr[k]), int(ptr[k + 1])
    hyp, best = ref["hyp"], ref["best"]
    assert snap["status"][k] == ref["status"] == HR.OK, (case, items)
    if not equalities:
        return None
    twins = (HC.same_up_to_sign(hyp["H"], np.broadcast_to(hyp["H"][best], hyp["H"].shape)) < 1e-9) & hyp["valid"]
    assert twins[best] and twins[snap["best_hypothesis"][k]], (case, items, snap["best_hypothesis"][k], best)
    assert abs(snap["cost_hypothesis"][k] - ref["cost"]) <= 1e-9 * ref["cost"], (case, items)
    assert snap["n_inliers"][k] == ref["n_inliers"] and np.array_equal(snap["mask"][lo:hi].astype(bool), ref["mask"]), (case, items)
    Hm, Hr = snap["H_mlesac"][k], snap["H_refined"][k]
    assert np.array_equal(Hm, snap["hyp"][k]["H"][snap["best_hypothesis"][k]])
    sgn, exp = GH.expected_choice(ref, Hm, c, opts)
    dm, dr = np.abs(Hm - sgn * ref["H_mlesac"]).max(), np.abs(Hr - sgn * ref["H_refined"]).max()
    ds = (np.abs(snap["sigma2"][k] - ref["refine"]["sigma2"]) / ref["refine"]["sigma2"]).max()
    assert dm < TH.H_LIMIT and dr < TH.REFINED_LIMIT and ds < TH.SIGMA_LIMIT, (case, items, dm, dr, ds)
    GH.check_choice(snap, k, exp, (case, items))
    return exp


def test_homography_batch():
    a, b, snap = solved("homography")
    worst, ambiguous = {}, 0
    for k, p in enumerate(RC.pair_problems()):
        case = RC.key("homography", k)
        exp = check_homography(snap, a["point_ptr"], k, case, RC.ITEMS["homography"], not RC.listed("homography", k))
        ambiguous += int(snap["ambiguous"][k])
        pose = snap["poses"][k]
        d = RC.pose7_deviation(np.concatenate([pose[:4], pose[4:]]), p)
        if not snap["ambiguous"][k]:
            ratio(worst, "rotation", d[0], 2 * RR.HOMOGRAPHY_ROT)
            ratio(worst, "direction of t", d[2], 2 * RR.HOMOGRAPHY_DIR)
        elif exp is not None:  # the nearer of the two the restatement kept, which check_choice has tied the device to
            e = RR.homography_deviation(exp, p)
            ratio(worst, "rotation (nearer kept)", e[0], 2 * RR.HOMOGRAPHY_ROT)
            ratio(worst, "direction of t (nearer kept)", e[1], 2 * RR.HOMOGRAPHY_DIR)
    print(f"homography: {ambiguous} of {len(RC.pair_problems())} choices ambiguous on the device")
    assert ambiguous == RR.HOMOGRAPHY_AMBIGUOUS
    report("homography", worst)


def test_sim3_batch():
    a, _, snap = solved("sim3")
    worst, ptr = {}, a["point_ptr"]
    for k, p in enumerate(RC.pair_problems()):
        ref = RC.reference("sim3", k)
        if not RC.listed("sim3", k):
            GS.check_against(snap, k, snap["mask"][ptr[k]:ptr[k + 1]], ref, p["pair"])
            hyp = snap["hyp"][k]
            assert np.array_equal(hyp["sample"], ref["hyp"]["sample"]) and np.array_equal(hyp["valid"], ref["hyp"]["valid"])
            assert np.array_equal(hyp["count"], ref["hyp"]["count"]), p["pair"]
            for h in np.flatnonzero(TS.well_conditioned(ref)):
                assert SC.sim3_deviation(hyp["sim3"][h], ref["hyp"]["sim3"][h]) < TS.MODEL_LIMIT, (p["pair"], h)
            if TS.best_is_unique(ref)[0]:
                assert snap["best_hypothesis"][k] == ref["best"], p["pair"]
            assert abs(snap["cost_hypothesis"][k] - ref["cost_hyp"]) < TS.CHI2_LIMIT * max(1.0, ref["cost_hyp"]), p["pair"]
        assert snap["status"][k] == 0
        d = RC.sim3_deviation(snap["sim3"][k], p)
        ratio(worst, "rotation", d[0], 2 * RR.SIM3_ROT)
        ratio(worst, "|dt| / |t|", d[1], 2 * RR.SIM3_DT)
        ratio(worst, "|s / 1.3 - 1|", d[2], 2 * RR.SIM3_SCALE)
    report("Sim(3)", worst)


# ---- the hypothesis and scoring read-outs on the six problems, by the stages' own tests ----------------------------------
def test_pnp_read_outs(monkeypatch):
    monkeypatch.setattr(PC, "SIZE_CASES", tuple(RC.key("pnp", k) for k in SIX))
    monkeypatch.setattr(GP, "_default_run", {})
    GP.test_hypotheses()
    # test_scoring_operator's comparisons; its last one, that the turned pose puts points behind the camera, has no
    # meaning at this scale (the pose is moved 15 map units, the scenes are 2 deep)
    a, b, _ = GP.default_run()
    poses = np.stack([PC.score_poses(*c) for c in PC.SIZE_CASES])
    count, cost = b.debug_score(poses)
    for k, case in enumerate(PC.SIZE_CASES):
        rc, rs, e2, _ = PC.reference_scores(PC.make_case(*case), poses[k])
        assert (np.abs(e2 - GP.THR2) > 1e-9 * GP.THR2).all(), case
        assert np.array_equal(count[k], rc), (case, np.where(count[k] != rc))
        assert (np.abs(cost[k] - rs) <= 1e-12 * rs).all(), (case, np.abs(cost[k] - rs).max())
        assert count[k, 0] >= 0.7 * case[0]


def test_essential_read_outs(monkeypatch):
    monkeypatch.setattr(EC, "SIZE_CASES", tuple(RC.key("essential", k) for k in SIX))
    monkeypatch.setattr(GE, "_default_run", {})
    GE.test_hypotheses()
    GE.test_scoring_operator()


def test_homography_read_outs(monkeypatch, tmp_path):
    """The hypotheses have the host build's bits on real pixels too (the stage is compiled without fused multiply-add),
    and agree with the restatement's within H_LIMIT where they are well-conditioned; the scoring operator's costs are
    the restatement's."""
    cases = tuple(RC.key("homography", k) for k in SIX)
    monkeypatch.setattr(HC, "RUNS", tuple((c, RC.ITEMS["homography"]) for c in cases))
    GH.test_hypotheses_have_the_host_builds_bits(tmp_path)
    a, b, snap = solved("homography")
    items = RC.ITEMS["homography"]
    for k, case in zip(SIX, cases):
        ref, dev, well = HC.reference(case, items)["hyp"], snap["hyp"][k], HC.conditioning(case, items)
        valid = dev["valid"].astype(bool)
        assert np.array_equal(dev["sample"], ref["sample"]) and np.array_equal(valid[well], ref["valid"][well]), case
        assert (dev["count"][valid] == case[0]).all(), case
        use = well & ref["valid"]
        assert HC.same_up_to_sign(dev["H"], ref["H"])[use].max() < TH.H_LIMIT, case
        assert (np.abs(dev["cost"] - ref["cost"])[use] <= 1e-9 * ref["cost"][use]).all(), case


def test_sim3_read_outs():
    """Sample, validity, model, count and cost of every hypothesis are the bits the host build gives, as in
    test_gpu_sim3_batch.py; debug_score on the device's own hypotheses returns the solve's counts and costs."""
    a, b, snap = solved("sim3")
    for k in SIX:
        case, hyp = RC.key("sim3", k), snap["hyp"][k]
        host = TS.host_hypotheses(case, RC.ITEMS["sim3"], sanitized=False)
        for f in ("sample", "valid", "sim3", "count", "cost"):
            assert hyp[f].tobytes() == host[f].astype(hyp[f].dtype).tobytes(), (case, f)
    count, cost = b.debug_score(np.stack([h["sim3"] for h in snap["hyp"]]))
    for k, h in enumerate(snap["hyp"]):
        v = h["valid"] != 0
        assert np.array_equal(count[k][v], h["count"][v]) and cost[k][v].tobytes() == h["cost"][v].tobytes()


# ---- the refinement -----------------------------------------------------------------------------------------------------
def test_two_view_batch():
    """cam0 the identity, cam1 the PnP restatement's pose: the run is ba_oracle's by test_gpu_two_view_batch.py's rule,
    and ends within twice the measured margin of PTAM's pose."""
    which = RC.two_view_subset()
    keys = [RC.key("two_view", k) for k in which]
    a = RC.MODULE["two_view"].batch_arrays(keys)
    snap = GT.snapshot(GT.run_batch(keys, a, **dict(RC.TWO_VIEW_ITEMS)))
    worst = {}
    for j, k in enumerate(which):
        p = RC.pair_problems()[k]
        GT.check_whole_run(snap, a["point_ptr"], j, keys[j], RC.TWO_VIEW_ITEMS)
        d = RC.pose7_deviation(snap["cam1"][j], p)
        ratio(worst, "rotation", d[0], 2 * RR.REFINED_ROT)
        ratio(worst, "|dt| / |t|", d[1], 2 * RR.REFINED_DT)
    report("PnP + two-view", worst)


# ---- matching and the depth lookup ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("knn_k", (1, MC.K, 16))
def test_match_depth_lookup(knn_k):
    fr = RC.match_frames()
    b = L.MatchBatch(device=0, knn_k=knn_k)
    b.set_frames(**MC.frame_arrays(fr), **RC.INTRINSICS)
    for f, frame in enumerate(fr):
        z, nb = b.debug_depth(f, frame["kp"])
        wz, wnb = MR.knn_depth(frame["kp"], frame["obs_uv"], frame["obs_depth"], knn_k)
        assert np.array_equal(nb, wnb), f
        assert np.array_equal(z, wz.astype(np.float64)), f


MATCH_OPTIONS = dict(knn_k=1, ratio=2.0)  # (a keypoint absent from the other frame has no partner: the ratio test drops it)


def match_pairs(which, **options):
    fr = RC.match_frames()
    m = L.MatchBatch(device=0, **dict(MATCH_OPTIONS, **options))
    m.set_frames(**MC.frame_arrays(fr), **RC.INTRINSICS)
    m.set_pairs([RC.pair_problems()[k]["pair"] for k in which])
    assert m.solve() == len(which)
    return m, m.match_ptr(), m.matches()


def test_match_batch_finds_the_id_joins():
    fr, P = RC.match_frames(), RC.pair_problems()
    _, ptr, mt = match_pairs(range(len(P)))
    total = 0
    for k, p in enumerate(P):
        lo, hi = ptr[k], ptr[k + 1]
        a, b = p["pair"]
        q, t = RC.filtered_join(a, b)
        assert np.array_equal(mt["query_idx"][lo:hi], q) and np.array_equal(mt["train_idx"][lo:hi], t), p["pair"]
        # knn_k = 1: the keypoint's own map point, or the lower-indexed one where two share a pixel
        z = MR.knn_depth(fr[a]["kp"][q], fr[a]["obs_uv"], fr[a]["obs_depth"], 1)[0].astype(np.float64)
        z1 = MR.knn_depth(fr[b]["kp"][t], fr[b]["obs_uv"], fr[b]["obs_depth"], 1)[0].astype(np.float64)
        uv0 = fr[a]["kp"][q].astype(np.float64)
        assert np.array_equal(mt["depth0"][lo:hi], z) and np.array_equal(mt["uv0"][lo:hi], uv0), p["pair"]
        assert np.array_equal(mt["depth1"][lo:hi], z1), p["pair"]
        assert not len(q) or (z == fr[a]["obs_depth"][q]).mean() > 0.98
        want = np.stack([z * ((uv0[:, 0] - RC.CX) / RC.FOCAL), z * ((uv0[:, 1] - RC.CY) / RC.FOCAL), z], axis=1)
        assert (np.abs(mt["points0"][lo:hi] - want) <= 1e-15 * np.abs(want)).all(), p["pair"]
        total += hi - lo
    print(f"matches: {total} of {sum(len(p['ids']) for p in P)} id joins pass the border and skew filters")
    assert total > 0.5 * sum(len(p["ids"]) for p in P)


# ---- the tracks -----------------------------------------------------------------------------------------------------------
def track_batch(**options):
    fr, mt, cam, kw = RC.track_arrays()
    T = L.TrackBatch(device=0, **options)
    T.set_frames(*fr)
    T.set_matches(**mt)
    T.set_cameras(*cam, **kw)
    t = RC.track_problem()
    ref = L.TrackBatch.reference(t["kp_ptr"], t["kp"], states=t["states"], **mt, **kw,
                                 max_reproj_px=options.get("max_reproj_px", 0.0))
    return T, ref


def check_tracks(T, ref):
    """test_gpu_track_batch.check's comparisons (it builds its reference from a case dict): every read-out byte for byte"""
    import test_gpu_track_batch as GK
    t = RC.track_problem()
    ref_ba = TR.ba_rows(ref, t["kp_ptr"], t["kp"], point_base=7)
    c = dict(name="kitti00 keyframes")
    GK.check(T, c, (ref, ref_ba))
    return GK.read_out(T)


def test_track_batch_equals_the_restatement_and_the_ids():
    t = RC.track_problem()
    T, ref = track_batch()
    out, _ = check_tracks(T, ref)
    d = T.dims()
    lens = np.diff(out["track_ptr"])
    assert d["n_tracks"] == 7722 and (out["status"] == 0).all()
    assert (lens > d["lane_max"]).sum() == 36 and (lens == d["lane_max"]).sum() == 39 and lens.max() <= d["wave_max"]
    # one id per track, and two observations of one id at most three frames apart in one track
    ids, of, g = RR.track_ids(out)
    assert (ids == ids[out["track_ptr"][:-1]][of]).all()
    track_of = np.full(len(t["kp"]), -1)
    track_of[g] = of
    order = np.lexsort((np.searchsorted(t["kp_ptr"], np.arange(len(t["kp"])), side="right") - 1, t["ids"]))
    frame = np.searchsorted(t["kp_ptr"], order, side="right") - 1
    near = (t["ids"][order][1:] == t["ids"][order][:-1]) & (frame[1:] - frame[:-1] <= 3)
    assert near.sum() > 10000 and (track_of[order][1:][near] == track_of[order][:-1][near]).all()
    assert (track_of[order][1:][near] >= 0).all()
    dist = RR.track_distances(out)
    print(f"tracks: worst distance from PTAM's point {dist.max():.3e} of {2 * RR.TRACK_DISTANCE:.3e}")
    assert dist.max() <= 2 * RR.TRACK_DISTANCE
    # the bundle-adjustment rows against the rows built directly from the ids
    ba = T.ba_rows()
    first_id = ids[out["track_ptr"][:-1]]
    got = sorted(zip(ba["obs_cam"].tolist(), first_id[ba["obs_point"]].tolist(), map(tuple, ba["obs_uv"].tolist())))
    m = np.zeros(len(t["kp"]), dtype=bool)
    for name in ("query_idx", "train_idx"):
        col = 0 if name == "query_idx" else 1
        m[t["kp_ptr"][np.repeat(t["pairs"][:, col], np.diff(t["match_ptr"]))] + t[name]] = True
    fr_of = np.searchsorted(t["kp_ptr"], np.flatnonzero(m), side="right") - 1
    want = sorted(zip(fr_of.tolist(), t["ids"][m].tolist(), map(tuple, t["kp"][m].astype(np.float64).tolist())))
    assert got == want
    cams = t["states"][:, :7]
    B = L.BundleAdjuster(device=0)
    B.set_problem(cams, ba["points"], ba["obs_cam"], ba["obs_point"], ba["obs_uv"])
    P = BO.Problem(cams, ba["points"], ba["obs_cam"], ba["obs_point"], ba["obs_uv"])
    chi = B.chi2()
    r, _ = BR.chi2_ratio(chi, P, P.cams, P.points)
    print(f"chi2 of the tracks' rows under PTAM's cameras {chi:.6f} (oracle {P.chi2():.6f}), error / tolerance {r:.3f}")
    assert np.isfinite(chi) and r <= 1
    B.close()
    T.close()


def test_track_batch_gate_splits():
    T, ref = track_batch(max_reproj_px=RR.TRACK_GATE_PX)
    out, _ = check_tracks(T, ref)
    share = float((out["status"] == TR.REPROJECTION).mean())
    print(f"gate {RR.TRACK_GATE_PX} px: {share:.4f} of the tracks rejected on the device")
    assert set(out["status"].tolist()) == {TR.OK, TR.REPROJECTION} and 0.1 < share < 0.9
    T.close()


# ---- the chain, once ------------------------------------------------------------------------------------------------------
def test_chain_on_the_six_problems():
    """MatchBatch -> PnpBatch -> TwoViewBatch and MatchBatch -> Sim3Batch, the arrays handed on unchanged (float32 pixels
    and depths, knn_k = 1; frame 1's depths are scaled by 1.3 for the Sim(3) leg).  The points are the pixels'
    back-projections at the map depth, not the map points, so the margins are the ones the CPU file measured for the
    restatements on these very arrays (the map points' PnP margin is missed by a tenth here, by the restatement too)."""
    P = RC.pair_problems()
    # (the two largest rotations move every pixel by more than the skew filter allows: the filters are opened, so that
    # the matches are the id joins the margins were measured on)
    _, ptr, mt = match_pairs(SIX, border_ratio=0.0, skew_x=1.0, skew_y=1.0)
    assert list(np.diff(ptr)) == [len(P[k]["ids"]) for k in SIX]
    want = RC.chain_arrays(SIX)  # (the inputs the CPU file measured the chain's margins on)
    for f in ("uv0", "uv1", "depth0", "depth1"):
        assert np.array_equal(mt[f], want[f]), f
    assert np.array_equal(ptr, want["point_ptr"]) and (np.abs(mt["points0"] - want["points0"]) <= 1e-15 * np.abs(want["points0"])).all()
    p = L.PnpBatch(device=0)
    p.set_problems(ptr, mt["points0"], mt["uv1"])
    assert p.solve() == len(SIX)
    tv = L.TwoViewBatch(device=0)
    tv.set_problems(ptr, np.tile([0.0, 0, 0, 1, 0, 0, 0], (len(SIX), 1)), p.poses(), mt["points0"], mt["uv0"], mt["uv1"])
    assert tv.optimize() == len(SIX)
    depth1 = RC.DEPTH_SCALE * mt["depth1"]
    s = L.Sim3Batch(device=0)
    s.set_problems(ptr, mt["uv0"], mt["uv1"], mt["depth0"], depth1)
    assert s.solve() == len(SIX)
    md = L.median_depth_ratio(ptr, mt["depth0"], depth1)
    worst = {}
    for j, k in enumerate(SIX):
        d = RC.pose7_deviation(p.poses()[j], P[k])
        ratio(worst, "PnP rotation", d[0], 2 * RR.CHAIN_PNP_ROT)
        ratio(worst, "PnP |dt| / |t|", d[1], 2 * RR.CHAIN_PNP_DT)
        d = RC.pose7_deviation(tv.cameras()[1][j], P[k])
        ratio(worst, "refined rotation", d[0], 2 * RR.CHAIN_REFINED_ROT)
        ratio(worst, "refined |dt| / |t|", d[1], 2 * RR.CHAIN_REFINED_DT)
        d = RC.sim3_deviation(s.sim3()[j], P[k])
        ratio(worst, "Sim(3) rotation", d[0], 2 * RR.CHAIN_SIM3_ROT)
        ratio(worst, "Sim(3) |dt| / |t|", d[1], 2 * RR.CHAIN_SIM3_DT)
        ratio(worst, "Sim(3) |s / 1.3 - 1|", d[2], 2 * RR.CHAIN_SIM3_SCALE)
        # the camera moves along its axis between keyframes, so the medians of the two frames' depths differ by up to a
        # fifth before any scaling (measured: md / 1.3 - 1 up to 0.197): what is within 1 % of 1.3 is the ratio over
        # that of PTAM's own depths, taken here in numpy from the float64 map points
        mid = int(0.5 * len(P[k]["ids"]))
        own = float(np.sort(P[k]["depth1"])[mid] / np.sort(P[k]["depth0"])[mid])
        print(f"chain {P[k]['pair']}: {ptr[j + 1] - ptr[j]} matches, median depth ratio {md[j]:.5f}, PTAM's depths' {own:.5f}")
        assert abs(md[j] / own / RC.DEPTH_SCALE - 1.0) < 0.01
    report("chain", worst)
