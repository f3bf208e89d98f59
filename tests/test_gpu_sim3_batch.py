"""The batched Sim(3) stage on the GPU (sim3opt_sim3_batch, sim3opt_amd/csrc/sim3_batch.hip: one workgroup per
problem; Horn hypotheses, scoring, LM refinement, final inliers and the information matrix in one launch) against the
host build of its arithmetic (bit for bit where no libm function is involved) and against tests/sim3_batch_ref.py, an
independent restatement.  PARITY UNPINNED (the reference has no such step): what is compared is the restatement, the
planted truth, and what the optimiser makes of the information matrix.  The cases and their reference runs are
tests/sim3_batch_cases.py's; tests/test_sim3_batch_ref.py shows on the CPU that the conditions these comparisons rest on
hold for them, and sets the limits from the host build against the restatement.  The host build used here is the
plain one (-O2): the sanitizer build of the same driver belongs to the CPU file alone.  Real inputs, the KITTI 00 keyframes, run in
tests/test_gpu_real_keyframes.py.

The refinement goes through exp, sin and cos, whose last bit differs between the device's and the host's libm: the
refined C, chi2 and Omega of a solve are compared with the host build within the limits, everything before the first
LM step (samples, validity, models, counts, costs, the hypothesis's mask, chi2 before, Omega and the weights at a
supplied C) bit for bit."""
import numpy as np
import pytest

import sim3_batch_cases as SC
import sim3_batch_ref as SR
import test_sim3_batch_ref as TS
from sim3opt_amd import lib as L
from sim3opt_amd import sim3np

pytestmark = pytest.mark.gpu
CHI2_7_99 = 18.475  # the 0.99 quantile of chi^2 with seven degrees of freedom
HYP_FIELDS = ("sample", "n_solutions", "valid", "sim3", "count", "cost")
SUMMARY_FIELDS = ("status", "best_hypothesis", "n_inliers_hypothesis", "cost_hypothesis", "rms_px", "refine_iterations",
                  "chi2")


def run_batch(cases, **opts):
    b = L.Sim3Batch(**dict(dict(iterations=SC.OPTS["iterations"]), **opts))
    b.set_problems(**SC.batch_arrays(cases))
    b.solve()
    return b


def snapshot(b):
    """Everything a solve returns, the hypotheses' read-out included, as arrays that can be compared bit for bit."""
    mask, count = b.inliers()
    return dict(sim3=b.sim3(), information=b.information(), mask=mask, n_inliers=count,
                hyp=[b.debug_hypotheses(k) for k in range(b.dims()[0])], **b.summary())


def problem_of(snap, ptr, k):
    lo, hi = int(ptr[k]), int(ptr[k + 1])
    return [snap["sim3"][k], snap["information"][k], snap["mask"][lo:hi], snap["n_inliers"][k:k + 1]] + \
        [snap[f][k:k + 1] for f in SUMMARY_FIELDS] + [snap["hyp"][k][f] for f in HYP_FIELDS]


def same_bits(x, y):
    return all(a.shape == b.shape and a.tobytes() == b.tobytes() for a, b in zip(x, y))


_mixed = {}


def mixed_run():
    """SC.MIXED as one batch under OPTS: solved once, shared; do not modify."""
    if not _mixed:
        b = run_batch(SC.MIXED)
        _mixed.update(ptr=SC.batch_arrays(SC.MIXED)["point_ptr"], batch=b, snap=snapshot(b))
    return _mixed["ptr"], _mixed["batch"], _mixed["snap"]


def check_against(got, k, mask, ref, what, limits=True):
    """Problem k of a snapshot against a reference solve (the restatement's or the host build's)"""
    assert got["status"][k] == ref["status"], (what, got["status"][k], ref["status"])
    assert np.array_equal(mask != 0, ref["mask"]) and got["n_inliers"][k] == ref["n_inliers"], what
    assert got["n_inliers_hypothesis"][k] == ref["n_hyp"], what
    assert SC.sim3_deviation(got["sim3"][k], ref["sim3"]) < TS.REFINED_LIMIT, what
    assert TS.omega_dev(got["information"][k], ref["information"]) < TS.OMEGA_LIMIT, what
    assert abs(got["rms_px"][k] - ref["rms"]) < TS.REFINED_LIMIT * max(1.0, ref["rms"]), what
    if ref["chi2"][0] > TS.CHI2_COMPARED:
        assert got["refine_iterations"][k] == ref["iterations"], what
        assert TS.rel_chi2(got["chi2"][k], ref["chi2"]) < TS.CHI2_LIMIT, what


# ---- the host build ---------------------------------------------------------------------------------------------------
def test_hypotheses_match_the_host_build_bit_for_bit():
    """Every problem of the mixed batch: sample, validity, model, count and cost of every hypothesis are the bits the
    host build of sim3_batch_math.hpp gives; best hypothesis, its mask-derived count, status and final mask equal, the
    refined C, Omega and chi2 within the limits."""
    ptr, b, snap = mixed_run()
    for k, case in enumerate(SC.MIXED):
        hyp = snap["hyp"][k]
        if case[0] < SC.OPTS["min_points"]:
            assert snap["status"][k] == L.SIM3_FEW_POINTS and not hyp["valid"].any() and not hyp["sim3"].any()
            continue
        host = TS.host_hypotheses(case, sanitized=False)
        for f in ("sample", "valid", "sim3", "count", "cost"):
            assert hyp[f].tobytes() == host[f].astype(hyp[f].dtype).tobytes(), (case, f)
        assert np.array_equal(hyp["n_solutions"], hyp["valid"])
        sol = TS.host_solve(case, sanitized=False)
        assert snap["best_hypothesis"][k] == sol["best"], case
        assert snap["cost_hypothesis"][k] == sol["cost_hyp"], case
        check_against(snap, k, snap["mask"][ptr[k]:ptr[k + 1]], sol, case)
        if sol["status"] not in (1, 2):
            assert snap["chi2"][k][0] == sol["chi2"][0] or sol["iterations"] == 0, case  # (before the first step)


def test_scoring_and_information_operators_match_the_host_build():
    """debug_score on the device's own hypotheses returns the solve's counts and costs (the same code on supplied
    models); debug_information at the planted C* on the planted inliers is the host build's, bit for bit, weights
    included; debug_refine from a displaced C* is the host build's within the limits, with its iteration counts."""
    cases = ((65, 3, "noisy"), (257, 3, "noisy"), (SC.LDS_POINTS + 1, 3, "noisy"), (256, 2, "exact"))
    o = SC.merged(SC.opt_items(huber_delta=0.4))
    b = run_batch(cases, huber_delta=0.4)
    ptr = SC.batch_arrays(cases)["point_ptr"]
    hyps = [b.debug_hypotheses(k) for k in range(len(cases))]
    count, cost = b.debug_score(np.stack([h["sim3"] for h in hyps]))
    for k, h in enumerate(hyps):
        v = h["valid"] != 0
        assert np.array_equal(count[k][v], h["count"][v]) and cost[k][v].tobytes() == h["cost"][v].tobytes()
    delta = np.array([2e-3, -1e-3, 1.5e-3, 0.02, -0.01, 0.03, 4e-3])
    sims = np.stack([SR.perturbed(SC.make_case(*c)["C_true"], delta) for c in cases])
    mask = np.concatenate([~SC.make_case(*c)["outlier"] for c in cases])
    inf, ref = b.debug_information(sims, mask), b.debug_refine(sims, mask)
    for k, case in enumerate(cases):
        m = mask[ptr[k]:ptr[k + 1]]
        host = TS.host_information(case, o, sims[k], m, sanitized=False)
        assert inf["information"][k].tobytes() == host["information"].tobytes(), case
        assert inf["weights"][ptr[k]:ptr[k + 1]].tobytes() == host["weights"].tobytes(), case
        assert inf["positive_definite"][k] == host["positive_definite"] == 1
        host = TS.host_refine(case, o, sims[k], m, sanitized=False)
        assert SC.sim3_deviation(ref["sim3"][k], host["sim3"]) < TS.REFINED_LIMIT, case
        assert ref["chi2"][k][0] == host["chi2"][0], case
        if host["chi2"][1] > TS.CHI2_COMPARED:
            assert ref["iterations"][k] == host["iterations"] and np.array_equal(ref["trials"][k], host["trials"]), case
            assert TS.rel_chi2(ref["chi2"][k], host["chi2"]) < TS.CHI2_LIMIT, case
        r = SR.refine(sims[k], SC.data_of(case), m, o)
        assert SC.sim3_deviation(ref["sim3"][k], r["sim3"]) < TS.REFINED_LIMIT, case
        w = SR.information(sims[k], SC.data_of(case), m, o)
        assert TS.omega_dev(inf["information"][k], w["information"]) < TS.OMEGA_LIMIT, case
        assert np.abs(inf["weights"][ptr[k]:ptr[k + 1]] - w["weights"]).max() < TS.OMEGA_LIMIT, case


# ---- the restatement --------------------------------------------------------------------------------------------------
def test_mixed_batch_agrees_with_the_restatement():
    """Every problem of the mixed batch: status, best hypothesis (where it is unique) and mask equal; hypotheses'
    validity and counts equal, their models within MODEL_LIMIT; refined C, Omega, chi2 and RMS within the limits."""
    ptr, b, snap = mixed_run()
    seen = set()
    for k, case in enumerate(SC.MIXED):
        ref = SC.reference(case)
        seen.add(ref["status"])
        check_against(snap, k, snap["mask"][ptr[k]:ptr[k + 1]], ref, case)
        if ref["status"] == 1:
            assert np.array_equal(snap["sim3"][k], sim3np.identity()) and not snap["information"][k].any()
            continue
        hyp = snap["hyp"][k]
        assert np.array_equal(hyp["sample"], ref["hyp"]["sample"]) and np.array_equal(hyp["valid"], ref["hyp"]["valid"])
        assert np.array_equal(hyp["count"], ref["hyp"]["count"]), case
        for h in np.flatnonzero(TS.well_conditioned(ref)):
            assert SC.sim3_deviation(hyp["sim3"][h], ref["hyp"]["sim3"][h]) < TS.MODEL_LIMIT, (case, h)
        if ref["status"] == 2:
            assert snap["best_hypothesis"][k] == -1 and not snap["information"][k].any()
            continue
        if TS.best_is_unique(ref)[0]:
            assert snap["best_hypothesis"][k] == ref["best"], case
        assert abs(snap["cost_hypothesis"][k] - ref["cost_hyp"]) < TS.CHI2_LIMIT * max(1.0, ref["cost_hyp"]), case
    assert seen == {0, 1, 2, 3}


OPTION_SETS = sorted({items for _, items in TS.RUNS if items})


@pytest.mark.parametrize("items", OPTION_SETS, ids=TS.RUN_IDS)
def test_option_sets_agree_with_the_restatement(items):
    """Every listed run under options other than OPTS, the runs of one option set as one batch"""
    cases = [c for c, i in TS.RUNS if i == items]
    b = run_batch(cases, **dict(items))
    ptr, snap = SC.batch_arrays(cases)["point_ptr"], snapshot(b)
    for k, case in enumerate(cases):
        ref = SC.reference(case, items)
        assert ref["status"] == TS.EXPECTED_STATUS.get((case, items), 0)
        check_against(snap, k, snap["mask"][ptr[k]:ptr[k + 1]], ref, (case, items))
        if TS.best_is_unique(ref)[0]:
            assert snap["best_hypothesis"][k] == ref["best"], (case, items)
        host = TS.host_hypotheses(case, items, sanitized=False)
        for f in ("sample", "valid", "sim3", "count", "cost"):
            assert snap["hyp"][k][f].tobytes() == host[f].astype(snap["hyp"][k][f].dtype).tobytes(), (case, items, f)


# ---- a problem's result is its own ------------------------------------------------------------------------------------
def test_a_problem_gives_the_same_bits_alone_in_the_batch_and_in_the_reversed_batch():
    ptr, _, snap = mixed_run()
    rev = tuple(reversed(SC.MIXED))
    rsnap, rptr = snapshot(run_batch(rev)), SC.batch_arrays(rev)["point_ptr"]
    n = len(SC.MIXED)
    for k, case in enumerate(SC.MIXED):
        here = problem_of(snap, ptr, k)
        assert same_bits(here, problem_of(rsnap, rptr, n - 1 - k)), case
        one = run_batch((case,))  # (alone: every case, the one past LDS_POINTS on the global-memory path included)
        assert same_bits(here, problem_of(snapshot(one), np.array([0, case[0]]), 0)), case


# ---- Omega means what the optimiser takes it to mean --------------------------------------------------------------------
def two_vertex_graph(C_true, meas, info):
    g = L.Graph(jacobians=1, fix_small_angle_b=1)
    g.add_vertex(0, sim3np.identity(), fixed=True)
    g.add_vertex(1, C_true)
    g.add_edge(0, 1, meas, info)
    g.initialize()
    return g


def test_information_is_what_the_optimiser_takes_it_to_be():
    """Noise-free pixels, Huber off: with v0 = identity (fixed), v1 = C* and one edge meas = exp(delta) C*,
    info = Omega(C*), the optimiser's chi2 is delta^T Omega delta; the restatement's sum of squared residuals at
    exp(delta) C* is the same to first order in |delta|: the ratio's deviation from 1 shrinks at least fivefold from
    |delta| = 1e-3 to 1e-4.  A wrong side, tangent order or layout of Omega leaves it O(1).  With meas = C* the
    marginal covariance of v1 is Omega^-1."""
    case = (256, 2, "exact")
    c, D = SC.make_case(*case), SC.data_of(case)
    b = L.Sim3Batch(huber_delta=0.0)
    b.set_problems(**SC.batch_arrays((case,)))
    mask = np.ones(case[0], dtype=np.uint8)
    Om = b.debug_information(c["C_true"][None], mask)["information"][0]
    assert TS.omega_dev(Om, SR.information(c["C_true"], D, mask != 0, SC.merged(SC.opt_items(huber_delta=0.0)))[
        "information"]) < TS.OMEGA_LIMIT
    rng = np.random.default_rng(77)
    for _ in range(4):
        d = rng.standard_normal(7)
        d /= np.linalg.norm(d)
        dev = []
        for size in (1e-3, 1e-4):
            meas = SR.perturbed(c["C_true"], size * d)
            g = two_vertex_graph(c["C_true"], meas, Om)
            r = SR.stacked(meas, D)
            ssq = float((r ** 2).sum(dtype=SR.LD))
            dev.append(abs(g.chi2() / ssq - 1.0))
            g.close()
        print("ratio - 1 at 1e-3, 1e-4:", dev)
        assert dev[0] < 0.1 and dev[1] <= dev[0] / 5.0, dev
    g = two_vertex_graph(c["C_true"], c["C_true"], Om)
    cov = g.marginal_covariances()[0]
    inv = np.linalg.inv(Om)
    print("cov against Omega^-1:", np.abs(cov - inv).max() / np.abs(inv).max())
    assert np.abs(cov - inv).max() / np.abs(inv).max() < TS.OMEGA_LIMIT
    g.close()


def chain_graph(C_rel, m=5):
    """v0 = identity (fixed) ... vm = C_rel along a geodesic, odometry edges exact with information 1e8 I: the
    vertices' own covariance is negligible beside Omega^-1"""
    g = L.Graph(jacobians=1, fix_small_angle_b=1)
    xi = sim3np.log(C_rel, fix_b=1)
    S = [sim3np.exp(xi * k / m, fix_b=1) for k in range(m)] + [np.array(C_rel)]
    g.add_vertices(np.stack(S), fixed=[1] + [0] * m)
    g.add_edges(np.arange(m), np.arange(1, m + 1), np.stack([sim3np.mul(S[k + 1], sim3np.inv(S[k])) for k in range(m)]),
                np.tile(1e8 * np.eye(7), (m, 1, 1)))
    g.initialize()
    return g, m


def test_the_gate_decides_with_the_stages_information():
    """On a small chain whose ends are related by the planted C*: the stage's measurement of the noisy case with the
    stage's Omega passes the chi^2_7 gate; a false candidate -- the measurement moved along Omega's stiffest direction,
    by an offset chosen on the CPU so that the restatement's Omega gives d2 twenty times the quantile while |e|^2 stays
    below it -- is accepted with info = NULL and rejected with the stage's Omega."""
    case = (65, 3, "noisy")
    c, ref = SC.make_case(*case), SC.reference(case)
    b = run_batch((case,))
    meas, Om = b.sim3()[0], b.information()[0]
    assert b.summary()["status"][0] == 0
    g, m = chain_graph(c["C_true"])
    _, _, d2 = g.gate_edges([0], [m], meas[None], Om[None])
    print("true candidate d2:", d2)
    assert d2[0] < CHI2_7_99
    lam, vec = np.linalg.eigh(ref["information"])
    alpha = np.sqrt(20.0 * CHI2_7_99 / lam[-1])
    off = alpha * vec[:, -1]
    assert off @ ref["information"] @ off > 10 * CHI2_7_99 and off @ off < 0.01 * CHI2_7_99
    false = SR.perturbed(ref["sim3"], off)
    e, _, d2_none = g.gate_edges([0], [m], false[None], None)
    _, _, d2_info = g.gate_edges([0], [m], false[None], Om[None])
    print("false candidate |e|^2, d2 without and with Omega:", float(e[0] @ e[0]), d2_none, d2_info)
    assert e[0] @ e[0] < CHI2_7_99 and d2_none[0] < CHI2_7_99 and d2_info[0] > CHI2_7_99
    g.close()


# ---- the handle -------------------------------------------------------------------------------------------------------
def test_read_outs_and_refusals_leave_the_last_results():
    ptr, b, snap = mixed_run()
    n, t = b.dims()
    b.debug_score(np.tile(sim3np.identity(), (n, 2, 1)))
    b.debug_refine(np.tile(sim3np.identity(), (n, 1)), np.ones(t, dtype=np.uint8))
    b.debug_information(np.tile(sim3np.identity(), (n, 1)), np.ones(t, dtype=np.uint8))
    bad = np.tile(sim3np.identity(), (n, 1))
    bad[0, 7] = -1.0
    for call in (lambda: b.debug_information(bad, np.ones(t, dtype=np.uint8)),
                 lambda: b.debug_refine(bad, np.ones(t, dtype=np.uint8)), lambda: b.debug_hypotheses(n),
                 lambda: b.set_options(iterations=0),
                 lambda: b.set_problems(**dict(SC.batch_arrays(((10, 2, "exact"),)), depth0=np.zeros(10)))):
        with pytest.raises(L.Sim3OptError) as e:
            call()
        assert e.value.code == L.ERR_ARG
    again = snapshot(b)
    for k in range(n):
        assert same_bits(problem_of(snap, ptr, k), problem_of(again, ptr, k)), k
    assert b.solve() == int((snap["status"] == 0).sum())
    again = snapshot(b)
    for k in range(n):
        assert same_bits(problem_of(snap, ptr, k), problem_of(again, ptr, k)), k  # (a solve is reproducible)


def test_device_memory_is_returned():
    L.Sim3Batch().close()  # (the process-wide device cache is warm)
    start = L.device_memory_in_use()
    b = run_batch(((65, 3, "noisy"), (257, 3, "noisy")))
    b.debug_information(b.sim3(), b.inliers()[0])
    b.debug_refine(b.sim3(), b.inliers()[0])
    assert L.device_memory_in_use() > start
    b.close()
    assert L.device_memory_in_use() == start


def test_conformance_program_runs_the_helper(tmp_path):
    """tests/cxx/sim3_batch_conformance.cpp: sim3opt_shim::Sim3Batch on three planted candidates, each measurement
    through the gate with its information and into a graph"""
    import subprocess
    exe = TS.compile_conformance(tmp_path)
    path = str(tmp_path / "candidates.txt")
    TS.write_conformance_file(path, TS.CONFORMANCE_CASES)
    r = subprocess.run([exe, "run", path], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and " 0 failed" in r.stdout, r.stdout + r.stderr


# ---- the chain --------------------------------------------------------------------------------------------------------
def test_chain_from_frames_to_an_optimised_graph():
    """MatchBatch -> Sim3Batch -> gate_edges -> add_edges -> optimize on a synthetic pair of frames: the keypoints are
    the projections of a planted scene in two cameras related by C*, the descriptors match, every keypoint carries its
    map depth."""
    case = (120, 4, "exact")
    c = SC.make_case(*case)
    rng = np.random.default_rng(5)
    desc = rng.standard_normal((case[0], 64))
    desc /= np.linalg.norm(desc, axis=1, keepdims=True)

    def frame(uv, depth, d):
        k = 6  # (every keypoint's map point six times over: whatever the K nearest are combined by, it is this depth)
        return dict(kp=uv.astype(np.float32), desc=d.astype(np.float32), obs_uv=np.repeat(uv, k, axis=0).astype(np.float32),
                    obs_depth=np.repeat(depth, k).astype(np.float32))
    d1 = desc + 0.01 * rng.standard_normal(desc.shape)
    frames = [frame(c["uv0"], c["depth0"], desc), frame(c["uv1"], c["depth1"], d1 / np.linalg.norm(d1, axis=1, keepdims=True))]
    import match_cases as MC
    mb = L.MatchBatch()
    mb.set_frames(**MC.frame_arrays(frames))
    mb.set_pairs([(0, 1)])
    assert mb.solve() == 1
    ptr, mt = mb.match_ptr(), mb.matches()
    assert ptr[-1] >= 40
    sb = L.Sim3Batch()
    sb.set_problems(ptr, mt["uv0"], mt["uv1"], mt["depth0"], mt["depth1"])
    assert sb.solve() == 1
    meas, Om = sb.sim3(), sb.information()
    err = SC.truth_errors(meas[0], c)
    print("chain: matches", int(ptr[-1]), "inliers", sb.inliers()[1], "against C*", err)
    assert err[0] < 1e-4 and err[1] < 1e-3 and err[2] < 1e-4  # (float32 pixels and depths)
    g, m = chain_graph(c["C_true"])
    _, _, d2 = g.gate_edges([0], [m], meas, Om)
    assert d2[0] < CHI2_7_99
    g.add_edges([0], [m], meas, Om)
    g.initialize()
    g.optimize(5)
    assert np.isfinite(g.chi2()) and g.chi2() < CHI2_7_99
    assert SC.sim3_deviation(g.get_vertex(m), c["C_true"]) < 1e-3
    g.close()
