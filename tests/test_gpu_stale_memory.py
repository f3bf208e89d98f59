"""Every handle on poisoned device memory with guarded block tails.

Every device block of the library comes from one cache (csrc/devmem.cpp).  Recycled blocks are not cleared and sizes are
rounded up by up to 12.5 %, so a kernel that reads what nobody wrote, or writes past an array's end into the block's own
slack, is silent -- and the same in every run, since the tests recycle blocks in the same order.  The cache's test mode
(sim3opt_debug_device_memory, include/sim3opt.h) makes both visible:

  covered      floating-point reads before writes: the bytes asked for are 0xFF, a quiet NaN as float and as double, so
               the result turns NaN or differs from the run without the mode; writes into a block's own slack: every
               block ends in at least 256 bytes of 0xA5 that are compared when the block comes back -- for every block
               of every handle and call, the two mailboxes of comm_local.hip included
  not covered  integer arrays: they are filled with 0.  A stale integer may be an index, and a poison that could send a
               load outside its array must not be used on shared machines, so integer reads before writes stay out of
               reach; LDS; pinned host memory; accesses outside the block

Run pattern (three_runs).  A scenario is a function that builds its handles, runs, reads everything out, closes them
and returns what it read as [(name, value)].  It runs three times in one process: A1 and A2 with the mode off, each
after sim3opt_release_device_cache -- A1 == A2 is the precondition that the scenario is deterministic, which the
project's own tests already hold each of these to --, then B with the mode on.  B must equal A1 bit for bit, and the
report must show no overwritten tail, as many blocks checked as filled once everything is closed, and at least as many
blocks filled as the scenario held while its handle was live.  What is compared is what the existing "change nothing"
tests compare: estimates, statistics without the ms_* times, the PCG-schedule and launch counters (outcome() and
as_bytes() of test_gpu_device_memory.py) and every read-out.

To run a new handle type under the mode: write its scenario -- build, run, held(), read everything out, close -- with
sizes that are no multiple of its kernels' tiles, and hand it to three_runs.

The check can fail: test_probe overruns a block on purpose (inside the block: hipMemset on the tail) and sees it
counted; tests/cxx/devmem_owners_driver.cpp checks the arithmetic on the CPU under ASan + UBSan.  No test plants a stale
read in a kernel."""
import gc

import numpy as np
import pytest

from conftest import gpu_available
from sim3opt_amd import lib as L, synth
import ba_cases as BC
import essential_cases as EC
import homography_cases as HC
import lm_cases as LC
import match_cases as MC
import pcg_cases as PC
import place_cases as PLC
import pnp_cases as PNC
import sim3_batch_cases as SC
import two_view_cases as TC
import vocab_cases as VC
import test_gpu_device_memory as DM

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a HIP device")]

LAM = DM.LAM
_held = []  # device_memory_in_use() at the moments a scenario says its handles are live


def held():
    _held.append(L.device_memory_in_use())


def frozen(x):
    """A read-out -- arrays, numbers, ctypes structures, tuples, lists and dicts of them -- as comparable bytes; the ms_*
    fields of statistics are measurements and left out."""
    if isinstance(x, dict):
        return tuple((k, frozen(v)) for k, v in sorted(x.items()) if not str(k).startswith("ms_"))
    if isinstance(x, (tuple, list)):
        return tuple(frozen(v) for v in x)
    if isinstance(x, L.C.Structure):
        return tuple((k, frozen(getattr(x, k))) for k, _ in x._fields_ if not k.startswith("ms_"))
    if x is None or isinstance(x, (str, bytes)):
        return x
    a = np.asarray(x)
    assert a.dtype != object, type(x)  # (the bytes of an object array are addresses)
    return (a.dtype.str, a.shape, DM.as_bytes(a))


def first_difference(a, b):
    """The name of the first item two records differ in, or None."""
    if [n for n, _ in a] != [n for n, _ in b]:
        return "the list of read-outs"
    for (name, x), (_, y) in zip(a, b):
        if frozen(x) != frozen(y):
            return name
    return None


REPORTS = {}  # scenario -> what run B's report showed (printed; the figures of the pull request's summary)


def three_runs(name, scenario):
    gc.collect()  # (handles other tests dropped go now: their blocks were handed out with the mode off)
    try:
        L.debug_device_memory(False)
        L.release_device_cache()
        a1 = scenario()
        L.release_device_cache()
        a2 = scenario()
        assert first_difference(a1, a2) is None, f"{name}: not deterministic in {first_difference(a1, a2)}"
        L.release_device_cache()
        start = L.device_memory_in_use()
        del _held[:]
        L.debug_device_memory(True)
        b = scenario()
        rep = L.debug_device_memory_report()
        L.debug_device_memory(False)
        live = max(h[0] for h in _held) - start[0]
        REPORTS[name] = dict(rep, live_blocks=live, live_bytes=max(h[1] for h in _held) - start[1])
        print(f"[stale] {name}: {rep['filled']} blocks filled, {rep['checked']} checked, {rep['overwritten']} tails "
              f"overwritten (first offset {rep['first_offset']}); {live} blocks / {REPORTS[name]['live_bytes']} poisoned "
              f"bytes held at once")
        assert rep["overwritten"] == 0 and rep["first_offset"] == -1, (name, rep)
        assert first_difference(a1, b) is None, f"{name}: differs on poisoned memory in {first_difference(a1, b)}"
        assert rep["checked"] == rep["filled"], (name, rep)
        assert live >= 1 and rep["filled"] >= live, (name, rep, live)
        assert L.device_memory_in_use() == start, name
    finally:
        L.debug_device_memory(False)
        L.release_device_cache()


# ---- Graph ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", sorted(DM.CONFIGS))
def test_graph_with_every_read_out(cfg):
    """optimize(3), every read-out of readouts(cfg, G), optimize(3): exact, multigrid and block-Jacobi."""
    DM.inputs(cfg)

    def scenario():
        G = DM.make(cfg)
        rec = [("optimize_1", G.optimize(3)), ("outcome_1", DM.outcome(G))]
        for name, call in DM.readouts(cfg, G):
            rec.append((name, call()))
        held()
        rec += [("optimize_2", G.optimize(3)), ("outcome_2", DM.outcome(G))]
        G.close()
        return rec

    three_runs(f"graph_{cfg}", scenario)


def mode_graph(kind):
    """(graph dict of lm_cases' layout, options, iterations) of test_graph_modes"""
    exact, pcg = dict(linear_solver=1), dict(linear_solver=0, preconditioner=0, pcg_rel_tol=1e-12)
    if kind == "gauss_newton_exact":
        return LC.graph("tail_1"), dict(algorithm=L.ALGORITHM_GAUSS_NEWTON, **exact), 3
    if kind == "gauss_newton_pcg":
        return LC.graph("tail_1"), dict(algorithm=L.ALGORITHM_GAUSS_NEWTON, **pcg), 3
    if kind == "dogleg_exact":
        return LC.graph("tail_1"), dict(algorithm=L.ALGORITHM_DOGLEG, dl_delta_init=0.1, **exact), 4
    if kind == "dogleg_pcg":
        return LC.graph("tail_1"), dict(algorithm=L.ALGORITHM_DOGLEG, dl_delta_init=0.1, **pcg), 4
    if kind == "info_kernels_exact":
        return LC.graph("info_kernels"), exact, 3
    if kind == "info_kernels_pcg":
        return LC.graph("info_kernels"), pcg, 3
    raise KeyError(kind)


MODES = ("gauss_newton_exact", "gauss_newton_pcg", "dogleg_exact", "dogleg_pcg", "info_kernels_exact", "info_kernels_pcg")


@pytest.mark.parametrize("kind", MODES)
def test_graph_modes(kind):
    """Gauss-Newton and dogleg (lm_cases "tail_1": 17 active edges, two linearisation workgroups of eight and one edge),
    LM on dense information with mixed robust kernels ("info_kernels": 30 vertices, 60 edges), each through the exact
    factorisation and the block-Jacobi PCG; a covariance request and gate_edges at the end."""
    g, opts, iters = mode_graph(kind)
    free = np.flatnonzero(np.asarray(g["fixed"]) == 0)
    a, z = int(free[0]), int(free[-1])
    ids = g["ids"] if g["ids"] is not None else np.arange(len(g["states"]))

    def scenario():
        G = LC.make(L, g, **opts)
        rec = [("optimize", G.optimize(iters)), ("outcome", DM.outcome(G)), ("edge_chi2", G.edge_chi2())]
        if "dogleg" in kind:
            rec.append(("trust_region_stats", G.trust_region_stats()))
        held()
        rec.append(("covariances", G.covariances([(int(ids[a]), int(ids[a])), (int(ids[a]), int(ids[z]))], LAM)))
        rec.append(("gate_edges", G.gate_edges(np.array([ids[a], ids[z]], dtype=np.int32),
                                               np.array([ids[z], ids[a]], dtype=np.int32), g["meas"][:2], lam=LAM)))
        rec.append(("outcome_end", DM.outcome(G)))
        G.close()
        return rec

    three_runs(f"graph_{kind}", scenario)


BATCH_ITERS = 12


def batch_graph():
    synth.DRIFT_TARGET = 0.05
    return PC.graph_of("m400")


def test_graph_batched_rejected_trials():
    """pcg_batch = 4 on the smallest multigrid case with g2o's finite-difference step 1e-9: LM reaches the noise floor
    of the numeric Jacobians and rejects trials in bursts, whose systems are solved together in the batch's buffers."""
    g = batch_graph()

    def scenario():
        G = L.Graph(fix_small_angle_b=1, pcg_rel_tol=1e-8, preconditioner=2, amg_coarsest=16, pcg_batch=4)
        G.add_vertices(g["states"], g["fixed"])
        G.add_edges(g["v0"], g["v1"], g["meas"])
        G.initialize()
        rec = [("optimize", G.optimize(BATCH_ITERS)), ("outcome", DM.outcome(G))]
        kt = G.kernel_times()
        assert int(kt.n_batches) >= 1 and int(kt.n_batched_solves) >= 2 * int(kt.n_batches), "no trial was batched"
        held()
        G.close()
        return rec

    three_runs("graph_batched_trials", scenario)


@pytest.mark.parametrize("cfg", sorted(DM.CONFIGS))
def test_graph_that_grows(cfg):
    """initialize, optimize(2), one more vertex and two more edges, initialize, optimize(2) on the same handle: the
    larger arrays land in the predecessor's blocks, the path the cache exists for.  (The project's incremental tests
    compare a grown graph with the CPU oracle within a tolerance, not with a fresh graph bit for bit; so nothing of
    that kind is claimed here.)"""
    g = DM.graph(cfg)
    n = len(g["states"])
    free = np.flatnonzero(np.asarray(g["fixed"]) == 0)

    def scenario():
        G = DM.make(cfg)
        rec = [("optimize_1", G.optimize(2)), ("outcome_1", DM.outcome(G))]
        held()
        G.add_vertex(n, g["states"][n - 1])
        G.add_edge(n - 1, n, g["meas"][0])
        G.add_edge(int(free[0]), n, g["meas"][1])
        G.initialize()
        rec += [("edge_errors", G.edge_errors()), ("optimize_2", G.optimize(2)), ("outcome_2", DM.outcome(G))]
        held()
        G.close()
        return rec

    three_runs(f"graph_grows_{cfg}", scenario)


def test_graph_on_two_ranks():
    """set_devices([0, 0]): two in-library ranks on one device, so that the mailboxes comm_local.hip takes straight
    from dev_malloc are covered (block-Jacobi PCG: all-reduces, the exchange, the all-gather of the step)."""
    synth.DRIFT_TARGET = 0.05
    g = synth.chain_loop(200, 239, seed_graph=911, seed_noise=912, min_gap=10)

    def scenario():
        G = L.Graph(preconditioner=0, fix_small_angle_b=1, fd_delta=1e-6, pcg_rel_tol=1e-12)
        G.add_vertices(g["states"], g["fixed"])
        G.add_edges(g["v0"], g["v1"], g["meas"])
        G.set_devices([0, 0])
        G.initialize()
        rec = [("optimize", G.optimize(3)), ("states", G.get_vertices()), ("stats", G.stats())]
        held()
        G.close()
        return rec

    three_runs("graph_two_ranks", scenario)


# ---- batch handles ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", [0, 1])
def test_bundle_adjuster(solver):
    """ba_cases "pcg_17" through the PCG on the reduced system and its exact factorisation, with the debug_* read-outs."""
    P = BC.problem("pcg_17")

    def scenario():
        b = L.BundleAdjuster(linear_solver=solver)
        b.set_problem(P.cams, P.points, P.oc, P.op, P.uv, P.f, P.cx, P.cy)
        if P.fixed.any():
            b.set_fixed_cameras(P.fixed.astype(np.uint8))
        rec = [("optimize_1", b.optimize(2)), ("cameras_1", b.cameras()), ("points_1", b.points()), ("stats_1", b.stats())]
        held()
        lam = 1e-4 * b.debug_reduced(1.0)["maxdiag"]
        rec += [("debug_pattern", b.debug_pattern()), ("debug_linearization", b.debug_linearization()),
                ("debug_reduced", b.debug_reduced(lam))]
        step = b.debug_step(lam, solver=0, pcg_max_iters=5)
        rec.append(("debug_step_pcg", step))
        if solver == 1:  # (the exact step needs the factorisation plan of linear_solver = 1)
            rec.append(("debug_step_exact", b.debug_step(lam, solver=1)))
        rec += [("debug_update", b.debug_update(step["dx_c"], step["dx_p"], lam)),
                ("debug_update_fail", b.debug_update(step["dx_c"], step["dx_p"], lam, fail=True))]
        rec += [("optimize_2", b.optimize(1)), ("cameras_2", b.cameras()), ("points_2", b.points()), ("stats_2", b.stats()),
                ("chi2", b.chi2())]
        b.close()
        return rec

    three_runs(f"bundle_adjuster_{solver}", scenario)


def test_two_view_batch():
    """ONE_ITERATION_CASES (1 to 1047 points, around the wavefront, the workgroup and their multiples) as one batch."""
    a = TC.batch_arrays(TC.ONE_ITERATION_CASES)

    def scenario():
        t = L.TwoViewBatch()
        t.set_problems(**a)
        rec = [("optimize", t.optimize()), ("getters", DM.two_view_getters(t))]
        held()
        rec += [("debug_trial", t.debug_trial(50.0)), ("getters_after", DM.two_view_getters(t))]
        t.close()
        return rec

    three_runs("two_view_batch", scenario)


def ransac_scenario(make, arrays, results, key, readouts):
    """A scenario of one of the four RANSAC stages: solve, the results, the hypotheses of every problem, the scoring of
    the results, and the stage's other read-outs on its own results and inlier mask.  A problem that ended without a
    model (fewer points than min_points) is given the first solved problem's: the read-outs refuse no batch."""
    def scenario():
        b = make()
        b.set_problems(**arrays)
        rec = [("solve", b.solve())]
        held()
        res = results(b)
        rec.append(("results", res))
        status = np.asarray(b.summary()["status"])
        assert (status != 0).any() and (status == 0).sum() >= 2  # the mix the scenario is about
        rec += [(f"debug_hypotheses_{k}", b.debug_hypotheses(k)) for k in range(len(status))]
        models = np.array(res[key], dtype=np.float64)
        models[status != 0] = models[np.flatnonzero(status == 0)[0]]
        mask = b.inliers()[0]
        rec.append(("debug_score", b.debug_score(models[:, None])))
        rec += [(name, getattr(b, name)(models, mask)) for name in readouts]
        rec.append(("results_after", results(b)))
        b.close()
        return rec
    return scenario


def test_pnp_batch():
    """5 points (fewer than min_points = 9), 65 and 257 in one batch."""
    three_runs("pnp_batch", ransac_scenario(
        L.PnpBatch, PNC.batch_arrays(((5, 27), (65, 5), (257, 8))),
        lambda b: dict(poses=b.poses(), inliers=b.inliers(), summary=b.summary()), "poses", ("debug_refine",)))


def test_essential_batch():
    """6 points (fewer than min_points = 9), 65 and 257 in one batch."""
    three_runs("essential_batch", ransac_scenario(
        lambda: L.EssentialBatch(iterations=100), EC.batch_arrays(((6, 5), (65, 5), (257, 1))),
        lambda b: dict(poses=b.poses(), essentials=b.essentials(), inliers=b.inliers(), summary=b.summary()),
        "essentials", ("debug_pose",)))


def test_homography_batch():
    """8 points (fewer than min_points = 10), 65 and 257 in one batch."""
    three_runs("homography_batch", ransac_scenario(
        lambda: L.HomographyBatch(iterations=HC.OPTS["iterations"]), HC.batch_arrays(((8, 1), (65, 1), (257, 1))),
        lambda b: dict(poses=b.poses(), refined=b.homographies()[1], mlesac=b.homographies()[0], inliers=b.inliers(),
                       summary=b.summary()), "refined", ("debug_refine", "debug_decompose")))


def test_sim3_batch():
    """3 points (fewer than min_points = 9), 65 and 257 in one batch."""
    three_runs("sim3_batch", ransac_scenario(
        lambda: L.Sim3Batch(iterations=SC.OPTS["iterations"]),
        SC.batch_arrays(((3, 1, "exact"), (65, 3, "noisy"), (257, 3, "noisy"))),
        lambda b: dict(sim3=b.sim3(), information=b.information(), inliers=b.inliers(), summary=b.summary()),
        "sim3", ("debug_refine", "debug_information")))


# ---- loop-candidate stages --------------------------------------------------------------------------------------------
def test_match_batch():
    """Two quantised frames of 65 and 37 keypoints, 30 and 45 map observations; both directions."""
    rng = np.random.default_rng(19)
    w, h = MC.KITTI["image_width"], MC.KITTI["image_height"]
    pool, homes = MC._pool(rng, 30, w, h)
    frames = [MC._quantised_frame(rng, pool, homes, n_kp, n_obs, w, h) for n_kp, n_obs in ((65, 30), (37, 45))]
    arrays = MC.frame_arrays(frames)

    def scenario():
        b = L.MatchBatch()
        b.set_frames(**arrays, **MC.KITTI)
        b.set_pairs([(0, 1), (1, 0)])
        rec = [("solve", b.solve()), ("getters", [b.match_ptr(), b.matches(), b.summary()])]
        assert b.match_ptr()[-1] > 0
        held()
        rec += [("debug_nn_0", b.debug_nn(0)), ("debug_nn_1", b.debug_nn(1)),
                ("debug_depth_0", b.debug_depth(0, frames[0]["kp"][:5])), ("debug_depth_1", b.debug_depth(1, frames[1]["kp"]))]
        b.close()
        return rec

    three_runs("match_batch", scenario)


@pytest.mark.parametrize("name", ["frame_sizes_repeated_words", f"tree_of_{PLC.TILES['lds_nodes'] + 1}_nodes"])
def test_place_batch(name):
    """Frames of 1023 and 1025 descriptors on a tree of 585 nodes (either side of bow_chunk, more nodes than lds_nodes
    stages); a tree of lds_nodes + 1 nodes."""
    case = next(c for c in PLC.all_cases() if c["name"] == name)
    n = len(case["kp_ptr"]) - 1

    def scenario():
        b = L.PlaceBatch(**case["options"])
        b.set_vocabulary(*case["voc"].arrays())
        b.set_frames(case["kp_ptr"], case["desc"])
        rec = [("solve", b.solve()), ("results", b.results()), ("pairs", b.pairs()), ("bow", b.bow())]
        held()
        rec.append(("debug_words", b.debug_words(case["desc"][:300])))
        for q in sorted({0, n // 2, n - 1}):
            rec += [(f"debug_scores_{q}", b.debug_scores(q)), (f"debug_islands_{q}", b.debug_islands(q))]
        b.close()
        return rec

    three_runs(f"place_batch_{name}", scenario)


@pytest.mark.parametrize("name", ["k10_L3", "n_around_k"])
def test_vocabulary_trainer(name):
    case = next(c for c in VC.all_cases() if c["name"] == name)

    def scenario():
        t = L.VocabularyTrainer(**case["options"])
        t.set_frames(case["kp_ptr"], case["desc"])
        rec = [("train", t.train()), ("vocabulary", t.vocabulary()), ("assignment", t.assignment(descent=True)),
               ("dims", t.dims())]
        held()
        rec += [("debug_seeding_0", t.debug_seeding(0)), ("debug_seeding_1", t.debug_seeding(1)),
                ("debug_lloyd_0_1", t.debug_lloyd(0, 1)), ("debug_lloyd_1_0", t.debug_lloyd(1, 0)),
                ("vocabulary_after", t.vocabulary())]
        t.close()
        return rec

    three_runs(f"vocabulary_{name}", scenario)


# ---- helpers ----------------------------------------------------------------------------------------------------------
def test_reanchor_points():
    """Three frames, 70 points, 130 observations (no multiple of the wavefront); the last point is never observed and
    comes back as it went in."""
    rng = np.random.default_rng(23)
    F, N, M = 3, 70, 130
    from sim3opt_amd import sim3np as S3
    new = np.array([S3.exp(np.concatenate([rng.standard_normal(3) * 0.1, rng.standard_normal(3), [0.1 * rng.standard_normal()]]),
                           fix_b=True) for _ in range(F)])
    old_Rt = np.array([np.concatenate([S3.quat_to_R(s[:4]).ravel(), s[4:7]]) for s in new])
    old_Rt[:, 9:] += 0.05 * rng.standard_normal((F, 3))
    points = rng.standard_normal((N, 3)) * 5
    obs_f, obs_p = rng.integers(0, F, M), rng.integers(0, N - 1, M)

    def scenario():
        held_before = L.device_memory_in_use()
        out = L.reanchor_points(old_Rt, new, points, obs_f, obs_p)
        _held.append((held_before[0] + 1, held_before[1]))  # (a call, no handle: its blocks are gone when it returns)
        assert out[N - 1].tobytes() == points[N - 1].tobytes() and np.isfinite(out).all()
        return [("points", out)]

    three_runs("reanchor_points", scenario)


# ---- the check itself -------------------------------------------------------------------------------------------------
def test_probe():
    """The mode's layout read back, and the check failing without any access outside a block: with no overrun the block
    is all NaN bytes or all zero by kind, its tail at least 256 bytes of 0xA5, the report clean; with 1 and 8 bytes set
    behind the request one violation each at offset 0; with the mode off nothing is filled and nothing reported."""
    gc.collect()
    try:
        L.release_device_cache()
        for nbytes in (0, 8, 1000, 4096, 100001):
            for floating in (True, False):
                L.debug_device_memory(True)
                blk = L.debug_device_memory_probe(nbytes, floating)
                assert blk.shape[0] >= nbytes + 256 and (blk[nbytes:] == 0xA5).all(), (nbytes, floating)
                assert (blk[:nbytes] == (0xFF if floating else 0)).all(), (nbytes, floating)
                if floating and nbytes >= 8:
                    assert np.isnan(blk[:nbytes - nbytes % 8].view(np.float64)).all()
                    assert np.isnan(blk[:nbytes - nbytes % 4].view(np.float32)).all()
                assert L.debug_device_memory_report() == dict(filled=1, checked=1, overwritten=0, first_offset=-1)
                for overrun in (1, 8):
                    L.debug_device_memory(True)  # (resets the counters)
                    blk = L.debug_device_memory_probe(nbytes, floating, overrun)
                    assert (blk[nbytes:nbytes + overrun] != 0xA5).all() and (blk[nbytes + overrun:] == 0xA5).all()
                    assert L.debug_device_memory_report() == dict(filled=1, checked=1, overwritten=1, first_offset=0)
                with pytest.raises(L.Sim3OptError):  # it would leave the block
                    L.debug_device_memory_probe(nbytes, floating, blk.shape[0] - nbytes + 1)
        L.debug_device_memory(True)
        L.debug_device_memory(False)
        blk = L.debug_device_memory_probe(1000, True)
        assert blk.shape[0] == 1024  # the size the cache rounds to, no tail
        L.debug_device_memory_probe(1000, True, 8)  # (inside the block's slack: nothing looks)
        assert L.debug_device_memory_report() == dict(filled=0, checked=0, overwritten=0, first_offset=-1)
    finally:
        L.debug_device_memory(False)
        L.release_device_cache()
