"""The batched descriptor matching and map-depth lookup on the GPU (sim3opt_match_batch,
sim3opt_amd/csrc/match_batch.hip) against tests/match_ref.py, a numpy restatement of the definition in
include/sim3opt.h.  PARITY UNPINNED (the reference stores neither descriptors nor matches, and its matcher is an
approximate search): what is compared is the restatement and planted truth.  The cases are tests/match_cases.py's;
tests/test_match_ref.py shows on the CPU that they reach the mistakes a kernel could make."""
import gc

import numpy as np
import pytest

import match_cases as MC
import match_ref as R
import pnp_cases as PC
from oracle import ba_oracle as BO
from sim3opt_amd import lib as L

pytestmark = pytest.mark.gpu
FIELDS = ("query_idx", "train_idx", "distance", "uv0", "uv1", "depth0", "depth1", "points0")


def run_case(case, pairs=None, **opts):
    b = L.MatchBatch(**dict(case["options"], **opts))
    b.set_frames(**MC.frame_arrays(case["frames"]), **case["intr"])
    b.set_pairs(case["pairs"] if pairs is None else pairs)
    b.solve()
    return b


def snapshot(b):
    return dict(match_ptr=b.match_ptr(), **b.matches(), **b.summary())


def pair_of(snap, k):
    """Pair k's share of a snapshot, as arrays that can be compared bit for bit."""
    lo, hi = int(snap["match_ptr"][k]), int(snap["match_ptr"][k + 1])
    return [snap[f][lo:hi] for f in FIELDS] + \
        [snap[f][k:k + 1] for f in ("status", "n_nearest", "n_after_ratio", "n_after_filters", "n_after_unique")]


def same_bits(x, y):
    return all(a.shape == b.shape and a.tobytes() == b.tobytes() for a, b in zip(x, y))


_runs = {}


def solved(case_fn):
    """A case solved as one batch: once, shared; do not modify."""
    if case_fn not in _runs:
        b = run_case(case_fn())
        _runs[case_fn] = (b, snapshot(b))
    return _runs[case_fn]


def test_tile_sizes_are_the_ones_the_cases_straddle():
    d = solved(MC.tiles)[0].dims()
    assert (d["wavefront"], d["query_tile"], d["train_tile"], d["obs_chunk"]) == \
        (MC.WAVE, MC.QUERY_TILE, MC.TRAIN_TILE, MC.OBS_CHUNK)
    assert solved(MC.tiles)[0].options()["knn_k"] == MC.K
    kp = {f["kp"].shape[0] for f in MC.tiles()["frames"]}
    obs = {f["obs_uv"].shape[0] for f in MC.tiles()["frames"]}
    for t in (d["wavefront"], d["query_tile"], d["train_tile"]):
        assert {t - 1, t, t + 1} <= kp
    assert {1, 2 * d["query_tile"] + 1} <= kp
    assert {0, 1, MC.K - 1, MC.K, MC.K + 1, d["obs_chunk"] - 1, d["obs_chunk"], d["obs_chunk"] + 1} <= obs
    assert d["n_frames"] == len(MC.tiles()["frames"]) and d["n_pairs"] == len(MC.tiles()["pairs"])


@pytest.mark.parametrize("case_fn", MC.QUANTISED, ids=lambda f: f.__name__)
def test_solve_matches_reference_exactly(case_fn):
    """Quantised descriptors: statuses, counts, match_ptr, indices, distance and depths bit for bit; points0 to 1e-15."""
    b, s = solved(case_fn)
    res, ptr = MC.reference(case_fn)
    assert np.array_equal(s["match_ptr"], ptr)
    assert b.solve() == sum(r["status"] == R.OK for r in res)
    for k, r in enumerate(res):
        lo, hi = ptr[k], ptr[k + 1]
        pair = case_fn()["pairs"][k]
        assert s["status"][k] == r["status"], pair
        assert (s["n_nearest"][k], s["n_after_ratio"][k], s["n_after_filters"][k], s["n_after_unique"][k]) == \
            r["counts"], pair
        for f in ("query_idx", "train_idx", "distance", "uv0", "uv1", "depth0", "depth1"):
            assert np.array_equal(s[f][lo:hi], r[f]), (pair, f)
        assert s["distance"].dtype == np.float32 and r["distance"].dtype == np.float32
        assert (np.abs(s["points0"][lo:hi] - r["points0"]) <= 1e-15 * np.abs(r["points0"])).all(), pair


@pytest.mark.parametrize("case_fn", MC.QUANTISED, ids=lambda f: f.__name__)
def test_nearest_neighbours_of_every_query(case_fn):
    """What k_match_nn wrote, which the uniqueness pass hides most of: exact for every query of every OK pair."""
    b, _ = solved(case_fn)
    c = case_fn()
    res, _ = MC.reference(case_fn)
    for k, (r, (f0, f1)) in enumerate(zip(res, c["pairs"])):
        nq = c["frames"][f0]["kp"].shape[0]
        if r["status"] != R.OK:
            with pytest.raises(L.Sim3OptError) as e:
                b.debug_nn(k)
            assert e.value.code == L.ERR_STATE
            continue
        got = b.debug_nn(k)
        assert got["best_idx"].shape == (nq,)
        bi, bd, si, sd = r["nn"]
        assert np.array_equal(got["best_idx"], bi) and np.array_equal(got["second_idx"], si), (f0, f1)
        assert np.array_equal(got["best_d2"], bd) and np.array_equal(got["second_d2"], sd), (f0, f1)


@pytest.mark.parametrize("knn_k", (1, MC.K, 16))
def test_depth_lookup_of_supplied_pixels(knn_k):
    """debug_depth: the K-nearest code on pixels that are no keypoints, on every observation count of the tiles case;
    neighbours (ties by index) and depth exact."""
    c = MC.tiles()
    b = L.MatchBatch(knn_k=knn_k)
    b.set_frames(**MC.frame_arrays(c["frames"]), **c["intr"])
    rng = np.random.default_rng(5)
    w, h = c["intr"]["image_width"], c["intr"]["image_height"]
    for n, lattice in ((MC.QUERY_TILE + 1, False), (MC.WAVE - 1, True)):
        uv = rng.uniform([0, 0], [w, h], (n, 2))
        uv = (np.round(uv / 2) * 2 if lattice else np.round(uv * 4) / 4).astype(np.float32)
        for f, fr in enumerate(c["frames"]):
            if fr["obs_uv"].shape[0] == 0:
                with pytest.raises(L.Sim3OptError) as e:
                    b.debug_depth(f, uv)
                assert e.value.code == L.ERR_ARG
                continue
            z, nb = b.debug_depth(f, uv)
            wz, wnb = R.knn_depth(uv, fr["obs_uv"], fr["obs_depth"], knn_k)
            assert np.array_equal(nb, wnb), (f, lattice)
            assert np.array_equal(z, wz.astype(np.float64)), (f, lattice)
    with pytest.raises(L.Sim3OptError) as e:  # no solve was needed, and none has happened
        b.match_ptr()
    assert e.value.code == L.ERR_STATE


def test_gaussian_descriptors():
    """The one case whose d2 rounds: indices exact (tests/test_match_ref.py: the float64 gap is above 1e-4 relative for
    every query), d2 within the error of a 64-term FP32 sum of non-negative terms in any order, with or without fused
    multiply-add -- (64 + 2) u relative, u = 2^-24: one rounding per difference (2 u on its square), one per product
    and at most 63 additions -- distance within half of that and one rounding of the root."""
    c = MC.gaussian()
    b, s = solved(MC.gaussian)
    bi, bd, si, sd = R.nearest_two(c["frames"][0]["desc"], c["frames"][1]["desc"], np.float64)
    got = b.debug_nn(0)
    assert np.array_equal(got["best_idx"], bi) and np.array_equal(got["second_idx"], si)
    u = 2.0 ** -24
    assert (np.abs(got["best_d2"] - bd) <= 66 * u * bd).all() and (np.abs(got["second_d2"] - sd) <= 66 * u * sd).all()
    res, ptr = MC.reference(MC.gaussian)
    r = res[0]
    assert np.array_equal(s["match_ptr"], ptr) and np.array_equal(s["query_idx"], r["query_idx"])
    assert np.array_equal(s["train_idx"], r["train_idx"]) and np.array_equal(s["train_idx"], c["planted"][r["query_idx"]])
    want = np.sqrt(bd[r["query_idx"]])
    assert (np.abs(s["distance"] - want) <= 34 * u * want).all()
    assert np.array_equal(s["depth0"], r["depth0"]) and np.array_equal(s["depth1"], r["depth1"])
    assert (np.abs(s["points0"] - r["points0"]) <= 1e-15 * np.abs(r["points0"])).all()


def test_pairs_are_independent_of_the_batch():
    """A pair alone, and the batch reversed: the same bits.  Two solves of one handle: the same bytes."""
    c = MC.tiles()
    b, s = solved(MC.tiles)
    n = len(c["pairs"])
    rev = snapshot(run_case(c, c["pairs"][::-1]))
    for k in range(n):
        assert same_bits(pair_of(rev, n - 1 - k), pair_of(s, k)), c["pairs"][k]
    for k in (0, 14, 60, 119, 120, n - 4, n - 1):
        alone = snapshot(run_case(c, [c["pairs"][k]]))
        assert same_bits(pair_of(alone, 0), pair_of(s, k)), c["pairs"][k]
    b.solve()
    again = snapshot(b)
    assert sorted(again) == sorted(s)
    for f in s:
        assert again[f].tobytes() == s[f].tobytes(), f


def test_new_pairs_on_resident_frames():
    """set_pairs alone: the frames stay on the device (their blocks are not handed back and fetched again) and the new
    candidate list gives what a fresh handle gives for it."""
    c = MC.ratio()
    b = run_case(c)
    first = snapshot(b)
    for pairs in (c["pairs"][::-1], c["pairs"][3:4], c["pairs"]):
        b.set_pairs(pairs)
        with pytest.raises(L.Sim3OptError) as e:  # the results went with the old pairs
            b.match_ptr()
        assert e.value.code == L.ERR_STATE
        b.solve()
        got, want = snapshot(b), snapshot(run_case(c, pairs))
        assert sorted(got) == sorted(want)
        for f in want:
            assert got[f].tobytes() == want[f].tobytes(), f
    now = snapshot(b)
    assert all(now[f].tobytes() == first[f].tobytes() for f in first)
    z, nb = b.debug_depth(4, np.array([[300.0, 200.0]]))  # the frames are still where the diagnostics look
    wz, wnb = R.knn_depth(np.array([[300.0, 200.0]], np.float32), c["frames"][4]["obs_uv"], c["frames"][4]["obs_depth"], 16)
    assert np.array_equal(nb, wnb) and z[0] == float(wz[0])


def test_memory_and_errors():
    """Refusals change nothing and leave the last results readable; getters before a solve are state errors; the
    diagnostics keep no device memory; all of it is back after close()."""
    gc.collect()  # (handles of earlier tests that nothing names any more go now, not in the middle of the count)
    start = L.device_memory_in_use()
    c = MC.ratio()
    fa = MC.frame_arrays(c["frames"])
    b = L.MatchBatch(**c["options"])
    with pytest.raises(L.Sim3OptError) as e:
        b.set_pairs(c["pairs"])
    assert e.value.code == L.ERR_STATE
    b.set_frames(**fa, **c["intr"])
    b.set_pairs(c["pairs"])
    for call in (b.match_ptr, b.matches, b.summary, lambda: b.debug_nn(6)):
        with pytest.raises(L.Sim3OptError) as e:
            call()
        assert e.value.code == L.ERR_STATE
    res, ptr = MC.reference(MC.ratio)
    assert b.solve() == sum(r["status"] == R.OK for r in res)
    held = L.device_memory_in_use()
    assert held[1] > start[1]
    first = snapshot(b)
    assert np.array_equal(first["match_ptr"], ptr)
    b.debug_nn(6)
    b.debug_depth(2, np.array([[100.0, 100.0], [7.25, 300.0]]))
    assert L.device_memory_in_use() == held
    b.solve()
    assert L.device_memory_in_use() == held

    def unchanged():
        now = snapshot(b)
        return all(now[f].tobytes() == first[f].tobytes() for f in first)
    assert unchanged()  # the diagnostics left the results as they were
    for kw in (dict(knn_k=0), dict(knn_k=17), dict(ratio=-0.1), dict(border_ratio=-1.0), dict(skew_x=-1e-9),
               dict(skew_y=float("nan")), dict(ratio=float("inf"))):
        with pytest.raises(L.Sim3OptError) as e:
            b.set_options(**kw)
        assert e.value.code == L.ERR_ARG, kw
    assert b.options()["knn_k"] == 16

    def frames_with(**kw):
        a = {k: np.array(v) for k, v in fa.items()}
        intr = dict(c["intr"])
        for k, v in kw.items():
            if k in intr:
                intr[k] = v
            else:
                idx, val = v
                a[k][idx] = val
        return dict(a, **intr)
    for kw in (dict(kp=((3, 1), np.nan)), dict(desc=((5, 60), np.inf)), dict(obs_uv=((0, 0), np.nan)),
               dict(obs_depth=(2, -np.inf)), dict(kp_ptr=(2, 0)), dict(obs_ptr=(0, 1)), dict(kp_ptr=(0, 1)),
               dict(focal=0.0), dict(focal=float("nan")), dict(cx=float("inf")), dict(image_width=0),
               dict(image_height=-3)):
        with pytest.raises(L.Sim3OptError) as e:
            b.set_frames(**frames_with(**kw))
        assert e.value.code == L.ERR_ARG, kw
    for bad in ([(0, len(c["frames"]))], [(-1, 0)], np.zeros((0, 2), np.int32)):
        with pytest.raises(L.Sim3OptError) as e:
            b.set_pairs(bad)
        assert e.value.code == L.ERR_ARG
    for args in ((len(c["frames"]), [[1.0, 1.0]]), (-1, [[1.0, 1.0]]), (0, [[np.nan, 1.0]])):
        with pytest.raises(L.Sim3OptError) as e:
            b.debug_depth(*args)
        assert e.value.code == L.ERR_ARG
    L_ = L.load()  # NULL arrays, which the wrapper cannot produce
    i32 = np.zeros(2, np.int32)
    f = np.zeros(64, np.float32)
    P = lambda a, t: a.ctypes.data_as(t)
    for null in range(6):
        a = [P(i32, L._ip), P(i32, L._ip), P(f, L._fp), P(f, L._fp), P(f, L._fp), P(f, L._fp)]
        a[null] = None
        assert L_.sim3opt_match_batch_set_frames(b._b, 1, *a, 700.0, 600.0, 180.0, 1241, 376) == L.ERR_ARG
    assert L_.sim3opt_match_batch_set_pairs(b._b, 1, None) == L.ERR_ARG
    assert unchanged()
    assert b.solve() == sum(r["status"] == R.OK for r in res) and unchanged()
    b.close()
    assert L.device_memory_in_use() == start


def test_match_pnp_refine_chain():
    """A planted scene through MatchBatch -> PnpBatch -> TwoViewBatch: the planted pose within what
    tests/test_pnp_ref.py measured for the PnP -> refinement chain on noisy pixels (8.5e-4 rad, 6.5e-2 m; this scene has
    none), and sim3opt_median_depth_ratio equal to the planted
    depths' (frame 1's map is `scale` times frame 0's, as after monocular drift)."""
    rng = np.random.default_rng(42)
    W, H = 1241, 376
    intr = dict(focal=PC.FOCAL, cx=PC.CX, cy=PC.CY, image_width=W, image_height=H)
    cases, scales = ((300, 31), (90, 32), (513, 33)), (1.0, 1.7, 0.6)
    frames, truth = [], []
    for (n, seed), scale in zip(cases, scales):
        pc = PC.make_case(n, seed)  # (points in camera 0's frame, camera 1's planted pose)
        P, cam1 = pc["points"], pc["cam1_true"]
        R1, t1 = BO.quat_to_R(cam1[None, :4])[0], cam1[4:]
        X1 = P @ R1.T + t1
        uv0 = np.stack([PC.FOCAL * P[:, 0] / P[:, 2] + PC.CX, PC.FOCAL * P[:, 1] / P[:, 2] + PC.CY], axis=1)
        uv1 = np.stack([PC.FOCAL * X1[:, 0] / X1[:, 2] + PC.CX, PC.FOCAL * X1[:, 1] / X1[:, 2] + PC.CY], axis=1)
        # the border and skew filters on the pixels as the frames hold them
        a, b = uv0.astype(np.float32).astype(np.float64), uv1.astype(np.float32).astype(np.float64)
        inside = (np.abs(b[:, 0] - a[:, 0]) < (1.0 / 3.0) * W) & (np.abs(b[:, 1] - a[:, 1]) < (1.0 / 4.0) * H)
        for uv in (a, b):
            inside &= (uv[:, 0] >= 0.1 * W) & (uv[:, 0] <= (1 - 0.1) * W) & (uv[:, 1] >= 0.1 * H) & (uv[:, 1] <= (1 - 0.1) * H)
        d = rng.standard_normal((n, 64))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        perm = rng.permutation(n)
        # every keypoint is a map-point observation of its frame: with knn_k = 1 a match's depth is its point's
        frames.append(dict(kp=uv0.astype(np.float32), desc=d.astype(np.float32), obs_uv=uv0.astype(np.float32),
                           obs_depth=P[:, 2].astype(np.float32)))
        frames.append(dict(kp=uv1[perm].astype(np.float32), desc=(d + 1e-3 * rng.standard_normal(d.shape))[perm]
                           .astype(np.float32), obs_uv=uv1[perm].astype(np.float32),
                           obs_depth=(scale * X1[perm, 2]).astype(np.float32)))
        truth.append(dict(cam1=cam1, inside=inside, perm=perm, z0=P[:, 2].astype(np.float32),
                          z1=(scale * X1[:, 2]).astype(np.float32)))
    m = L.MatchBatch(knn_k=1)
    m.set_frames(**MC.frame_arrays(frames), **intr)
    m.set_pairs([(0, 1), (2, 3), (4, 5)])
    assert m.solve() == 3
    ptr, mt = m.match_ptr(), m.matches()
    for k, t in enumerate(truth):
        lo, hi = ptr[k], ptr[k + 1]
        assert np.array_equal(mt["query_idx"][lo:hi], np.nonzero(t["inside"])[0])  # the planted matches, all of them
        assert np.array_equal(t["perm"][mt["train_idx"][lo:hi]], mt["query_idx"][lo:hi])
        assert hi - lo > 60
    p = L.PnpBatch()
    p.set_problems(ptr, mt["points0"], mt["uv1"])
    assert p.solve() == 3
    tv = L.TwoViewBatch()
    cam0 = np.tile([0.0, 0, 0, 1, 0, 0, 0], (3, 1))
    tv.set_problems(ptr, cam0, p.poses(), mt["points0"], mt["uv0"], mt["uv1"])
    assert tv.optimize() == 3
    ratio = L.median_depth_ratio(ptr, mt["depth0"], mt["depth1"])
    for k, t in enumerate(truth):
        for pose in (p.poses()[k], tv.cameras()[1][k]):
            assert PC.rot_dist(pose[:4], t["cam1"][:4]) < 8.5e-4 and np.abs(pose[4:] - t["cam1"][4:]).max() < 6.5e-2
        q = mt["query_idx"][ptr[k]:ptr[k + 1]]
        mid = int(0.5 * len(q))
        assert ratio[k] == float(np.sort(t["z1"][q])[mid]) / float(np.sort(t["z0"][q])[mid])
        assert abs(ratio[k] / scales[k] - 1) < 0.2
