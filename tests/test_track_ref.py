"""The loop-track definition on the CPU: the reference's connection loop (tests/track_ref.py::reference_connect,
kitti_surf.cpp:349-391 as written) against the connected-components definition (tracks_ref) on the reference-held
fixture and on planted cases, the one-line defects the restatement notices, and the library's host restatement
(sim3opt_track_reference, track_host.hpp) against tracks_ref.  No GPU."""
import collections

import numpy as np
import pytest

from sim3opt_amd import lib as L
import track_cases as TC
import track_ref as TR

INTS = ("track_ptr", "obs_frame", "obs_keypoint", "status", "first_match", "match_track", "n_depths")


def ref_kwargs(c, **over):
    kw = dict(kp_ptr=c["kp_ptr"], kp=c["kp"], pairs=c["pairs"], match_ptr=c["match_ptr"], query_idx=c["query_idx"],
              train_idx=c["train_idx"], states=c["states"], mask=c["mask"], depth0=c["depth0"], depth1=c["depth1"],
              focal=c["focal"], cx=c["cx"], cy=c["cy"], max_reproj_px=c["options"].get("max_reproj_px", 0.0))
    kw.update(over)
    return kw


def rows_of(c):
    """(frame, keypoint, frame, keypoint) per match, the form of loopTracks.txt"""
    p = np.repeat(np.arange(len(c["pairs"])), np.diff(c["match_ptr"]))
    return np.stack([c["pairs"][p, 0], c["query_idx"], c["pairs"][p, 1], c["train_idx"]], axis=1)


def as_sets(tr):
    return [frozenset(zip(tr["obs_frame"][a:b].tolist(), tr["obs_keypoint"][a:b].tolist()))
            for a, b in zip(tr["track_ptr"][:-1], tr["track_ptr"][1:])]


@pytest.fixture(scope="module")
def fixture_ref():
    return TR.tracks_ref(**ref_kwargs(TC.fixture(False)))


def test_fixture_is_what_the_script_says():
    rows = TC.fixture_rows()
    assert rows.shape == (16591, 4) and np.load(TC.GOLDEN).dtype == np.int16
    c = TC.fixture(False)
    assert len(c["pairs"]) == 29 and len(set(map(tuple, c["pairs"].tolist()))) == 29
    in_pairs = collections.Counter(f for p in c["pairs"].tolist() for f in set(p))
    assert sum(n > 1 for n in in_pairs.values()) == 14
    assert all(in_pairs[a] > 1 or in_pairs[b] > 1 for a, b in c["pairs"].tolist())


def test_reference_loop_and_definition_agree_on_the_reference_data(fixture_ref):
    """The pin: on the reference's own matches the order-dependent loop and the connected components are the same
    tracks in the same order -- 11 430 of them, 6 530 / 4 639 / 261 of length 2 / 3 / 4, no match dropped, no frame twice."""
    c = TC.fixture(False)
    tracks, dropped = TR.reference_connect(rows_of(c))
    assert dropped == []
    assert collections.Counter(len(t) for t in tracks.values()) == {2: 6530, 3: 4639, 4: 261}
    assert all(len({f for f, _ in t}) == len(t) for t in tracks.values())
    got = fixture_ref
    assert len(got["status"]) == 11430 and not (got["status"] == TR.CONFLICT).any()
    keys = sorted(tracks)
    assert got["first_match"].tolist() == keys  # the key order of _TrackMap
    assert as_sets(got) == [frozenset(tracks[k]) for k in keys]
    assert (got["match_track"] >= 0).all() and (got["status"] == TR.OK).all()  # unit depths, identity cameras


def test_they_differ_exactly_where_the_deviations_say():
    """A match between two observations that sit in different tracks: the reference drops it, the definition joins"""
    c = TC.case("join", [2, 2, 2, 2], [((0, 1), [(0, 0), (1, 1)]), ((2, 3), [(0, 0)]), ((1, 2), [(0, 0)])])
    tracks, dropped = TR.reference_connect(rows_of(c))
    assert dropped == [3] and [sorted(t) for t in tracks.values()] == [[(0, 0), (1, 0)], [(0, 1), (1, 1)], [(2, 0), (3, 0)]]
    got = TR.tracks_ref(**ref_kwargs(c))
    assert as_sets(got) == [frozenset({(0, 0), (1, 0), (2, 0), (3, 0)}), frozenset({(0, 1), (1, 1)})]
    assert got["first_match"].tolist() == [0, 1] and got["match_track"].tolist() == [0, 1, 0, 0]
    # ... and without that match they agree again, order inside a track aside (by g here, by insertion there)
    c = TC.case("chain", [1, 1, 1], [((1, 2), [(0, 0)]), ((0, 1), [(0, 0)])])
    tracks, dropped = TR.reference_connect(rows_of(c))
    assert dropped == [] and tracks == {0: [(1, 0), (2, 0), (0, 0)]}
    got = TR.tracks_ref(**ref_kwargs(c))
    assert list(zip(got["obs_frame"].tolist(), got["obs_keypoint"].tolist())) == [(0, 0), (1, 0), (2, 0)]


def posed_mixed():
    c = dict(TC.mixed(), name="mixed_posed", states=TC.random_states(7, 21), options=dict(max_reproj_px=250.0))
    rng = np.random.default_rng(22)
    for k in ("depth0", "depth1"):
        d = c[k].copy()
        d[d == 1.0] = rng.uniform(3, 30, int((d == 1.0).sum()))
        c[k] = d
    return c


def test_statuses_of_the_planted_cases():
    m = TR.tracks_ref(**ref_kwargs(TC.mixed()))
    assert collections.Counter(m["status"].tolist()) == {TR.OK: 7, TR.CONFLICT: 2, TR.NO_DEPTH: 1}
    assert m["match_track"][TC.mixed()["mask"] == 0].tolist() == [-1]
    behind, gate = (TR.tracks_ref(**ref_kwargs(c)) for c in TC.geometry())
    assert behind["status"].tolist() == [TR.BEHIND] * 4
    assert gate["status"].tolist() == [TR.OK, TR.OK, TR.OK, TR.REPROJECTION] and gate["n_depths"].tolist() == [1] * 4
    assert len(TR.tracks_ref(**ref_kwargs(TC.all_masked()))["status"]) == 0


@pytest.mark.parametrize("defect,case", [
    ("order_by_g", "mixed"), ("mask_ignored", "mixed"), ("depth_highest", "mixed"), ("mean_all", "gate"),
    ("t_not_subtracted", "mixed"), ("scale_dropped", "mixed"), ("conflict_keypoint", "mixed"), ("gate_depth_only", "gate")])
def test_one_line_defects_are_noticed(defect, case):
    c = posed_mixed() if case == "mixed" else TC.geometry()[1]
    good, bad = TR.tracks_ref(**ref_kwargs(c)), TR.tracks_ref(**ref_kwargs(c), defect=defect)
    same_ints = all(np.array_equal(good[k], bad[k]) for k in INTS)
    # a point moved by far more than any rounding, or an integer output changed
    moved = good["points"].shape != bad["points"].shape or np.abs(good["points"] - bad["points"]).max() > 1e-3
    assert not same_ints or moved, defect


def check_host(c, want=None):
    want = TR.tracks_ref(**ref_kwargs(c)) if want is None else want
    got = L.TrackBatch.reference(**ref_kwargs(c))
    for k in INTS:
        assert np.array_equal(got[k], want[k]), (c["name"], k)
    # about 15 roundings a coordinate of relative size 2^-53 each on terms no larger than (|X_c| + |t|) / s
    bound = 32 * 2.0 ** -53 * want["bound"]
    err = np.abs(got["points"] - want["points"]).max(axis=1) if len(bound) else np.zeros(0)
    assert (err <= bound).all(), (c["name"], float((err - bound).max()))


def test_host_restatement_equals_the_definition_on_the_fixture(fixture_ref):
    check_host(TC.fixture(False), fixture_ref)


@pytest.mark.parametrize("c", [posed_mixed(), TC.mixed(), *TC.geometry(), TC.all_masked(), TC.path("bit_reversed"),
                               TC.one_to_one(TC.SCAN_TILE + 1), TC.segments((7, 9, 65))], ids=lambda c: c["name"])
def test_host_restatement_equals_the_definition(c):
    check_host(c)


def test_host_restatement_refuses_what_the_setters_refuse():
    c = TC.mixed()
    for over in (dict(kp_ptr=np.r_[1, c["kp_ptr"][1:]]), dict(match_ptr=c["match_ptr"][::-1].copy()),
                 dict(query_idx=np.where(np.arange(len(c["query_idx"])) == 3, 99, c["query_idx"])),
                 dict(pairs=np.where(np.arange(2 * len(c["pairs"])).reshape(-1, 2) == 5, 7, c["pairs"])),
                 dict(focal=0.0), dict(max_reproj_px=-1.0),
                 dict(states=np.where(np.arange(56).reshape(7, 8) == 15, 0.0, c["states"])),
                 dict(kp=np.where(np.arange(2 * len(c["kp"])).reshape(-1, 2) == 9, np.inf, c["kp"]))):
        with pytest.raises(L.Sim3OptError):
            L.TrackBatch.reference(**ref_kwargs(c, **over))


def test_refusals_that_need_no_device():
    """Every refusal of the setters, with its message, leaves the handle as it was; out-of-order calls are STATE"""
    before = L.device_memory_in_use()
    b, lib = L.TrackBatch(), L.load()
    d = b.dims()
    assert [d[k] for k in L.TrackBatch.DIMS] == [0] * 8
    assert [d[k] for k in L.TrackBatch.TILES] == [TC.WORKGROUP, TC.SCAN_TILE, TC.LANE_MAX, TC.WAVE_MAX]
    c = TC.mixed()
    fr, mt, cam, camkw = TC.arrays(c)

    def refused(call, code, message):
        with pytest.raises(L.Sim3OptError) as e:
            call()
        assert e.value.code == code and message in str(e.value), (str(e.value), message)

    refused(lambda: b.set_matches(**mt), L.ERR_STATE, "track_batch_set_matches: no frames set")
    refused(lambda: b.set_cameras(*cam, **camkw), L.ERR_STATE, "track_batch_set_cameras: no frames set")
    refused(b.solve, L.ERR_STATE, "track_batch_solve: no frames set")
    refused(b.tracks, L.ERR_STATE, "track_batch_get_tracks: no solve yet")
    refused(b.points, L.ERR_STATE, "track_batch_get_points: no solve yet")
    refused(b.ba_rows, L.ERR_STATE, "track_batch_get_ba: no solve yet")
    assert lib.sim3opt_track_batch_get_match_track(b._b, None) == L.ERR_STATE
    refused(lambda: b.set_frames(np.r_[1, c["kp_ptr"][1:]], c["kp"]), L.ERR_ARG, "kp_ptr[0] must be 0")
    refused(lambda: b.set_frames(c["kp_ptr"][::-1].copy(), c["kp"]), L.ERR_ARG, "kp_ptr")
    bad = c["kp"].copy()
    bad[3, 1] = np.nan
    refused(lambda: b.set_frames(c["kp_ptr"], bad), L.ERR_ARG, "track_batch_set_frames: a non-finite keypoint")
    assert lib.sim3opt_track_batch_set_frames(b._b, 7, None, None) == L.ERR_ARG
    refused(lambda: b.set_frames_from(None), L.ERR_ARG, "track_batch_set_frames_from: NULL store")
    s = L.FrameStore()
    refused(lambda: b.set_frames_from(s), L.ERR_STATE, "track_batch_set_frames_from: the store is not filled")
    assert b.dims()["n_frames"] == 0
    b.set_frames(*fr)
    refused(b.solve, L.ERR_STATE, "track_batch_solve: no matches set")
    b.set_matches(**mt)
    refused(b.solve, L.ERR_STATE, "track_batch_solve: no cameras set")
    b.set_cameras(*cam, **camkw)
    want = b.dims()
    assert (want["n_frames"], want["n_pairs"], want["total_matches"]) == (7, len(c["pairs"]), len(c["mask"]))
    q = c["query_idx"].copy()
    q[3] = 99
    refused(lambda: b.set_matches(**dict(mt, query_idx=q)), L.ERR_ARG, "match 3 of pair 1: an index outside its frame")
    t = c["train_idx"].copy()
    t[0] = -1
    refused(lambda: b.set_matches(**dict(mt, train_idx=t)), L.ERR_ARG, "match 0 of pair 0: an index outside its frame")
    pr = c["pairs"].copy()
    pr[2, 1] = 7
    refused(lambda: b.set_matches(**dict(mt, pairs=pr)), L.ERR_ARG, "pair 2: no such frame")
    refused(lambda: b.set_matches(**dict(mt, match_ptr=np.r_[1, c["match_ptr"][1:]])), L.ERR_ARG, "match_ptr[0] must be 0")
    mp = c["match_ptr"].copy()
    mp[2] = mp[1] - 1
    refused(lambda: b.set_matches(**dict(mt, match_ptr=mp)), L.ERR_ARG, "match_ptr is not monotone at pair 1")
    assert lib.sim3opt_track_batch_set_matches(b._b, 1, None, None, None, None, None, None, None) == L.ERR_ARG
    for col, value, message in ((7, 0.0, "frame 1: s <= 0"), (7, -1.0, "frame 1: s <= 0"), (2, np.nan, "a non-finite state"),
                                (4, np.inf, "a non-finite state")):
        st = c["states"].copy()
        st[1, col] = value
        refused(lambda: b.set_cameras(st, **camkw), L.ERR_ARG, "track_batch_set_cameras: " + message)
    refused(lambda: b.set_cameras(c["states"][:6], **camkw), L.ERR_ARG, "states are of 6 frames, the handle holds 7")
    refused(lambda: b.set_cameras(c["states"], focal=0.0), L.ERR_ARG, "focal <= 0")
    refused(lambda: b.set_cameras(c["states"], cx=np.nan), L.ERR_ARG, "non-finite intrinsics")
    assert lib.sim3opt_track_batch_set_cameras(b._b, 7, None, 1.0, 0.0, 0.0) == L.ERR_ARG
    for kw in (dict(max_reproj_px=-1.0), dict(max_reproj_px=np.nan), dict(max_rounds=0), dict(device=-2)):
        with pytest.raises(L.Sim3OptError):
            b.set_options(**kw)
    assert b.dims() == want and b.options() == dict(max_reproj_px=0.0, max_rounds=64, device=-1)
    assert L.device_memory_in_use() == before
    b.close()
    s.close()
