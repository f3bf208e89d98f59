"""TrackBatch on the device against sim3opt_track_reference, the serial restatement on the host: every output byte --
tracks, their order and observations, statuses, first matches, the track of every match, points, depth counts and the
bundle-adjustment rows -- on the reference-held fixture and the planted cases of tests/track_cases.py; the rounds of the
component search, the handle's life (a second solve, new matches on resident frames, frames from a FrameStore, the
rounds running out) and its refusals."""
import numpy as np
import pytest

from sim3opt_amd import lib as L
import track_cases as TC
import track_ref as TR
from test_track_ref import ref_kwargs

pytestmark = pytest.mark.gpu

KEYS = ("track_ptr", "obs_frame", "obs_keypoint", "status", "first_match", "match_track", "points", "n_depths")
BA = ("points", "obs_cam", "obs_point", "obs_uv")


def reference(c):
    ref = L.TrackBatch.reference(**ref_kwargs(c))
    return ref, TR.ba_rows(ref, c["kp_ptr"], c["kp"], point_base=7)


def read_out(T):
    out = T.tracks()
    out["points"], out["n_depths"] = T.points()
    return out, T.ba_rows(point_base=7)


def frozen(out, ba):
    return b"".join(np.ascontiguousarray(out[k]).tobytes() for k in KEYS) + \
        b"".join(np.ascontiguousarray(ba[k]).tobytes() for k in BA)


def load(T, c, frames=True):
    fr, mt, cam, camkw = TC.arrays(c)
    if frames:
        T.set_frames(*fr)
    T.set_matches(**mt)
    T.set_cameras(*cam, **camkw)


def check(T, c, ref=None):
    """Solves what T holds; the device's read-outs against the restatement's, byte for byte.  Returns the bytes."""
    ref, ref_ba = reference(c) if ref is None else ref
    kept = T.solve()
    out, ba = read_out(T)
    for k in KEYS:
        assert out[k].dtype == ref[k].dtype and out[k].shape == ref[k].shape, (c["name"], k, out[k].shape, ref[k].shape)
        assert out[k].tobytes() == ref[k].tobytes(), (c["name"], k)
    for k in BA:
        assert ba[k].dtype == ref_ba[k].dtype and ba[k].tobytes() == ref_ba[k].tobytes(), (c["name"], k)
    d = T.dims()
    assert kept == int((ref["status"] == TR.OK).sum()) == d["n_kept_tracks"] and d["n_tracks"] == len(ref["status"])
    assert d["n_observations"] == len(ref["obs_frame"]) and d["n_kept_observations"] == len(ref_ba["obs_cam"])
    return frozen(out, ba)


def test_tiles_are_the_ones_the_cases_are_built_for():
    d = L.TrackBatch(device=0).dims()
    assert [d[k] for k in L.TrackBatch.TILES] == [TC.WORKGROUP, TC.SCAN_TILE, TC.LANE_MAX, TC.WAVE_MAX]


@pytest.mark.parametrize("c", TC.all_cases(), ids=lambda c: c["name"])
def test_device_equals_the_host_restatement(c):
    T = L.TrackBatch(device=0, **c["options"])
    load(T, c)
    check(T, c)
    d = T.dims()
    assert 1 <= d["rounds"] <= T.options()["max_rounds"] or d["total_matches"] == 0
    if c["name"].startswith("path_"):
        assert d["n_tracks"] == 1 and d["n_observations"] == 300 and 1 < d["rounds"] <= 64
    if c["name"].startswith("segments_"):
        assert sorted(np.diff(T.tracks()["track_ptr"]).tolist()) == sorted(TC.SEGMENT_LENGTHS)
    if c["name"] == "all_masked":
        assert d["n_tracks"] == 0 and (T.tracks()["match_track"] == -1).all()
    if c["name"] == "fixture_unit":
        assert d["n_tracks"] == 11430 and np.bincount(np.diff(T.tracks()["track_ptr"])).tolist() == [0, 0, 6530, 4639, 261]
    if c["name"] == "fixture_posed":  # every status occurs
        assert set(T.tracks()["status"].tolist()) == {0, 2, 3, 4}
    T.close()


def test_second_solve_new_matches_and_a_frame_store_give_the_same_bytes():
    c, other = TC.fixture(True), TC.mixed()
    ref = reference(c)
    T = L.TrackBatch(device=0, **c["options"])
    load(T, c)
    want = check(T, c, ref)
    assert check(T, c, ref) == want                     # a second solve
    _, mt, cam, camkw = TC.arrays(c)
    T.set_matches(**dict(mt, mask=None))                # other matches on the resident frames ...
    assert T.solve() != int((ref[0]["status"] == 0).sum()) or frozen(*read_out(T)) != want
    T.set_matches(**mt)                                 # ... and the first ones again
    assert check(T, c, ref) == want
    T.set_options(max_reproj_px=0.0)
    T.solve()
    assert frozen(*read_out(T)) != want                 # (the gate mattered)
    load(T, other)                                      # another problem size through the same handle
    T.set_options()
    check(T, other)
    # the frames from a store, read in place
    S = L.FrameStore(device=0)
    S.set(c["kp_ptr"], c["kp"], np.ones((len(c["kp"]), 64), dtype=np.float32))
    held = L.device_memory_in_use()
    U = L.TrackBatch(device=0, **c["options"])
    U.set_frames_from(S)
    assert L.device_memory_in_use() == held             # nothing allocated: the snapshot is shared
    load(U, c, frames=False)
    assert check(U, c, ref) == want
    S.close()                                           # the consumer keeps the snapshot
    assert check(U, c, ref) == want
    with pytest.raises(L.Sim3OptError):
        U.set_options(device=1)
    U.set_frames(c["kp_ptr"], c["kp"])                  # ... and drops it for arrays of its own
    load(U, c, frames=False)
    assert check(U, c, ref) == want
    T.close()
    U.close()


def test_rounds_running_out_is_an_error_and_the_handle_solves_again():
    c = TC.path("bit_reversed")
    T = L.TrackBatch(device=0, max_rounds=1)
    load(T, c)
    with pytest.raises(L.Sim3OptError) as e:
        T.solve()
    assert e.value.code == L.ERR_ARG and "track_batch_solve: the components did not settle in max_rounds = 1 rounds" in str(e.value)
    with pytest.raises(L.Sim3OptError):
        T.tracks()
    T.set_options(max_rounds=64)
    check(T, c)
    assert 1 < T.dims()["rounds"] <= 64
    T.close()


def test_refusals_leave_a_solved_handle_as_it_was():
    c = TC.mixed()
    T = L.TrackBatch(device=0)
    load(T, c)
    want, dims = check(T, c), T.dims()
    fr, mt, cam, camkw = TC.arrays(c)
    q, st, bad = c["query_idx"].copy(), c["states"].copy(), c["kp"].copy()
    q[0], st[2, 7], bad[0, 0] = 50, 0.0, np.inf
    for call in (lambda: T.set_frames(c["kp_ptr"], bad), lambda: T.set_frames(c["kp_ptr"][::-1].copy(), c["kp"]),
                 lambda: T.set_frames_from(None), lambda: T.set_matches(**dict(mt, query_idx=q)),
                 lambda: T.set_matches(**dict(mt, match_ptr=np.r_[1, c["match_ptr"][1:]])),
                 lambda: T.set_cameras(st, **camkw), lambda: T.set_cameras(c["states"], focal=-1.0),
                 lambda: T.set_options(max_rounds=0), lambda: T.ba_rows(point_base=-1)):
        with pytest.raises(L.Sim3OptError):
            call()
        assert T.dims() == dims and frozen(*read_out(T)) == want
    assert check(T, c) == want
    T.close()
