"""Inputs of the loop-track stage for tests/test_track_ref.py (CPU) and tests/test_gpu_track_batch.py: the reference-held
fixture tests/golden/kitti00/loop_tracks_29pairs.npy (tests/golden/make_loop_tracks_fixture.py) and planted cases, each a
dict of the arrays TrackBatch.set_frames / set_matches / set_cameras take plus `options`.  The switch sizes below are
asserted against TrackBatch.dims() by the GPU tests, so a change of a kernel's tile moves the cases with it."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kitti00", "loop_tracks_29pairs.npy")
WORKGROUP, SCAN_TILE, LANE_MAX, WAVE_MAX = 256, 256, 8, 64
FOCAL, CX, CY = 718.856, 607.1928, 185.2157
IDENTITY = (0, 0, 0, 1, 0, 0, 0, 1.0)
ARRAYS = ("kp_ptr", "kp", "pairs", "match_ptr", "query_idx", "train_idx", "mask", "depth0", "depth1", "states")


def fixture_rows():
    return np.load(GOLDEN).astype(np.int64)


def pixels(n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(0, 1240, n), rng.uniform(0, 370, n)], axis=1).astype(np.float32)


def case(name, n_kp, pair_list, states=None, kp=None, options=None, seed=0):
    """n_kp: keypoints per frame; pair_list: ((f0, f1), [(query, train[, depth0, depth1[, mask]]), ...]) per pair"""
    kp_ptr = np.concatenate([[0], np.cumsum(n_kp)]).astype(np.int32)
    rows = [(q, t) + tuple(r) + (1.0, 1.0, 1)[len(r):] for _, ms in pair_list for q, t, *r in ms]
    a = np.array(rows, dtype=np.float64).reshape(-1, 5)
    nf = len(n_kp)
    return dict(name=name, kp_ptr=kp_ptr, kp=pixels(int(kp_ptr[-1]), seed) if kp is None else np.asarray(kp, np.float32),
                pairs=np.array([p for p, _ in pair_list], dtype=np.int32).reshape(-1, 2),
                match_ptr=np.concatenate([[0], np.cumsum([len(ms) for _, ms in pair_list])]).astype(np.int32),
                query_idx=a[:, 0].astype(np.int32), train_idx=a[:, 1].astype(np.int32), mask=a[:, 4].astype(np.uint8),
                depth0=a[:, 2].copy(), depth1=a[:, 3].copy(),
                states=np.tile(IDENTITY, (nf, 1)).astype(np.float64) if states is None else np.asarray(states, np.float64),
                focal=FOCAL, cx=CX, cy=CY, options=dict(options or {}))


def arrays(c):
    """(set_frames args, set_matches kwargs, set_cameras args + kwargs) of a case"""
    return ((c["kp_ptr"], c["kp"]),
            dict(pairs=c["pairs"], match_ptr=c["match_ptr"], query_idx=c["query_idx"], train_idx=c["train_idx"],
                 mask=c["mask"], depth0=c["depth0"], depth1=c["depth1"]),
            (c["states"],), dict(focal=c["focal"], cx=c["cx"], cy=c["cy"]))


def random_states(n, seed):
    rng = np.random.default_rng(seed)
    q = rng.normal(size=(n, 4)) * [0.05, 0.05, 0.05, 0] + [0, 0, 0, 1]
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return np.concatenate([q, rng.uniform(-2, 2, (n, 3)), rng.uniform(0.7, 1.4, (n, 1))], axis=1)


@functools.lru_cache(maxsize=None)
def fixture(posed):
    """The 29 pairs of the fixture with their frames renumbered 0 .. and as many keypoints a frame as its largest
    index says.  posed = False: unit depths, identity cameras.  True: planted poses, depths of 2 .. 40 with absent ones
    of every kind among them, and a pixel gate that the random pixels mostly miss."""
    rows = fixture_rows()
    frames = np.unique(rows[:, [0, 2]])
    f0, f1 = np.searchsorted(frames, rows[:, 0]), np.searchsorted(frames, rows[:, 2])
    n_kp = np.zeros(len(frames), dtype=np.int64)
    np.maximum.at(n_kp, f0, rows[:, 1] + 1)
    np.maximum.at(n_kp, f1, rows[:, 3] + 1)
    start = np.flatnonzero(np.r_[True, (f0[1:] != f0[:-1]) | (f1[1:] != f1[:-1])])
    c = case("fixture_posed" if posed else "fixture_unit", n_kp, [], seed=11)
    c.update(pairs=np.stack([f0[start], f1[start]], axis=1).astype(np.int32),
             match_ptr=np.r_[start, len(rows)].astype(np.int32), query_idx=rows[:, 1].astype(np.int32),
             train_idx=rows[:, 3].astype(np.int32), mask=np.ones(len(rows), dtype=np.uint8),
             depth0=np.ones(len(rows)), depth1=np.ones(len(rows)))
    if posed:
        rng = np.random.default_rng(5)
        c["states"] = random_states(len(frames), 6)
        for k in ("depth0", "depth1"):
            d = rng.uniform(2, 40, len(rows))
            d[rng.random(len(rows)) < 0.3] = np.nan
            d[rng.random(len(rows)) < 0.05] = 0.0
            d[rng.random(len(rows)) < 0.05] = -3.0
            d[rng.random(len(rows)) < 0.05] = np.inf
            c[k] = d
        c["mask"] = (rng.random(len(rows)) < 0.9).astype(np.uint8)
        c["options"] = dict(max_reproj_px=400.0)
    return c


def bit_reversed(n):
    bits = max(1, (n - 1).bit_length())
    return [i for i in (int(format(k, f"0{bits}b")[::-1], 2) for k in range(1 << bits)) if i < n]


def path(order, n=300):
    """A path of n observations over n frames, one match a pair; one hooking round cannot finish it"""
    links = {"ascending": list(range(n - 1)), "descending": list(range(n - 2, -1, -1)),
             "bit_reversed": bit_reversed(n - 1)}[order]
    return case("path_" + order, [1] * n, [((i, i + 1), [(0, 0)]) for i in links], seed=3)


def one_to_one(n_tracks):
    """n_tracks tracks of length 2 from one pair: the scan's carry at tile - 1, tile, tile + 1 and across its second level"""
    return case(f"tracks_{n_tracks}", [n_tracks, n_tracks], [((0, 1), [(i, n_tracks - 1 - i) for i in range(n_tracks)])], seed=4)


def segments(lengths):
    """Track j is keypoint j of the first lengths[j] frames, joined as a star from frame 0 listed from the far end"""
    nf = max(lengths)
    pl = [((0, i), [(j, j) for j, L in enumerate(lengths) if L > i]) for i in range(nf - 1, 0, -1)]
    return case("segments_" + "_".join(map(str, lengths)), [len(lengths)] * nf, pl, seed=8)


SEGMENT_LENGTHS = (LANE_MAX - 1, LANE_MAX, LANE_MAX + 1, WAVE_MAX - 1, WAVE_MAX, WAVE_MAX + 1, WORKGROUP, WORKGROUP + 1,
                   2 * WORKGROUP + 88)
NAN, INF = float("nan"), float("inf")


def mixed():
    """Chain, star, triangle, a match joining two tracks, a conflict, a track without a depth, masked matches, a pair
    with no match and frames with no keypoint, in one batch"""
    n_kp = [7, 7, 0, 7, 5, 0, 5]
    pl = [((0, 1), [(0, 0), (1, 1, NAN, 2.0)]),            # chain 0: a0 - b0 (- d0 below); triangle: a1 - b1
          ((1, 3), [(0, 0), (1, 1)]),                      # chain: b0 - d0; triangle: b1 - d1
          ((0, 3), [(1, 1, 3.0, NAN)]),                    # triangle closes: a1 - d1
          ((4, 6), []),                                    # a pair with no match
          ((0, 4), [(2, 0), (3, 1)]),                      # two tracks ...
          ((3, 6), [(2, 0), (3, 1)]),                      # ... and two more ...
          ((4, 3), [(0, 2)]),                              # ... the first of each joined by one match
          ((0, 1), [(4, 2), (4, 3)]),                      # a conflict: a4 seen twice in frame 1
          ((1, 4), [(4, 2, NAN, 0.0), (4, 3, -1.0, INF)]),  # a conflict without any depth: the conflict comes first
          ((3, 4), [(4, 3, NAN, INF, 1), (5, 2, 1.0, 1.0, 0), (6, 3, INF, -2.0, 1)]),  # ... grown; a masked match
          ((1, 6), [(5, 3, NAN, -1.0)]),                   # a track whose only depths are absent
          ((6, 0), [(2, 5), (2, 5)])]                      # the same match twice; a star follows
    pl += [((6, f), [(4, k)]) for f, k in ((0, 6), (1, 6), (3, 5), (4, 4))]
    return case("mixed", n_kp, pl, seed=9)


def geometry():
    """Statuses by geometry, one track each over frames 0 (identity) and 1: in front of both; behind frame 1, which looks
    the other way; the pixel gate (3 px) missed by 0.1 px on either side by an observation without a depth"""
    states = np.tile(IDENTITY, (2, 1)).astype(np.float64)
    states[1] = (0, 1, 0, 0, 0.5, 0, 0, 1)  # half a turn about y
    states2 = np.tile(IDENTITY, (2, 1)).astype(np.float64)
    kp = np.zeros((8, 2), dtype=np.float32)  # frame 0: 4 keypoints, frame 1: 4
    kp[:4] = [[CX + 50, CY + 20], [CX - 30, CY + 10], [CX + 8, CY - 64], [CX - 128, CY + 32]]
    kp[4:] = kp[:4]
    kp[6, 0] += 2.875   # inside the gate: 2.875 px
    kp[7, 1] -= 3.125   # outside: 3.125 px
    pl = [((0, 1), [(0, 0, 5.0, NAN), (1, 1, 5.0, NAN), (2, 2, 4.0, NAN), (3, 3, 4.0, NAN)])]
    behind = case("behind", [4, 4], pl, states=states, kp=kp)
    gate = case("gate", [4, 4], pl, states=states2, kp=kp, options=dict(max_reproj_px=3.0))
    return behind, gate


def all_masked():
    c = one_to_one(5)
    c.update(name="all_masked", mask=np.zeros(5, dtype=np.uint8))
    return c


def small_cases():
    return [mixed(), *geometry(), all_masked(), path("ascending"), path("descending"), path("bit_reversed"),
            one_to_one(SCAN_TILE - 1), one_to_one(SCAN_TILE), one_to_one(SCAN_TILE + 1),
            one_to_one(SCAN_TILE * SCAN_TILE + 300), segments(SEGMENT_LENGTHS)]


def all_cases():
    return [fixture(False), fixture(True)] + small_cases()
