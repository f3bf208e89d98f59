"""Cases of the batched descriptor matching (tests/test_match_ref.py, tests/test_gpu_match_batch.py): the smallest
shapes at which the kernels of sim3opt_amd/csrc/match_batch.hip can go wrong, not the workload's.

Descriptors of every case but "gaussian" are multiples of 2^-8 in [0, 1): a squared difference is then a multiple of
2^-16 below 1 and every d2 a multiple of 2^-16 below 64 -- at most 22 bits, exact in FP32 in any summation order, with
or without fused multiply-add.  Everything computed on those cases is compared exactly.  (Squared pixel distances need no
such care: the definition fixes each of their roundings, fl(fl(dx dx) + fl(dy dy)).)"""
import functools

import numpy as np

import match_ref as R

# the sizes at which the kernels take another path (sim3opt_match_batch_dims reports them; the GPU test asserts that
# these are the library's and that the cases straddle them)
WAVE, QUERY_TILE, TRAIN_TILE, OBS_CHUNK = 64, 256, 128, 1024
K = 6
KP_SIZES = (1, WAVE - 1, WAVE, WAVE + 1, TRAIN_TILE - 1, TRAIN_TILE, TRAIN_TILE + 1, QUERY_TILE - 1, QUERY_TILE,
            QUERY_TILE + 1, 2 * QUERY_TILE + 1)
OBS_SIZES = (1, K - 1, K, K + 1, OBS_CHUNK - 1, OBS_CHUNK, OBS_CHUNK + 1, 2 * OBS_CHUNK + 1, 300, 17, K)
KITTI = dict(focal=718.856, cx=607.1928, cy=185.2157, image_width=1241, image_height=376)


def _quantised_frame(rng, pool, homes, n_kp, n_obs, w, h, lattice=False):
    """n_kp keypoints drawn (with replacement) from a pool of descriptors that the frames share, half of them copied
    exactly -- so train descriptors repeat (the index tie) and queries repeat (the uniqueness tie) -- the others with
    four entries moved by a few 2^-8; a keypoint lies near its pool entry's home pixel."""
    pick = rng.integers(0, pool.shape[0], n_kp)
    d = pool[pick].copy()
    for i in np.nonzero(rng.random(n_kp) < 0.5)[0]:
        k = rng.integers(0, 64, 4)
        d[i, k] = np.clip(d[i, k] + rng.integers(-3, 4, 4), 0, 255)
    kp = homes[pick] + rng.integers(-8, 9, (n_kp, 2)) / 4.0
    if lattice:  # observations on the integer lattice round integer keypoints: equal distances by the dozen
        kp = np.round(kp)
        ouv = np.round(rng.uniform([0, 0], [w, h], (n_obs, 2)) / 2) * 2
    else:
        ouv = np.round(rng.uniform([0, 0], [w, h], (n_obs, 2)) * 4) / 4
    return dict(kp=kp.astype(np.float32), desc=(d / 256.0).astype(np.float32), obs_uv=ouv.astype(np.float32),
                obs_depth=rng.uniform(5, 50, n_obs).astype(np.float32))


def _pool(rng, n, w, h):
    # homes: most inside the border, some in it (so the border filter has work), quarter pixels
    homes = np.round(rng.uniform([0.05 * w, 0.02 * h], [0.95 * w, 0.98 * h], (n, 2)) * 4) / 4
    return rng.integers(0, 256, (n, 64)), homes


@functools.lru_cache(maxsize=None)
def tiles():
    """Keypoint counts round the wavefront, the query tile and the train tile on either side of a pair (the full cross
    product, so every (f, f) and every frame shared by 22 pairs), observation counts round K and the LDS chunk, a
    frame without keypoints and one without observations."""
    rng = np.random.default_rng(20261019)
    w, h = KITTI["image_width"], KITTI["image_height"]
    pool, homes = _pool(rng, 400, w, h)
    frames = [_quantised_frame(rng, pool, homes, n, m, w, h, lattice=(i % 3 == 2))
              for i, (n, m) in enumerate(zip(KP_SIZES, OBS_SIZES))]
    frames.append(_quantised_frame(rng, pool, homes, 0, 10, w, h))   # no keypoints
    frames.append(_quantised_frame(rng, pool, homes, 40, 0, w, h))   # no map
    n = len(KP_SIZES)
    e, m = n, n + 1
    pairs = [(a, b) for a in range(n) for b in range(n)] + [(0, e), (e, 3), (m, 2), (2, m), (e, m), (m, m)]
    return dict(name="tiles", frames=frames, pairs=pairs, intr=KITTI, options={})


@functools.lru_cache(maxsize=None)
def ratio():
    """The ratio test of USE_KNN_MATCH and K = 16: one train descriptor (no second nearest), exact copies (d_1 = 0 with
    d_2 > 0, and d_1 = d_2 = 0)."""
    rng = np.random.default_rng(7)
    w, h = KITTI["image_width"], KITTI["image_height"]
    pool, homes = _pool(rng, 60, w, h)
    sizes = ((1, 3), (2, 15), (WAVE + 1, 16), (TRAIN_TILE + 2, 17), (90, 40))
    frames = [_quantised_frame(rng, pool, homes, n, m, w, h, lattice=(i == 3)) for i, (n, m) in enumerate(sizes)]
    pairs = [(a, b) for a in range(len(sizes)) for b in range(len(sizes))]
    return dict(name="ratio", frames=frames, pairs=pairs, intr=KITTI, options=dict(ratio=1.25, knn_k=16))


@functools.lru_cache(maxsize=None)
def boundaries():
    """Keypoints exactly on the border lines and exactly at the skew limits, observations equidistant from a keypoint.
    A 1024 x 512 image with border_ratio = 1/8, skew_x = 1/4 and skew_y = 1/8 puts every limit on an integer: x in
    [128, 896], y in [64, 448], |dx| < 256, |dy| < 64.  Train descriptor j is query descriptor j, so query j meets train j at d2 = 0."""
    rng = np.random.default_rng(11)
    intr = dict(focal=500.0, cx=512.0, cy=256.0, image_width=1024, image_height=512)
    xs0 = [128, 127.75, 128.25, 896, 896.25, 895.75, 300, 300, 300, 300, 400, 400, 400, 400, 400, 400, 500, 500]
    ys0 = [200, 200, 200, 200, 200, 200, 64, 63.75, 448, 448.25, 200, 200, 200, 200, 200, 200, 300, 300]
    # displacement to the train keypoint: zero on the border rows, then round the skew limits
    dx = [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 256, 255.75, -256, -255.75, 0, 0, 0, 0]
    dy = [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 64, 63.75, -64, -63.75]
    # ... and the same limits reached by the train keypoint alone (query inside, train on or over the line)
    xs0 += [200, 200, 640, 640]
    ys0 += [100, 100, 320, 320]
    dx += [-72, -72.25, 256, 256.25]
    dy += [-36, -36.25, 64, 64.25]
    n = len(xs0)
    kp0 = np.stack([xs0, ys0], axis=1).astype(np.float32)
    kp1 = (kp0.astype(np.float64) + np.stack([dx, dy], axis=1)).astype(np.float32)
    desc = (rng.integers(0, 256, (n, 64)) / 256.0).astype(np.float32)
    # observations: the four lattice neighbours at distance 1, the four at sqrt 2 and the four at 2 of every keypoint,
    # in shuffled order -- K = 6 cuts through a group of equals
    def obs(kp):
        off = np.array([(1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (1, -1), (-1, 1), (-1, -1), (2, 0), (-2, 0), (0, 2),
                        (0, -2)], dtype=np.float64)
        uv = (np.round(kp.astype(np.float64))[:, None, :] + off[None]).reshape(-1, 2)
        uv = uv[rng.permutation(uv.shape[0])]
        return uv.astype(np.float32), rng.uniform(5, 50, uv.shape[0]).astype(np.float32)
    u0, z0 = obs(kp0)
    u1, z1 = obs(kp1)
    frames = [dict(kp=kp0, desc=desc, obs_uv=u0, obs_depth=z0), dict(kp=kp1, desc=desc.copy(), obs_uv=u1, obs_depth=z1)]
    return dict(name="boundaries", frames=frames, pairs=[(0, 1), (1, 0)], intr=intr,
                options=dict(border_ratio=0.125, skew_x=0.25, skew_y=0.125))


@functools.lru_cache(maxsize=None)
def gaussian():
    """Unit-norm Gaussian descriptors, every query a train descriptor plus small noise (renormalised): the one case
    whose d2 is not exact in FP32."""
    rng = np.random.default_rng(3)
    w, h = KITTI["image_width"], KITTI["image_height"]
    nt, nq = 300, QUERY_TILE + 1
    b = rng.standard_normal((nt, 64))
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    planted = rng.permutation(nt)[:nq]
    a = b[planted] + 0.02 * rng.standard_normal((nq, 64))
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    kp1 = np.round(rng.uniform([0.15 * w, 0.15 * h], [0.85 * w, 0.85 * h], (nt, 2)) * 4) / 4
    kp0 = kp1[planted] + rng.integers(-8, 9, (nq, 2)) / 4.0

    def frame(kp, d, m):
        return dict(kp=kp.astype(np.float32), desc=d.astype(np.float32),
                    obs_uv=(np.round(rng.uniform([0, 0], [w, h], (m, 2)) * 4) / 4).astype(np.float32),
                    obs_depth=rng.uniform(5, 50, m).astype(np.float32))
    return dict(name="gaussian", frames=[frame(kp0, a, 200), frame(kp1, b, 230)], pairs=[(0, 1)], intr=KITTI,
                options={}, planted=planted)


QUANTISED = (tiles, ratio, boundaries)


@functools.lru_cache(maxsize=None)
def reference(case_fn, defect=None, dtype=np.float32):
    """(per-pair results, match_ptr) of tests/match_ref.py on a case: computed once, shared, left unchanged."""
    c = case_fn()
    return R.match_batch(c["frames"], c["pairs"], c["intr"], c["options"], dtype, defect)


def frame_arrays(frames):
    """The ragged arrays sim3opt_match_batch_set_frames takes."""
    kp_ptr = np.zeros(len(frames) + 1, np.int32)
    obs_ptr = np.zeros(len(frames) + 1, np.int32)
    kp_ptr[1:] = np.cumsum([f["kp"].shape[0] for f in frames])
    obs_ptr[1:] = np.cumsum([f["obs_uv"].shape[0] for f in frames])
    cat = lambda k, shape: np.concatenate([f[k].reshape(shape) for f in frames]).astype(np.float32)
    return dict(kp_ptr=kp_ptr, obs_ptr=obs_ptr, kp=cat("kp", (-1, 2)), desc=cat("desc", (-1, 64)),
                obs_uv=cat("obs_uv", (-1, 2)), obs_depth=cat("obs_depth", (-1,)))
