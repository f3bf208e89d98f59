"""numpy restatement of the batched descriptor matching and map-depth lookup (include/sim3opt.h, "batched descriptor
matching"; kittiDetector.h:1085-1160 and :1229-1279), written from the definition and not from the kernels.

`dtype` is the arithmetic of the two distance computations: np.float32 is the definition, np.float64 runs next to it
to tell how far FP32 rounding is from deciding a comparison.  `defect` plants one one-line mistake (DEFECTS), for
tests/test_match_ref.py to show that the cases of tests/match_cases.py reach it."""
import numpy as np

OK, NO_KEYPOINTS, NO_MAP = 0, 1, 2
DEFAULTS = dict(ratio=0.0, border_ratio=0.1, skew_x=1.0 / 3.0, skew_y=1.0 / 4.0, knn_k=6)
DEFECTS = ("tie_high", "uniq_lt", "border_gt", "skew_swapped", "ratio_inverted", "k_off_by_one", "mean_over_k",
           "arrival_order", "side1_keypoint0")


def d2_matrix(a, b, dtype=np.float32):
    """d2(i, j) = sum_k (a_ik - b_jk)^2 in `dtype` (the difference form)."""
    a, b = np.asarray(a, dtype=dtype), np.asarray(b, dtype=dtype)
    out = np.empty((a.shape[0], b.shape[0]), dtype=dtype)
    for i0 in range(0, a.shape[0], 64):  # (blocks of queries bound the temporary)
        diff = a[i0:i0 + 64, None, :] - b[None, :, :]
        out[i0:i0 + 64] = (diff * diff).sum(axis=-1, dtype=dtype)
    return out


def nearest_two(a, b, dtype=np.float32, defect=None):
    """best_idx, best_d2, second_idx, second_d2 per query; the lower train index on equal d2.  One train descriptor:
    second_idx = -1, second_d2 = inf."""
    d2 = d2_matrix(a, b, dtype)
    nq, nt = d2.shape
    rows = np.arange(nq)

    def argmin(m):
        if defect == "tie_high":
            return nt - 1 - np.argmin(m[:, ::-1], axis=1)
        return np.argmin(m, axis=1)  # the first of equal minima

    bi = argmin(d2)
    bd = d2[rows, bi]
    if nt < 2:
        return bi.astype(np.int32), bd, np.full(nq, -1, np.int32), np.full(nq, np.inf, dtype)
    rest = d2.copy()
    rest[rows, bi] = np.inf
    si = argmin(rest)
    return bi.astype(np.int32), bd, si.astype(np.int32), rest[rows, si]


def knn_depth(uv, obs_uv, obs_depth, K, dtype=np.float32, defect=None):
    """(depth (n,) float32, neighbours (n, K) int32, -1 padded) of the pixels uv on one frame's observations."""
    uv, ouv = np.asarray(uv, dtype=dtype).reshape(-1, 2), np.asarray(obs_uv, dtype=dtype).reshape(-1, 2)
    od = np.asarray(obs_depth, dtype=np.float32)
    n, m = uv.shape[0], ouv.shape[0]
    k_used = K + 1 if defect == "k_off_by_one" else K
    k = min(k_used, m)
    dx, dy = ouv[None, :, 0] - uv[:, None, 0], ouv[None, :, 1] - uv[:, None, 1]
    d = dx * dx + dy * dy  # each product and the sum rounded to dtype
    order = np.argsort(d, axis=1, kind="stable")[:, :k]  # stable: the lower index on equal distance
    s = np.zeros(n)
    for j in range(k):  # summed in double in (distance, index) order
        s = s + od[order[:, j]].astype(np.float64)
    depth = (s / (k_used if defect == "mean_over_k" else k)).astype(np.float32)
    nb = np.full((n, K), -1, np.int32)
    nb[:, :min(k, K)] = order[:, :K]
    return depth, nb


def match_pair(frame0, frame1, intr, options=None, dtype=np.float32, defect=None):
    """One candidate.  frame: dict kp (n, 2) f32, desc (n, 64) f32, obs_uv (m, 2) f32, obs_depth (m,) f32; intr: dict
    focal, cx, cy, image_width, image_height.  Returns dict status, counts (nearest, after ratio, after border + skew,
    after uniqueness), the per-match arrays of sim3opt_match_batch_get_matches, and nn (nearest_two's four arrays)."""
    o = dict(DEFAULTS)
    o.update(options or {})
    nq, nt = frame0["kp"].shape[0], frame1["kp"].shape[0]
    empty = dict(counts=(0, 0, 0, 0), nn=None, query_idx=np.zeros(0, np.int32), train_idx=np.zeros(0, np.int32),
                 distance=np.zeros(0, np.float32), uv0=np.zeros((0, 2)), uv1=np.zeros((0, 2)), depth0=np.zeros(0),
                 depth1=np.zeros(0), points0=np.zeros((0, 3)))
    if nq == 0 or nt == 0:
        return dict(empty, status=NO_KEYPOINTS)
    if frame0["obs_uv"].shape[0] == 0 or frame1["obs_uv"].shape[0] == 0:
        return dict(empty, status=NO_MAP)
    bi, bd, si, sd = nearest_two(frame0["desc"], frame1["desc"], dtype, defect)
    # ratio test (:1097): float distances, a float division
    keep = np.ones(nq, bool)
    if o["ratio"] > 0:
        d1, d2 = np.sqrt(bd.astype(np.float32)), np.sqrt(sd.astype(np.float32))
        with np.errstate(divide="ignore", invalid="ignore"):
            q = (d1 / d2) if defect == "ratio_inverted" else (d2 / d1)
            keep = (nt >= 2) & (((d1 == 0) & (d2 > 0)) | (q.astype(np.float64) > o["ratio"]))
    n_ratio = int(keep.sum())
    # border and skew (:1101-1106), in double on the float pixels
    w, h, r = intr["image_width"], intr["image_height"], o["border_ratio"]
    p0, p1 = frame0["kp"].astype(np.float64), frame1["kp"][bi].astype(np.float64)
    x_lo, x_hi, y_lo, y_hi = r * w, (1 - r) * w, r * h, (1 - r) * h
    ge = (lambda a, b: a > b) if defect == "border_gt" else (lambda a, b: a >= b)
    border = np.ones(nq, bool)
    for p in (p0, p1):
        border &= ge(p[:, 0], x_lo) & ge(p[:, 1], y_lo) & (p[:, 0] <= x_hi) & (p[:, 1] <= y_hi)
    sx, sy = (o["skew_y"], o["skew_x"]) if defect == "skew_swapped" else (o["skew_x"], o["skew_y"])
    skew = (np.abs(p1[:, 1] - p0[:, 1]) < sy * h) & (np.abs(p1[:, 0] - p0[:, 0]) < sx * w)
    keep &= border & skew
    n_filters = int(keep.sum())
    # uniqueness (:1128-1160): per train index the smallest d2, the lower query index on equal d2
    cand = np.nonzero(keep)[0]
    qkey = -cand if defect == "uniq_lt" else cand
    order = np.lexsort((qkey, bd[cand], bi[cand]))  # by train index, then d2, then query index
    sorted_c = cand[order]
    first = np.ones(sorted_c.shape[0], bool)
    first[1:] = bi[sorted_c][1:] != bi[sorted_c][:-1]
    surv = sorted_c[first]  # (in train-index order here)
    if defect != "arrival_order":
        surv = np.sort(surv)  # ascending query index
    mq, mt = surv.astype(np.int32), bi[surv]
    K = o["knn_k"]
    kp0, kp1 = frame0["kp"][mq], frame1["kp"][mt]
    z0, _ = knn_depth(kp0, frame0["obs_uv"], frame0["obs_depth"], K, dtype, defect)
    z1, _ = knn_depth(kp0 if defect == "side1_keypoint0" else kp1, frame1["obs_uv"], frame1["obs_depth"], K, dtype,
                      defect)
    uv0, uv1 = kp0.astype(np.float64), kp1.astype(np.float64)
    z = z0.astype(np.float64)
    pts = np.stack([z * ((uv0[:, 0] - intr["cx"]) / intr["focal"]), z * ((uv0[:, 1] - intr["cy"]) / intr["focal"]), z],
                   axis=1)
    return dict(status=OK, counts=(nq, n_ratio, n_filters, int(surv.shape[0])), nn=(bi, bd, si, sd), query_idx=mq,
                train_idx=mt.astype(np.int32), distance=np.sqrt(bd[surv].astype(np.float32)), uv0=uv0, uv1=uv1,
                depth0=z, depth1=z1.astype(np.float64), points0=pts)


def match_batch(frames, pairs, intr, options=None, dtype=np.float32, defect=None):
    """Every pair; returns (list of match_pair results, match_ptr)."""
    res = [match_pair(frames[a], frames[b], intr, options, dtype, defect) for a, b in pairs]
    ptr = np.zeros(len(res) + 1, np.int32)
    ptr[1:] = np.cumsum([r["query_idx"].shape[0] for r in res])
    return res, ptr
