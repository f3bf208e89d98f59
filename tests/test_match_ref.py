"""tests/match_ref.py against a brute-force loop on tiny inputs, and its sensitivity to one-line defects on the cases
of tests/match_cases.py (no GPU): a defect that changed nothing there would be one the GPU tests could not see."""
import math

import numpy as np
import pytest

import match_cases as MC
import match_ref as R

f32 = np.float32


def brute_force(frame0, frame1, intr, o):
    """The definition of include/sim3opt.h as loops over scalars, one candidate."""
    nq, nt = len(frame0["kp"]), len(frame1["kp"])
    if nq == 0 or nt == 0:
        return R.NO_KEYPOINTS, []
    if len(frame0["obs_uv"]) == 0 or len(frame1["obs_uv"]) == 0:
        return R.NO_MAP, []
    w, h, r = intr["image_width"], intr["image_height"], o["border_ratio"]
    good = []
    for i in range(nq):
        best, second = (f32(np.inf), -1), (f32(np.inf), -1)
        for j in range(nt):
            d = f32(0)
            for k in range(64):
                t = f32(frame0["desc"][i, k] - frame1["desc"][j, k])
                d = f32(d + f32(t * t))
            if d < best[0]:
                best, second = (d, j), best
            elif d < second[0]:
                second = (d, j)
        if o["ratio"] > 0:
            if nt < 2:
                continue
            d1, d2 = f32(math.sqrt(best[0])), f32(math.sqrt(second[0]))
            if not ((d1 == 0 and d2 > 0) or (d1 > 0 and float(f32(d2 / d1)) > o["ratio"])):
                continue
        (x0, y0), (x1, y1) = map(float, frame0["kp"][i]), map(float, frame1["kp"][best[1]])
        if not (x0 >= r * w and y0 >= r * h and x0 <= (1 - r) * w and y0 <= (1 - r) * h and x1 >= r * w and
                y1 >= r * h and x1 <= (1 - r) * w and y1 <= (1 - r) * h):
            continue
        if abs(y1 - y0) < o["skew_y"] * h and abs(x1 - x0) < o["skew_x"] * w:
            good.append([i, best[1], best[0]])
    unique = {}  # kittiDetector.h:1128-1149, with d2 for the distance
    for m in good:
        if m[1] in unique:
            if unique[m[1]][2] <= m[2]:
                m[1] = -1
            else:
                unique[m[1]][1] = -1
                unique[m[1]] = m
        else:
            unique[m[1]] = m
    # (the loop above marks by trainIdx = -1 what :1142 / :1145 mark; collect the rest in order)
    kept = sorted(v for v in unique.values())
    out = []
    for i, j, d in kept:
        z = []
        for (u, v), fr in ((frame0["kp"][i], frame0), (frame1["kp"][j], frame1)):
            dist = []
            for n, (a, b) in enumerate(fr["obs_uv"]):
                dx, dy = f32(a - u), f32(b - v)
                dist.append((f32(f32(dx * dx) + f32(dy * dy)), n))
            dist.sort()
            near = dist[:o["knn_k"]]
            s = 0.0
            for _, n in near:
                s += float(fr["obs_depth"][n])
            z.append(float(f32(s / len(near))))
        u, v = map(float, frame0["kp"][i])
        out.append((i, j, f32(math.sqrt(d)), z[0], z[1],
                    (z[0] * ((u - intr["cx"]) / intr["focal"]), z[0] * ((v - intr["cy"]) / intr["focal"]), z[0])))
    return R.OK, out


def tiny(seed, nq, nt, m0, m1):
    rng = np.random.default_rng(seed)
    w, h = 64, 32
    pool, homes = rng.integers(0, 256, (6, 64)), rng.integers([8, 5], [56, 27], (6, 2))

    def frame(n, m):
        pick = rng.integers(0, 6, n)
        d = pool[pick].copy()
        d[:, 0] = np.clip(d[:, 0] + rng.integers(-1, 2, n), 0, 255)
        return dict(kp=(homes[pick] + rng.integers(-2, 3, (n, 2))).astype(f32), desc=(d / 256.0).astype(f32),
                    obs_uv=rng.integers(0, 32, (m, 2)).astype(f32), obs_depth=rng.uniform(1, 9, m).astype(f32))
    return frame(nq, m0), frame(nt, m1), dict(focal=40.0, cx=31.5, cy=15.5, image_width=w, image_height=h)


@pytest.mark.parametrize("seed,nq,nt,m0,m1,opts", [
    (0, 9, 7, 10, 3, {}),
    (1, 12, 12, 6, 7, dict(ratio=1.1)),
    (2, 5, 1, 4, 9, dict(ratio=1.1)),
    (3, 14, 9, 20, 20, dict(knn_k=2, border_ratio=0.2, skew_x=0.2, skew_y=0.3)),
    (4, 0, 5, 3, 3, {}),
    (5, 5, 5, 0, 3, {}),
])
def test_restatement_is_the_brute_force_loop(seed, nq, nt, m0, m1, opts):
    f0, f1, intr = tiny(seed, nq, nt, m0, m1)
    o = dict(R.DEFAULTS)
    o.update(opts)
    status, want = brute_force(f0, f1, intr, o)
    got = R.match_pair(f0, f1, intr, opts)
    assert got["status"] == status
    assert got["query_idx"].tolist() == [m[0] for m in want]
    assert got["train_idx"].tolist() == [m[1] for m in want]
    assert got["distance"].tolist() == [m[2] for m in want]
    assert got["depth0"].tolist() == [m[3] for m in want] and got["depth1"].tolist() == [m[4] for m in want]
    assert got["points0"].tolist() == [list(m[5]) for m in want]
    assert got["counts"][3] == len(want)


def test_tiny_cases_are_not_vacuous():
    n = [len(brute_force(*tiny(s, *dims)[:2], tiny(s, *dims)[2], dict(R.DEFAULTS, **o))[1])
         for s, *dims, o in [(0, 9, 7, 10, 3, {}), (1, 12, 12, 6, 7, dict(ratio=1.1))]]
    assert min(n) >= 2, n


def _flat(res):
    return [(r["status"], r["counts"], r["query_idx"].tolist(), r["train_idx"].tolist(), r["depth0"].tolist(),
             r["depth1"].tolist()) for r in res]


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_cases_reach_every_defect(defect):
    """Each planted one-line mistake changes the result on at least one case."""
    cases = {"ratio_inverted": (MC.ratio,), "border_gt": (MC.boundaries,)}.get(defect, (MC.ratio, MC.boundaries, MC.tiles))
    changed = [c.__name__ for c in cases if _flat(MC.reference(c, defect)[0]) != _flat(MC.reference(c)[0])]
    assert changed, f"no case of {[c.__name__ for c in cases]} notices {defect}"


def test_tiles_case_straddles_every_size():
    c = MC.tiles()
    kp = sorted({f["kp"].shape[0] for f in c["frames"]})
    for t in (MC.WAVE, MC.TRAIN_TILE, MC.QUERY_TILE):
        assert {t - 1, t, t + 1} <= set(kp)
    assert {0, 1, 2 * MC.QUERY_TILE + 1} <= set(kp)
    obs = {f["obs_uv"].shape[0] for f in c["frames"]}
    assert {0, 1, MC.K - 1, MC.K, MC.K + 1, MC.OBS_CHUNK - 1, MC.OBS_CHUNK, MC.OBS_CHUNK + 1} <= obs
    res, ptr = MC.reference(MC.tiles)
    st = [r["status"] for r in res]
    assert R.NO_KEYPOINTS in st and R.NO_MAP in st
    # the stages all have work: every filter removes something somewhere, and plenty survives
    tot = np.sum([r["counts"] for r in res], axis=0)
    assert tot[0] > tot[2] > tot[3] > 1000, tot
    # ties in both places: a best d2 shared by two train descriptors ...
    assert any(r["nn"] is not None and (r["nn"][1] == r["nn"][3]).any() for r in res)
    # ... and two queries that pass the filters with one train index at equal d2, of which uniqueness keeps the lower:
    # the kept set under "<" for "<=" is the reference's own filters with the other tie rule, so a pair where the two
    # differ by a query with an equal (train index, d2) partner is such a tie
    other, _ = MC.reference(MC.tiles, "uniq_lt")
    ties = 0
    for r, o in zip(res, other):
        if r["nn"] is None:
            continue
        bi, bd = r["nn"][0], r["nn"][1]
        kept = {(int(bi[q]), float(bd[q])): int(q) for q in r["query_idx"]}  # (one survivor per train index)
        for q2 in sorted(set(o["query_idx"].tolist()) - set(r["query_idx"].tolist())):
            q = kept[(int(bi[q2]), float(bd[q2]))]  # the same train index at the same d2 ...
            assert q < q2                             # ... and the lower query index is the one that is kept
            ties += 1
    assert ties > 0


def test_quantised_d2_is_exact():
    for fn in MC.QUANTISED:
        c = fn()
        for f in c["frames"]:
            q = f["desc"].astype(np.float64) * 256
            assert (q == np.round(q)).all() and q.min(initial=0) >= 0 and q.max(initial=0) < 256
    f0, f1 = MC.tiles()["frames"][3], MC.tiles()["frames"][5]
    assert (R.d2_matrix(f0["desc"], f1["desc"], np.float32) == R.d2_matrix(f0["desc"], f1["desc"], np.float64)).all()


def test_gaussian_case_has_a_gap():
    """The float64 restatement's nearest and second-nearest d2 differ by more than 1e-4 relative for every query, so
    FP32 rounding of a 64-term sum (below 1e-5 relative) decides no comparison; and the planted match is found."""
    c = MC.gaussian()
    bi, bd, si, sd = R.nearest_two(c["frames"][0]["desc"], c["frames"][1]["desc"], np.float64)
    assert ((sd - bd) > 1e-4 * sd).all()
    assert (bi == c["planted"]).all()
    b32 = R.nearest_two(c["frames"][0]["desc"], c["frames"][1]["desc"], np.float32)
    assert (b32[0] == bi).all() and (b32[2] == si).all()
