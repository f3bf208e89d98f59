"""The SURF-64 definition of include/sim3opt.h ("batched SURF-64 extraction") restated in numpy, independently of
sim3opt_amd/csrc/surf_host.hpp: written from the header's text alone, in double (exact integers for the integral
image), numpy.linalg.solve for the interpolation, numpy.arctan2 for the angles, numpy.sin / cos for the rotation.  It is
not bit-compatible with the library and is not meant to be.  Only the discrete choices that the definition makes in
FP32 -- s, g and win of a keypoint, which decide array shapes -- are taken in FP32 here as well.

`defects` names one-line defects (DEFECTS) that tests/test_surf_ref.py switches on to show that each changes an output.
"""
import numpy as np

DXX = [(0, 2, 3, 7, 1), (3, 2, 6, 7, -2), (6, 2, 9, 7, 1)]
DYY = [(y1, x1, y2, x2, w) for x1, y1, x2, y2, w in DXX]
DXY = [(1, 1, 4, 4, 1), (5, 1, 8, 4, -1), (1, 5, 4, 8, -1), (5, 5, 8, 8, 1)]
HAAR_X = [(0, 0, 2, 4, -1), (2, 0, 4, 4, 1)]
HAAR_Y = [(0, 0, 4, 2, 1), (0, 2, 4, 4, -1)]
OPTIONS = dict(hessian_threshold=400.0, n_octaves=4, n_octave_layers=3, upright=0, max_keypoints=0)
DEFECTS = ("dyy_not_transposed", "weight_0.9", "ge_for_gt", "margin_off_by_one", "centre_without_half", "x_wrong_sign",
           "gaussian_wrong_sigma", "window_without_wrap", "unrotated_window", "subregions_in_column_order",
           "no_normalisation")
OK, NO_KEYPOINTS = 0, 1
F = np.float32


def integral(img):
    img = np.asarray(img)
    S = np.zeros((img.shape[0] + 1, img.shape[1] + 1), dtype=np.int64)
    S[1:, 1:] = img.astype(np.int64).cumsum(0).cumsum(1)
    return S


def resize(pattern, old, new):
    r = new / old
    out = []
    for x1, y1, x2, y2, w in pattern:
        a, b, c, d = (int(np.rint(r * v)) for v in (x1, y1, x2, y2))
        out.append((a, b, c, d, w / ((c - a) * (d - b))))
    return out


def boxes_at(S, boxes, ys, xs):
    """The response of `boxes` anchored at every (y, x) of ys x xs.  The boxes of one pattern have one area, so the
    sum is taken over the integers first (weight x area is -2, -1 or 1) and divided once: equal pixels give equal
    responses whatever the order of the boxes, as in exact arithmetic."""
    ys, xs = np.asarray(ys)[:, None], np.asarray(xs)[None, :]
    areas = {(x2 - x1) * (y2 - y1) for x1, y1, x2, y2, _ in boxes}
    assert len(areas) == 1
    area = areas.pop()
    num = np.zeros((ys.shape[0], xs.shape[1]), dtype=np.int64)
    for x1, y1, x2, y2, w in boxes:
        num += int(np.rint(w * area)) * (S[ys + y1, xs + x1] + S[ys + y2, xs + x2] - S[ys + y2, xs + x1] - S[ys + y1, xs + x2])
    return num / float(area)


def layer_size(o, l):
    return (9 + 6 * l) << o


def response_plane(S, o, l, defects=()):
    """(det, trace), (h // step) x (w // step), zero outside the samples"""
    h, w = S.shape[0] - 1, S.shape[1] - 1
    step, size = 1 << o, layer_size(o, l)
    det, tr = np.zeros((h // step, w // step)), np.zeros((h // step, w // step))
    if size > h or size > w:
        return det, tr
    ni, nj, m = 1 + (h - size) // step, 1 + (w - size) // step, (size // 2) // step
    ys, xs = np.arange(ni) * step, np.arange(nj) * step
    dx = boxes_at(S, resize(DXX, 9, size), ys, xs)
    dy = boxes_at(S, resize(DXX if "dyy_not_transposed" in defects else DYY, 9, size), ys, xs)
    dxy = boxes_at(S, resize(DXY, 9, size), ys, xs)
    det[m:m + ni, m:m + nj] = dx * dy - (0.9 if "weight_0.9" in defects else 0.81) * dxy * dxy
    tr[m:m + ni, m:m + nj] = dx + dy
    return det, tr


def candidates(S, opts, defects=(), slack=0.0):
    """The strict maxima above the threshold in scan order, each a dict; `margin` is the least of det - threshold and
    det - the largest neighbour (what a rounding of det would have to overcome to change the set).  slack > 0 lists
    the positions of margin > -slack as well: what a rounding of that size could turn into a candidate."""
    h, w = S.shape[0] - 1, S.shape[1] - 1
    nl, thr = opts["n_octave_layers"], float(opts["hessian_threshold"])
    out = []
    for o in range(opts["n_octaves"]):
        step, rows, cols = 1 << o, h >> o, w >> o
        planes = [response_plane(S, o, l, defects) for l in range(nl + 2)]
        for l in range(1, nl + 1):
            size = layer_size(o, l)
            m = (layer_size(o, l + 1) // 2) // step + 1 + ("margin_off_by_one" in defects)
            if rows - 2 * m <= 0 or cols - 2 * m <= 0:
                continue
            D = np.stack([planes[l - 1][0], planes[l][0], planes[l + 1][0]])
            c = D[1, m:rows - m, m:cols - m]
            nb = np.full(c.shape, -np.inf)
            for q in range(3):
                for di in (-1, 0, 1):
                    for dj in (-1, 0, 1):
                        if (q, di, dj) != (1, 0, 0):
                            nb = np.maximum(nb, D[q, m + di:rows - m + di, m + dj:cols - m + dj])
            hit = (c > thr) & ((c >= nb) if "ge_for_gt" in defects else (c > nb))
            if slack > 0:
                hit = np.minimum(c - thr, c - nb) > -slack
            for a, b in zip(*np.nonzero(hit)):
                i, j = int(a) + m, int(b) + m
                half = 0.0 if "centre_without_half" in defects else (size - 1) * 0.5
                cand = dict(octave=o, layer=l, i=i, j=j, key=((o * nl + l - 1) * h + i) * w + j,
                            x0=step * (j - (size // 2) // step) + half, y0=step * (i - (size // 2) // step) + half,
                            size0=float(size), response=float(c[a, b]), laplacian=int(np.sign(planes[l][1][i, j])),
                            margin=float(min(c[a, b] - thr, c[a, b] - nb[a, b])))
                N = D[:, i - 1:i + 2, j - 1:j + 2]
                bvec = -np.array([(N[1, 1, 2] - N[1, 1, 0]) / 2, (N[1, 2, 1] - N[1, 0, 1]) / 2, (N[2, 1, 1] - N[0, 1, 1]) / 2])
                axy = (N[1, 2, 2] - N[1, 2, 0] - N[1, 0, 2] + N[1, 0, 0]) / 4
                axs = (N[2, 1, 2] - N[2, 1, 0] - N[0, 1, 2] + N[0, 1, 0]) / 4
                ays = (N[2, 2, 1] - N[2, 0, 1] - N[0, 2, 1] + N[0, 0, 1]) / 4
                A = np.array([[N[1, 1, 0] - 2 * N[1, 1, 1] + N[1, 1, 2], axy, axs],
                              [axy, N[1, 0, 1] - 2 * N[1, 1, 1] + N[1, 2, 1], ays],
                              [axs, ays, N[0, 1, 1] - 2 * N[1, 1, 1] + N[2, 1, 1]]])
                try:
                    x = np.linalg.solve(A, bvec)
                    kept = bool(np.any(x != 0) and np.all(np.abs(x) <= 1))
                except np.linalg.LinAlgError:
                    x, kept = np.zeros(3), False
                if "x_wrong_sign" in defects:
                    x = -x
                cand.update(kept=kept, shift=x, x=cand["x0"], y=cand["y0"], size=cand["size0"])
                if kept:
                    cand.update(x=cand["x0"] + x[0] * step, y=cand["y0"] + x[1] * step,
                                size=float(np.rint(size + x[2] * (size - layer_size(o, l - 1)))))
                out.append(cand)
    return out


def gaussian(n, sigma):
    x = np.arange(n) - (n - 1) * 0.5
    g = np.exp(-x * x / (2 * sigma * sigma))
    return g / g.sum()


def geometry(size):
    """s, g, win as the definition's FP32 operations give them"""
    s = F(F(F(size) * F(1.2)) / F(9.0))
    return float(s), 2 * int(np.rint(F(2) * s)), int(F(21) * s)


def atan2deg(y, x):
    return np.mod(np.degrees(np.arctan2(y, x)), 360.0)


def orientation(S, x, y, size, defects=()):
    """dict: valid, vx, vy, angle (113 each), window (72), angle_out; None when no sample counts"""
    h, w = S.shape[0] - 1, S.shape[1] - 1
    s, g, _ = geometry(size)
    g13 = gaussian(13, 2.0 if "gaussian_wrong_sigma" in defects else 2.5)
    pts = [(i, j) for i in range(-6, 7) for j in range(-6, 7) if i * i + j * j <= 36]
    hx, hy = resize(HAAR_X, 4, max(g, 2)), resize(HAAR_Y, 4, max(g, 2))
    valid, vx, vy = np.zeros(113, dtype=bool), np.zeros(113), np.zeros(113)
    for k, (i, j) in enumerate(pts):
        px, py = int(np.rint(x + i * s - (g - 1) / 2)), int(np.rint(y + j * s - (g - 1) / 2))
        if g < 2 or not (0 <= px < w + 1 - g and 0 <= py < h + 1 - g):
            continue
        wt = g13[i + 6] * g13[j + 6]
        valid[k], vx[k], vy[k] = True, boxes_at(S, hx, [py], [px])[0, 0] * wt, boxes_at(S, hy, [py], [px])[0, 0] * wt
    if not valid.any():
        return None
    ang = np.where(valid, atan2deg(vy, vx), 0.0)
    win, sums = np.zeros(72), np.zeros((72, 2))
    for c in range(72):
        d = np.abs(np.rint(ang) - 5 * c)
        m = valid & ((d < 30) if "window_without_wrap" in defects else ((d < 30) | (d > 330)))
        sums[c] = vx[m].sum(), vy[m].sum()
        win[c] = sums[c, 0] ** 2 + sums[c, 1] ** 2
    b = int(np.argmax(win))
    bx, by = (sums[b] if win[b] > 0 else (0.0, 0.0))
    return dict(valid=valid, vx=vx, vy=vy, angle=ang, window=win, angle_out=float(atan2deg(-by, bx)))


def window(img, x, y, angle, win):
    """the win x win window turned by `angle` about (x, y)"""
    h, w = img.shape
    sin_dir, cos_dir = -np.sin(np.radians(angle)), np.cos(np.radians(angle))
    f = np.arange(win) - (win - 1) / 2
    fi, fj = f[:, None], f[None, :]
    px, py = x + fj * cos_dir + fi * sin_dir, y - fj * sin_dir + fi * cos_dir
    ix, iy = np.floor(px).astype(int), np.floor(py).astype(int)
    inside = (ix >= 0) & (iy >= 0) & (ix < w - 1) & (iy < h - 1)
    cx, cy = np.clip(ix, 0, w - 2) if w > 1 else ix * 0, np.clip(iy, 0, h - 2) if h > 1 else iy * 0
    im = img.astype(float)
    if w > 1 and h > 1:
        a, b = px - ix, py - iy
        bil = np.rint(im[cy, cx] * (1 - a) * (1 - b) + im[cy, cx + 1] * a * (1 - b) + im[cy + 1, cx] * (1 - a) * b +
                      im[cy + 1, cx + 1] * a * b)
    else:
        bil = np.zeros(px.shape)
    near = im[np.clip(np.rint(py), 0, h - 1).astype(int), np.clip(np.rint(px), 0, w - 1).astype(int)]
    return np.where(inside, bil, near)


def area_weights(win):
    """21 x win: the share of sample i in cell u"""
    scale = win / 21.0
    u, i = np.arange(21)[:, None], np.arange(win)[None, :]
    return np.clip(np.minimum((u + 1) * scale, i + 1) - np.maximum(u * scale, i), 0, None), scale


def patch_of(img, x, y, angle, win):
    W, scale = area_weights(win)
    return np.clip(np.rint(W @ window(img, x, y, angle, win) @ W.T / (scale * scale)), 0, 255)


def descriptor(img, x, y, size, angle, defects=()):
    _, _, win = geometry(size)
    if win < 1:
        return None, None
    patch = patch_of(img, x, y, 0.0 if "unrotated_window" in defects else angle, win)
    g20 = gaussian(20, 3.3)
    dw = np.outer(g20, g20)
    vx = (patch[:-1, 1:] - patch[:-1, :-1] + patch[1:, 1:] - patch[1:, :-1]) * dw
    vy = (patch[1:, :-1] - patch[:-1, :-1] + patch[1:, 1:] - patch[:-1, 1:]) * dw
    d = []
    for r in range(16):
        i, j = (r % 4, r // 4) if "subregions_in_column_order" in defects else (r // 4, r % 4)
        a, b = vx[5 * i:5 * i + 5, 5 * j:5 * j + 5], vy[5 * i:5 * i + 5, 5 * j:5 * j + 5]
        d += [a.sum(), b.sum(), np.abs(a).sum(), np.abs(b).sum()]
    d = np.array(d)
    if "no_normalisation" not in defects:
        d = d / (np.sqrt((d * d).sum()) + np.finfo(np.float32).eps)
    return d, patch


def extract(img, defects=(), **options):
    """dict: kp (n, 2), desc (n, 64), size, angle, response, octave, laplacian, status, counts (candidates,
    interpolated, dropped), S, candidates (scan order)"""
    opts = dict(OPTIONS, **options)
    img = np.asarray(img, dtype=np.uint8)
    S = integral(img)
    cand = candidates(S, opts, defects)
    kept = sorted((c for c in cand if c["kept"]), key=lambda c: (-c["response"], c["key"]))
    if opts["max_keypoints"] > 0:
        kept = kept[:opts["max_keypoints"]]
    rows, dropped = [], 0
    for c in kept:
        angle = 270.0
        _, g, _ = geometry(c["size"])
        if not opts["upright"]:
            o = orientation(S, c["x"], c["y"], c["size"], defects)
            angle = None if o is None else o["angle_out"]
        elif g > img.shape[0] + 1 or g > img.shape[1] + 1:
            angle = None
        d = descriptor(img, c["x"], c["y"], c["size"], angle, defects)[0] if angle is not None else None
        if d is None:
            dropped += 1
            continue
        rows.append((c["x"], c["y"], c["size"], angle, c["response"], c["octave"], c["laplacian"], d))
    col = lambda k, t=float: np.array([r[k] for r in rows], dtype=t)
    return dict(kp=np.array([[r[0], r[1]] for r in rows]).reshape(-1, 2), desc=np.array([r[7] for r in rows]).reshape(-1, 64),
                size=col(2), angle=col(3), response=col(4), octave=col(5, int), laplacian=col(6, int),
                status=OK if rows else NO_KEYPOINTS,
                counts=(len(cand), sum(c["kept"] for c in cand), dropped), S=S, candidates=cand)
