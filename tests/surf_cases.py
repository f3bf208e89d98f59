"""The images of the SURF-64 tests: seeded and synthetic, at the smallest sizes at which a path of the extraction can go
wrong (tests/test_surf_ref.py, tests/test_gpu_surf_batch.py).  reference(name) is the numpy restatement's result
(tests/surf_ref.py), computed once per process and shared."""
import functools

import numpy as np

import surf_ref as R

GREY, NOISE_SIGMA = 110.0, 2.0


def _finish(f, rng):
    if rng is not None:
        f = f + rng.normal(0.0, NOISE_SIGMA, f.shape)
    return np.clip(np.rint(f), 0, 255).astype(np.uint8)


def render_blobs(w, h, blobs, seed=None):
    """Gaussian blobs (x, y, sigma, amplitude) on grey 110, with noise of sigma 2 when seeded"""
    yy, xx = np.mgrid[0:h, 0:w].astype(float)
    f = np.full((h, w), GREY)
    for x, y, s, a in blobs:
        f += a * np.exp(-((xx - x) ** 2 + (yy - y) ** 2) / (2 * s * s))
    return _finish(f, None if seed is None else np.random.default_rng(seed))


# (a) 176 x 120: blobs of both signs, sigma 2.5 .. 7, amplitude >= 80, apart by more than their filters
BLOBS_A = ((30.0, 28.0, 2.5, 100.0), (88.3, 30.6, 4.0, -90.0), (142.7, 34.2, 5.5, 120.0), (48.4, 84.9, 7.0, -100.0),
           (120.2, 86.5, 3.2, 80.0))
# (b) 131 x 97: odd in both axes
BLOBS_B = ((28.0, 25.0, 3.0, 110.0), (75.5, 30.5, 4.5, -95.0), (104.0, 66.0, 2.8, 100.0), (40.2, 66.7, 5.0, 90.0))
# (c) 300 x 280: octaves 2 and 3 have layers of a handful of samples and layers of none
BLOBS_C = ((60.0, 60.0, 4.0, 100.0), (200.0, 70.0, 12.0, -100.0), (110.0, 190.0, 20.0, 110.0), (240.0, 220.0, 7.0, 90.0))
# (g) one pattern for the rotations, square and off-centre.  An isotropic blob has no orientation, and one with
# companions has several nearly equal ones, so the blobs (with two weaker companions each) sit on a linear ramp that
# turns with them: the ramp adds nothing to the Hessian's determinant and gives every gradient sum one direction
_G_MAIN = ((40.0, 38.0, 3.0, 100.0, 20.0), (92.0, 44.0, 4.5, -95.0, 110.0), (60.0, 96.0, 6.0, 110.0, 200.0),
           (104.0, 100.0, 3.5, 90.0, 290.0), (70.0, 66.0, 2.6, -100.0, 335.0))
G_SIDE, G_AMPLITUDE, G_SLOPE, G_RAMP_DIRECTION = 140, 0.5, 1.0, 40.0


def _companions(x, y, s, a, phi):
    at = lambda deg, r: (x + r * s * np.cos(np.radians(deg)), y + r * s * np.sin(np.radians(deg)))
    a *= G_AMPLITUDE
    return ((x, y, s, a), at(phi, 1.8) + (0.8 * s, 0.7 * a), at(phi + 100.0, 1.8) + (0.7 * s, 0.35 * a))


BLOBS_G = tuple(b for m in _G_MAIN for b in _companions(*m))


def smooth(f, sigma):
    k = np.exp(-0.5 * (np.arange(-int(3 * sigma), int(3 * sigma) + 1) / sigma) ** 2)
    k /= k.sum()
    f = np.apply_along_axis(lambda r: np.convolve(np.pad(r, len(k) // 2, mode="reflect"), k, mode="valid"), 1, f)
    return np.apply_along_axis(lambda r: np.convolve(np.pad(r, len(k) // 2, mode="reflect"), k, mode="valid"), 0, f)


def textured(w, h, seed, sigma=2.5):
    """smoothed noise, contrast stretched: keypoints everywhere, the borders included"""
    f = smooth(np.random.default_rng(seed).normal(0.0, 1.0, (h, w)), sigma)
    f = (f - f.min()) / (f.max() - f.min())
    return np.clip(np.rint(255 * f), 0, 255).astype(np.uint8)


def checkerboard(w, h, cell=8, lo=40, hi=210):
    """cells of even side: every peak of the response lies between samples and ties with its mirror images"""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.where(((xx // cell) + (yy // cell)) % 2 == 0, lo, hi).astype(np.uint8)


SQUARES = tuple((x, y) for y in (40, 80) for x in (40, 80, 120))  # the centres of six equal 7 x 7 squares


def squares(w=176, h=120, lo=60, hi=200):
    """Equal squares 40 apart (a multiple of every octave's step): bit-equal responses, so the order is the tie rule's"""
    f = np.full((h, w), lo, dtype=np.uint8)
    for x, y in SQUARES:
        f[y - 3:y + 4, x - 3:x + 4] = hi
    return f


def turn(x, y, deg):
    """(x, y) of the (g) pattern turned by `deg` about the image centre, in numpy.rot90's sense: at 90 degrees (x, y)
    goes to (y, side - 1 - x)"""
    c, t = (G_SIDE - 1) / 2, np.radians(deg)
    return c + np.cos(t) * (x - c) + np.sin(t) * (y - c), c - np.sin(t) * (x - c) + np.cos(t) * (y - c)


def rotated_blobs(deg):
    """The (g) pattern turned by `deg`.  Multiples of 90 are the pattern at 0 turned as an array, an exact index
    permutation; any other angle is rendered anew from the turned centres and the turned ramp."""
    if deg % 90 == 0 and deg != 0:
        return np.ascontiguousarray(np.rot90(rotated_blobs(0), (deg // 90) % 4))
    c = (G_SIDE - 1) / 2
    yy, xx = np.mgrid[0:G_SIDE, 0:G_SIDE].astype(float)
    f = np.full((G_SIDE, G_SIDE), 128.0)
    for x, y, s, a in BLOBS_G:
        x, y = turn(x, y, deg)
        f += a * np.exp(-((xx - x) ** 2 + (yy - y) ** 2) / (2 * s * s))
    ux, uy = turn(c + np.cos(np.radians(G_RAMP_DIRECTION)), c + np.sin(np.radians(G_RAMP_DIRECTION)), deg)
    f += G_SLOPE * ((xx - c) * (ux - c) + (yy - c) * (uy - c))
    return _finish(f, np.random.default_rng(7))


@functools.lru_cache(maxsize=None)
def image(name):
    if name == "blobs":
        return render_blobs(176, 120, BLOBS_A, seed=1)
    if name == "noise":
        return render_blobs(176, 120, (), seed=1)
    if name == "odd":
        return render_blobs(131, 97, BLOBS_B, seed=2)
    if name == "large":
        return render_blobs(300, 280, BLOBS_C, seed=3)
    if name == "small":
        return render_blobs(40, 36, ((20.0, 18.0, 3.0, 100.0),), seed=4)
    if name == "tiny":
        return render_blobs(12, 12, ((6.0, 6.0, 2.5, 100.0),), seed=5)
    if name == "textured":
        return textured(200, 150, seed=6)
    if name == "textured_large":  # (e) on the device: more than two of the ranking's tiles of 256 keys
        return textured(MIXED_W, MIXED_H, seed=8)
    if name == "constant":
        return np.full((120, 176), 128, dtype=np.uint8)
    if name == "checker":
        return checkerboard(176, 120)
    if name == "squares":
        return squares()
    if name.startswith("mixed_"):  # the images of the mixed batch, at its one size
        return _mixed(name[6:])
    if name.startswith("rot"):
        return rotated_blobs(int(name[3:]))
    raise KeyError(name)


SINGLE = ("blobs", "noise", "odd", "large", "small", "tiny", "textured", "textured_large", "constant", "checker", "squares")
# (h) one size, 7 images: the textured one has more than 512 candidates, so next to it the workgroups of the ranking's
# later tiles find nothing of the small images and return
MIXED_W, MIXED_H = 320, 240
MIXED = ("blobs", "textured", "constant", "checker", "noise", "squares", "blobs")


def _mixed(kind):
    if kind == "blobs":
        return render_blobs(MIXED_W, MIXED_H, BLOBS_A, seed=1)
    if kind == "textured":
        return image("textured_large")
    if kind == "constant":
        return np.full((MIXED_H, MIXED_W), 128, dtype=np.uint8)
    if kind == "checker":
        return checkerboard(MIXED_W, MIXED_H)
    if kind == "noise":
        return render_blobs(MIXED_W, MIXED_H, (), seed=1)
    if kind == "squares":
        return squares(MIXED_W, MIXED_H)
    raise KeyError(kind)


def mixed_batch():
    return np.stack([image("mixed_" + n) for n in MIXED])


@functools.lru_cache(maxsize=None)
def reference(name, **options):
    return R.extract(image(name), **options)
