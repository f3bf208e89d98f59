"""Descriptors that round: the cases on which vocabulary training and place recognition are compared bit for bit with
the order-exact restatement (vocab_ref.train(exact=True), place_ref.detect(exact=True); tests/test_rounding_ref.py on
the CPU, tests/test_gpu_rounding_descriptors.py on the device).  The committed cases of tests/vocab_cases.py and
tests/place_cases.py live on a lattice on which every sum is exact in any order; here no sum is, so an FP32
accumulator, partial sums, another scan, a fused multiply-add or another association changes a double that is read out.
The sizes are the smallest that reach every order the definition names, not the workload's.

A case is a dict: name, kp_ptr, desc, options (the training's), place_options."""
import functools

import numpy as np

import place_ref as PR
import vocab_ref as VR

N_SURF_LIKE = 2 * 1024 + 300  # the root: 10 runs of 256 of which the last is partial, 3 mean runs of 1024
SURF_LIKE_SEED = 11           # chosen on the CPU: tests/test_rounding_ref.py asserts what it was chosen for
PLACE_OPTIONS = dict(dislocal=4, k=1, alpha=0.3, max_db_results=50)  # lowered so that queries get past step 1


def surf_like_descriptors(n, rng, scale=None):
    """Unit-norm FP32 descriptors built as SURF-64 builds them: 16 cells of (sum dx, sum dy, sum |dx|, sum |dy|) over 9
    samples each, so the second pair of every four entries is non-negative and bounds the first.  The samples of a cell
    are scaled by a power of two between 2^-7 and 1 (scale: n x 16, drawn when None), so the entries of one descriptor
    span several binades."""
    if scale is None:
        scale = 2.0 ** rng.uniform(-7, 0, size=(n, 16))
    dx = rng.standard_normal((n, 16, 9)) * scale[:, :, None]
    dy = rng.standard_normal((n, 16, 9)) * scale[:, :, None]
    d = np.stack([dx.sum(-1), dy.sum(-1), np.abs(dx).sum(-1), np.abs(dy).sum(-1)], axis=-1).reshape(n, 64)
    return unit(d)


def unit(d):
    d = np.asarray(d, dtype=np.float64)
    return (d / np.sqrt((d * d).sum(-1, keepdims=True))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def surf_like(seed=SURF_LIKE_SEED):
    """2348 descriptors over 36 frames.  52 prototypes; frame f < 24 draws its descriptors around the prototypes 2 f ..
    2 f + 5, so neighbouring frames share words and frames further apart do not; the frames 24 .. 35 are noisy copies of
    the frames 0 .. 11, descriptor by descriptor: the planted revisit.  k = 4 at three levels: the nodes of level 1
    still span several runs of 256."""
    rng = np.random.default_rng(seed)
    proto = surf_like_descriptors(52, rng).astype(np.float64)
    sizes = [65] * 12 + [66] * 8 + [65] * 4
    assert sum(sizes) + sum(sizes[:12]) == N_SURF_LIKE
    frames = []
    for f, m in enumerate(sizes):
        which = 2 * f + rng.integers(6, size=m)
        frames.append(unit(proto[which] + 0.05 * surf_like_descriptors(m, rng)))
    for g in range(12):
        frames.append(unit(frames[g].astype(np.float64) + 0.01 * surf_like_descriptors(sizes[g], rng)))
    kp_ptr = np.concatenate([[0], np.cumsum([len(x) for x in frames])]).astype(np.int32)
    return dict(name="surf_like", kp_ptr=kp_ptr, desc=np.concatenate(frames), options=dict(k=4, levels=3, seed=seed),
                place_options=dict(PLACE_OPTIONS))


TINY = 2.0 ** -70


@functools.lru_cache(maxsize=None)
def subnormal_squares():
    """Eight descriptors in four frames, equal in 63 coordinates and j 2^-70 in coordinate 5, j = 0 .. 7: every
    difference is a multiple of 2^-70 and every FP32 square a multiple of 2^-140, a subnormal (the smallest normal FP32
    is 2^-126).  With subnormals flushed every d2 would be 0, W would be 0 and the root a leaf; by the definition W > 0
    and the seeding goes on.  k = 2 at three levels."""
    base = surf_like_descriptors(1, np.random.default_rng(5))[0]
    desc = np.tile(base, (8, 1))
    desc[:, 5] = (np.array([3, 0, 6, 1, 7, 4, 2, 5]) * TINY).astype(np.float32)
    return dict(name="subnormal_squares", kp_ptr=np.array([0, 2, 4, 6, 8], dtype=np.int32), desc=desc,
                options=dict(k=2, levels=3, seed=2), place_options=dict(PLACE_OPTIONS, dislocal=1, k=0))


def subnormal_pair():
    """(vocabulary, descriptors, words): a root with two leaves whose centres are two descriptors of subnormal_squares
    2^-70 apart, and those two descriptors: each is its own word, by a d2 of 0 against one of 2^-140."""
    d = subnormal_squares()["desc"][[1, 3]]
    voc = PR.Vocabulary([-1, 0, 0], np.concatenate([np.zeros((1, 64), np.float32), d]), [0.0, 1.0, 1.0], [-1, 0, 1])
    return voc, d, [0, 1]


def cpu_cases():
    return (surf_like(), subnormal_squares())


@functools.lru_cache(maxsize=None)
def training(name):
    """The exact restatement's Training of a CPU case, computed once; do not modify."""
    case = next(c for c in cpu_cases() if c["name"] == name)
    return VR.train(case["kp_ptr"], case["desc"], exact=True, **case["options"])


def vocabulary_of(T):
    return PR.Vocabulary(T.parent, T.centre, T.weight, T.word_id)


@functools.lru_cache(maxsize=None)
def detection(name):
    """The exact restatement's Detection of a CPU case on its own trained tree, computed once; do not modify."""
    case = next(c for c in cpu_cases() if c["name"] == name)
    return PR.detect(vocabulary_of(training(name)), case["kp_ptr"], case["desc"], exact=True, **case["place_options"])


# device_surf (GPU only): the SurfBatch output of tests/surf_cases.mixed_batch() through a FrameStore -- real SURF
# descriptors, of which the restatement is fed the read-back.  Frames 0 and 6 are one image; its neighbours are other
# scenes, so the score against the frame before is no measure here (use_nss = 0) and one query is a candidate (k = 0).
DEVICE_SURF = dict(name="device_surf", options=dict(k=4, levels=3, seed=3),
                   place_options=dict(PLACE_OPTIONS, dislocal=2, k=0, use_nss=0))
