"""The cases of the batched vocabulary training, shared by tests/test_vocab_ref.py (the restatement's own checks, no
GPU) and tests/test_gpu_vocab_train.py.  Every coordinate is a multiple of 2^-8 in [-1, 1], so every sum of coordinates
is exact in double in any order and the device's centres must equal the restatement's bit for bit; a d2 between two
descriptors is exact too, so W of a seeding round is.  A case is a dict: name, kp_ptr, desc, options, and `converged`
(every node converged and no two children of a node have one centre: the descent equals the clustering)."""
import functools

import numpy as np

import vocab_ref as VR

TILES = dict(chunk=256, mean_chunk=1024)  # sim3opt_vocabulary_dims; the GPU test asserts they are these
Q = 256.0


def blobs(sizes, rng, noise=4):
    """len(sizes) planted groups: a centre of multiples of 1/256 in [-0.7, 0.7] and members off by up to noise/256 in
    every dimension; the groups are some hundred times further apart than they are wide.  Returns (desc, group)."""
    rows, group = [], []
    for g, n in enumerate(sizes):
        c = rng.integers(-180, 181, size=64)
        rows.append((c[None, :] + rng.integers(-noise, noise + 1, size=(n, 64))) / Q)
        group += [g] * n
    return np.concatenate(rows).astype(np.float32), np.asarray(group)


def in_frames(name, desc, rng, n_frames, options, empty=(2,), first=None, converged=True, group=None):
    """Shuffles the descriptors over n_frames frames (those in `empty` own none); `first`: rows that open every
    non-empty frame (a word present in every frame)."""
    order = rng.permutation(len(desc))
    desc = desc[order]
    owners = [f for f in range(n_frames) if f not in empty]
    cuts = np.sort(rng.choice(np.arange(1, len(desc)), size=len(owners) - 1, replace=False))
    parts = np.split(np.arange(len(desc)), cuts)
    rows, kp_ptr, it = [], [0], iter(parts)
    for f in range(n_frames):
        part = [] if f in empty else next(it)
        d = desc[part]
        if first is not None and f not in empty:
            d = np.concatenate([np.asarray(first, dtype=np.float32).reshape(-1, 64), d])
        rows.append(d)
        kp_ptr.append(kp_ptr[-1] + len(d))
    return dict(name=name, kp_ptr=np.asarray(kp_ptr, dtype=np.int32), desc=np.concatenate(rows).astype(np.float32),
                options=dict(options), converged=converged)


def line(xs):
    """Descriptors on the first axis at xs / 256."""
    d = np.zeros((len(xs), 64), dtype=np.float32)
    d[:, 0] = np.asarray(xs) / Q
    return d


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = []
    rng = np.random.default_rng(100)
    # the general shape: ten-ary, three levels, nodes of every kind
    rng = np.random.default_rng(101)
    d, _ = blobs([60] * 10, rng, noise=40)
    cases.append(in_frames("k10_L3", d, rng, 7, dict(k=10, levels=3, seed=1)))
    # binary, and a root that is the last level
    rng = np.random.default_rng(102)
    d, _ = blobs([40] * 8, rng, noise=30)
    cases.append(in_frames("k2_L3", d, rng, 5, dict(k=2, levels=3, seed=2)))
    cases.append(in_frames("k2_L1", d[:90], rng, 3, dict(k=2, levels=1, seed=3), empty=()))
    # the widest node: 64 centres in LDS, then nodes of fewer than k members
    rng = np.random.default_rng(103)
    d, _ = blobs([5] * 70, rng, noise=20)
    cases.append(in_frames("k64_L2", d, rng, 4, dict(k=64, levels=2, seed=4)))
    # groups of 3, 4, 5 and 9 under k = 4: a node of n < k, of n = k and of n = k + 1 at level 1
    rng = np.random.default_rng(104)
    d, _ = blobs([3, 4, 5, 9], rng)
    cases.append(in_frames("n_around_k", d, rng, 3, dict(k=4, levels=2, seed=SEEDS["n_around_k"]), empty=(1,)))
    # groups of every tile size minus one, exactly, plus one: their nodes at level 1 straddle the chunks of the
    # assignment and of the mean; the root is a node of several mean chunks
    rng = np.random.default_rng(105)
    sizes = [t + m for t in (TILES["chunk"], TILES["mean_chunk"]) for m in (-1, 0, 1)]
    d, _ = blobs(sizes, rng, noise=12)
    cases.append(in_frames("tile_sizes", d, rng, 9, dict(k=6, levels=2, seed=SEEDS["tile_sizes"], max_iters=30)))
    # duplicates: twelve copies of one descriptor (their node's seeding ends with one centre: a leaf at level 1, and
    # with a copy opening every frame a word of weight 0), a group of two values (a seeding that ends with two centres),
    # three copies under k = 6 (children of one centre: the later ones are leaves no descent reaches), a single
    # descriptor far away (a leaf at level 1 beside subtrees)
    rng = np.random.default_rng(106)
    d, _ = blobs([30, 25], rng, noise=25)
    extra, _ = blobs([1, 1, 1, 1, 1], rng)
    same, pair, triple, alone = extra[0:1], extra[1:3], extra[3:4], extra[4:5]
    pair[1] = pair[0]
    pair[1, :8] += 6 / Q
    d = np.concatenate([d, np.repeat(same, 8, axis=0), np.repeat(pair, 6, axis=0), np.repeat(triple, 3, axis=0), alone])
    cases.append(in_frames("duplicates_unbalanced", d, rng, 5, dict(k=6, levels=3, seed=SEEDS["duplicates_unbalanced"]),
                           first=same, converged=False))
    cases.append(dict(cases[-1], name="duplicates_idf0", options=dict(cases[-1]["options"], idf=0)))
    # a cluster that goes empty, and an exact tie between two centres: points on a line, found by search on the CPU
    for name, xs, opts in (("empty_cluster", EMPTY_XS, EMPTY_OPTS), ("exact_tie", TIE_XS, TIE_OPTS)):
        cases.append(dict(name=name, kp_ptr=np.asarray([0, len(xs) // 2, len(xs)], dtype=np.int32), desc=line(xs),
                          options=dict(opts), converged=True))
    # stopped by max_iters: uniform descriptors do not settle in two passes
    rng = np.random.default_rng(107)
    d = (rng.integers(-256, 257, size=(400, 64)) / Q).astype(np.float32)
    cases.append(in_frames("capped", d, rng, 6, dict(k=5, levels=2, max_iters=2, seed=7), converged=False))
    return tuple(cases)


# seeds chosen on the CPU (tests/test_vocab_ref.py asserts what they were chosen for)
SEEDS = dict(n_around_k=0, tile_sizes=0, duplicates_unbalanced=1)
EMPTY_XS, EMPTY_OPTS = (-84, -40, 216, -36, -4, -148, 184, -24, 132), dict(k=3, levels=1, seed=6117)
TIE_XS, TIE_OPTS = (112, -136, -160, 36, -88, -240, -40, 140, -60, -44, 92), dict(k=4, levels=1, seed=48)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement's Training of a case, computed once."""
    case = next(c for c in all_cases() if c["name"] == name)
    return VR.train(case["kp_ptr"], case["desc"], **case["options"])


def planted(seed=None):
    """Gaussian groups, not quantised: 4 groups of 4 subgroups, sigma 0.01, every two centres at least 20 sigma apart;
    k = 4 at two levels.  Returns the case and the subgroup of every descriptor."""
    rng = np.random.default_rng(200)
    sigma = 0.01
    top = rng.uniform(-0.6, 0.6, size=(4, 64))
    sub = top[:, None, :] + rng.uniform(-0.1, 0.1, size=(4, 4, 64))
    cen = sub.reshape(16, 64)
    gaps = np.sqrt(((cen[:, None, :] - cen[None, :, :]) ** 2).sum(-1)) + 1e9 * np.eye(16)
    assert gaps.min() >= 20 * sigma
    label = np.repeat(np.arange(16), 25)
    desc = (cen[label] + sigma * rng.standard_normal((len(label), 64))).astype(np.float32)
    order = rng.permutation(len(label))
    desc, label = desc[order], label[order]
    kp_ptr = np.asarray([0, 90, 90, 200, 310, 400], dtype=np.int32)
    case = dict(name="planted", kp_ptr=kp_ptr, desc=desc,
                options=dict(k=4, levels=2, seed=PLANTED_SEED if seed is None else seed), converged=True)
    return case, label


PLANTED_SEED = 0


def one_group_per_leaf(assignment, label):
    """Every leaf holds the descriptors of exactly one planted group and every group sits in one leaf."""
    pairs = set(zip((int(a) for a in assignment), (int(g) for g in label)))
    return len(pairs) == len(set(label)) == len({a for a, _ in pairs})


@functools.lru_cache(maxsize=None)
def end_to_end():
    """The planted revisit of tests/place_cases.py (descriptors around the leaves of a coded 8-ary tree of 3 levels),
    trained with that tree's k and L, then detected on the trained tree.  dict: case, training (the restatement's), voc
    (place_ref.Vocabulary of the trained tree), detection (place_ref.detect on it)."""
    import place_cases as PCS
    import place_ref as PR
    src = next(c for c in PCS.all_cases() if c["name"] == "revisit")
    case = dict(name="end_to_end", kp_ptr=src["kp_ptr"], desc=src["desc"], options=dict(k=8, levels=3, seed=5),
                converged=True, place_options=dict(src["options"]))
    T = VR.train(case["kp_ptr"], case["desc"], **case["options"])
    voc = PR.Vocabulary(T.parent, T.centre, T.weight, T.word_id)
    return dict(case=case, training=T, voc=voc, detection=PR.detect(voc, case["kp_ptr"], case["desc"], **src["options"]))
