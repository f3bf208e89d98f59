"""The cases of the batched bag-of-words place recognition, shared by tests/test_place_ref.py (the restatement's own
checks, no GPU) and tests/test_gpu_place_batch.py.  Centres and descriptors are multiples of 1/64 of small magnitude,
so every d2 is exact in any order of summation.  A case is a dict: name, voc (place_ref.Vocabulary), kp_ptr, desc,
options, and for some `expect` (frame -> status)."""
import functools

import numpy as np

import place_ref as PR

# the sizes at which the kernels change path (sim3opt_place_batch_dims; the GPU test asserts they are these)
TILES = dict(wavefront=64, workgroup=256, bow_chunk=1024, score_lds=2048, score_frames=64, lds_nodes=128)
BITS = 6  # a node's children are told apart by a 6-bit code in the dimensions of their level


def coded_tree(spec, seed, zero_every=0, unit_weights=False):
    """spec: None for a leaf, a list of specs for an inner node.  Nodes are numbered as DBoW2 creates them (all children
    of a node, then each child's subtree), which is not breadth first; word ids are a permutation of the leaves."""
    rng = np.random.default_rng(seed)
    parent, centre, leaf = [-1], [np.zeros(64, dtype=np.float32)], []

    def expand(i, sub, level):
        if sub is None:
            leaf.append(i)
            return
        kids = []
        for c, _ in enumerate(sub):
            v = centre[i].copy()
            for b in range(BITS):
                v[level * BITS + b] = (c >> b) & 1
            parent.append(i)
            centre.append(v)
            kids.append(len(parent) - 1)
        for k, s in zip(kids, sub):
            expand(k, s, level + 1)

    expand(0, spec, 0)
    n = len(parent)
    word_id, weight = np.full(n, -1, dtype=np.int32), np.zeros(n)
    perm = rng.permutation(len(leaf))
    for w, i in zip(perm, leaf):
        word_id[i] = w
        weight[i] = 1.0 if unit_weights else rng.integers(8, 25) / 8.0
        if zero_every and w % zero_every == zero_every - 1:
            weight[i] = 0.0
    voc = PR.Vocabulary(parent, np.stack(centre), weight, word_id)
    voc.leaf_of_word = np.zeros(len(leaf), dtype=np.int64)
    for i in leaf:
        voc.leaf_of_word[word_id[i]] = i
    return voc


def balanced(arity, levels):
    return None if levels == 0 else [balanced(arity, levels - 1) for _ in range(arity)]


def descriptors(voc, words, rng):
    """One descriptor per word: its leaf's centre off by up to 2/64 in every dimension, which no descent can mistake
    (a wrong child is at least 1 - 4/64 further)."""
    words = np.asarray(words, dtype=np.int64)
    noise = rng.integers(-2, 3, size=(len(words), 64)) / 64.0
    return (voc.centre[voc.leaf_of_word[words]] + noise).astype(np.float32).reshape(-1, 64)


def from_word_lists(name, voc, word_lists, seed, options=None, copies=None, extra=None, expect=None):
    """copies: frame -> the earlier frame whose descriptors it repeats exactly; extra: frame -> descriptors put first"""
    rng = np.random.default_rng(seed)
    rows, kp_ptr = [], [0]
    for f, w in enumerate(word_lists):
        if copies and f in copies:
            d = rows[copies[f]]
        else:
            d = descriptors(voc, w, rng)
            if extra and f in extra:
                d = np.concatenate([np.asarray(extra[f], dtype=np.float32).reshape(-1, 64), d])
        rows.append(d)
        kp_ptr.append(kp_ptr[-1] + len(d))
    desc = np.concatenate(rows) if kp_ptr[-1] else np.zeros((0, 64), dtype=np.float32)
    return dict(name=name, voc=voc, kp_ptr=np.asarray(kp_ptr, dtype=np.int32), desc=desc, options=dict(options or {}),
                expect=expect or {})


def revisit(name, voc, seed, n_places, words_per_place, n_own, n_next, path, options=None, expect=None):
    """Place p owns words_per_place words no other place owns; a frame at p is n_own descriptors of p's words and n_next
    of the next place's."""
    rng = np.random.default_rng(seed)
    lists = []
    for p in path:
        q = (p + 1) % n_places
        lists.append(list(p * words_per_place + rng.integers(words_per_place, size=n_own)) +
                     list(q * words_per_place + rng.integers(words_per_place, size=n_next)))
    return from_word_lists(name, voc, lists, seed + 1, options, expect=expect)


def linked(name, voc, seed, n_frames, links, options, n_slots=32, prev=6, copies=None, sizes=None):
    """Frames of n_slots distinct words: `prev` of the frame before's own words, links[f][j] of frame j's own words, the
    rest its own.  With unit weights s(f, j) = links[f][j] / n_slots and ns = prev / n_slots."""
    own, lists, nxt = [], [], 0
    for f in range(n_frames):
        if copies and f in copies:
            own.append(own[copies[f]])
            lists.append(lists[copies[f]])
            continue
        lo = prev if copies and f - 1 in copies else 0  # (a copy's follower shares other words than the original's)
        w = list(own[f - 1][lo:lo + prev]) if f else []
        for j, c in links.get(f, {}).items():
            w += own[j][-c:]
        mine = list(range(nxt, nxt + n_slots - len(w)))
        assert len(mine) >= prev + 8
        nxt += len(mine)
        own.append(mine)
        lists.append((w + mine)[:sizes[f]] if sizes and f in sizes else w + mine)
    assert nxt <= len(voc.word_weight)
    return from_word_lists(name, voc, lists, seed, options, copies=copies)


@functools.lru_cache(maxsize=None)
def vocabularies():
    v = dict(
        tree8x3=coded_tree(balanced(8, 3), 1, zero_every=7),       # 512 words, every seventh of weight 0
        flat512=coded_tree(balanced(8, 3), 2, unit_weights=True),  # the same shape, every weight 1
        tree3x2=coded_tree(balanced(3, 2), 3, zero_every=4),
        # a node of one child whose child has 64 leaves, a leaf at the first level, an inner node of two leaves
        unbalanced=coded_tree([[[None] * 64], None, [None, None]], 4),
        wide=coded_tree(balanced(64, 2), 5),                       # 4096 words: frames longer than SCORE_LDS
    )
    for m in (-1, 0, 1):  # 1 + 64 + (lds_nodes - 65 + m) nodes: the staged part of the tree ends at, before, after the last
        v[f"nodes{m:+d}"] = coded_tree([[None] * (TILES["lds_nodes"] - 65 + m)] + [None] * 63, 6 + m)
    v["trap"] = trap_vocabulary()
    return v


def trap_vocabulary():
    """A 3-ary tree of 2 levels with centres chosen by hand: first-level centres A = (0, 0), B = (2, 0), C = (0, 8)."""
    c = np.zeros((13, 64), dtype=np.float32)
    xy = [(0, 0), (0, 0), (2, 0), (0, 8), (-1, 0), (-1.5, 0), (-0.5, 1), (1, 0), (3, 0), (3.5, 0), (0, 8), (0, 9), (0, 10)]
    c[:, :2] = xy
    parent = [-1, 0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3]
    word_id = [-1, -1, -1, -1, 3, 0, 7, 1, 8, 2, 5, 4, 6]
    weight = [0, 0, 0, 0, 1.5, 1, 2, 1, 1.25, 3, 1, 2, 0.5]
    voc = PR.Vocabulary(parent, c, weight, word_id)
    voc.leaf_of_word = np.zeros(9, dtype=np.int64)
    for i, w in enumerate(word_id):
        if w >= 0:
            voc.leaf_of_word[w] = i
    return voc


def trap_descriptors():
    """(descriptors, expected words): at exactly equal d2 from A and B (the lower child A, then its leaf 6 = word 7);
    nearest to A at the first level while the nearest leaf of all is B's (1, 0) (greedy: A's leaf 6 = word 7); at
    exactly equal d2 from two leaves of C (the lower, node 10 = word 5)."""
    d = np.zeros((3, 64), dtype=np.float32)
    d[0, :2] = (1, 0)
    d[1, :2] = (0.875, 0)
    d[2, :2] = (0, 8.5)
    return d, [7, 7, 5]


REVISIT_PATH = list(range(30)) + list(range(3, 15))
# what the planted revisit gives with the defaults (frame -> status)
REVISIT_EXPECT = {**{i: PR.CLOSE_MATCHES_ONLY for i in range(21)}, **{i: PR.NO_DB_RESULTS for i in range(21, 29)},
                  29: PR.NO_TEMPORAL_CONSISTENCY, 30: PR.LOW_NSS_FACTOR, 31: PR.NO_TEMPORAL_CONSISTENCY,
                  32: PR.NO_TEMPORAL_CONSISTENCY, **{i: PR.CANDIDATE for i in range(33, 42)}}
REVISIT_MATCH = {29: 0, **{i: i - 27 for i in range(31, 42)}}  # frame 33 is at place 6, first seen at frame 6


def sequence_cases():
    V = vocabularies()
    small = dict(dislocal=2, k=1)
    cases = [
        revisit("revisit", V["tree8x3"], 10, 30, 12, 40, 12, REVISIT_PATH, expect=REVISIT_EXPECT),
        revisit("revisit_no_accumulate", V["tree8x3"], 10, 30, 12, 40, 12, REVISIT_PATH, dict(accumulate=0)),
        revisit("revisit_no_nss", V["tree8x3"], 10, 30, 12, 40, 12, REVISIT_PATH, dict(use_nss=0)),
        revisit("unbalanced_revisit", V["unbalanced"], 13, 11, 6, 17, 5, list(range(11)) + list(range(2, 8)),
                dict(dislocal=3, k=2)),
        revisit("tree3x2_revisit", V["tree3x2"], 12, 9, 1, 3, 2, list(range(9)) + list(range(9)), dict(dislocal=4, k=1)),
        linked("low_scores", V["flat512"], 20, 7, {5: {0: 1}}, small),
        linked("no_groups", V["flat512"], 21, 7, {5: {0: 6}}, dict(small, min_matches_per_group=2)),
        linked("two_islands_later_wins", V["flat512"], 22, 10, {8: {0: 3, 3: 4, 4: 5}}, small),
        linked("island_tie", V["flat512"], 23, 10, {8: {0: 4}}, small, copies={4: 0}),
        linked("max_db_results_cuts", V["flat512"], 24, 10, {8: {0: 3, 1: 5, 2: 4}}, dict(small, max_db_results=2)),
        linked("query_gap", V["flat512"], 25, 13, {6: {0: 3}, 7: {1: 3}, 10: {2: 3}, 11: {3: 3}}, small),
        linked("group_gap", V["flat512"], 26, 13, {8: {0: 3}, 9: {3: 3}, 10: {7: 3}, 11: {1: 3}}, small),
        linked("empty_and_single_frames", V["flat512"], 27, 10, {7: {0: 4}, 8: {1: 4}}, small, sizes={3: 0, 5: 1}),
        # frame 6 repeats frame 0 and alpha is 1: s(7, 0) equals its threshold ns = s(7, 6) by construction
        linked("threshold_met_exactly", V["flat512"], 30, 9, {}, dict(small, alpha=1.0), copies={6: 0}),
        linked("identical_database_frames", V["flat512"], 28, 8, {6: {0: 4}}, dict(small, max_db_results=1), copies={1: 0}),
    ]
    cases[5]["expect"] = {5: PR.LOW_SCORES}
    cases[6]["expect"] = {5: PR.NO_GROUPS}
    # the hand-made tree: some frames start with the special descriptors
    d, _ = trap_descriptors()
    lists = [[0, 1, 1], [1, 2, 2, 2], [3, 4], [8, 6, 6], [0, 0, 1, 3], [1, 2, 4, 4], [3, 3, 4, 4, 4, 0], [1, 1, 1, 2, 8]]
    cases.append(from_word_lists("trap_descents", V["trap"], lists, 29, dict(dislocal=4, k=0),
                                 extra={0: d, 3: d[1:], 5: d, 6: d[:1], 7: d[:2]}))
    return cases


def shape_cases():
    """Frame sizes and frame counts at every tile size minus one, exactly, plus one.  The frame counts are those at the
    tile sizes that bound frames (the database frames of a workgroup or wavefront round, the scan width of the
    per-query row); the longer tiles bound the entries of one frame."""
    V = vocabularies()
    rng = np.random.default_rng(40)
    sizes = [t + m for t in (TILES["wavefront"], TILES["workgroup"], TILES["bow_chunk"], TILES["score_lds"])
             for m in (-1, 0, 1)]
    # distinct words of the wide tree: the vector is as long as the frame; each frame takes half of the one before
    lists, before = [], None
    for s in sizes + [TILES["score_lds"] + 1, 300]:
        w = rng.permutation(4096)[:s]
        if before is not None:
            k = min(len(before), s) // 2
            w = np.concatenate([before[:k], np.setdiff1d(w, before[:k])[:s - k]])
        lists.append(list(w))
        before = w
    cases = [from_word_lists("frame_sizes", V["wide"], lists, 41, dict(dislocal=2, k=0))]
    # repeated words: the runs of the sorted words cross the scan width and the staged chunk
    lists = [list(rng.integers(40, size=s)) for s in (255, 257, 1023, 1025, 1300, 257)]
    cases.append(from_word_lists("frame_sizes_repeated_words", V["tree8x3"], lists, 42, dict(dislocal=2, k=0)))
    for n in [t + m for t in (TILES["score_frames"], TILES["workgroup"]) for m in (-1, 0, 1)]:
        back = 24
        path = list(range(n - back)) + list(range(5, 5 + back))
        cases.append(revisit(f"frame_count_{n}", V["wide"], 50 + n, n - back, 8, 12, 4, path))
    for m in (-1, 0, 1):
        voc = V[f"nodes{m:+d}"]
        nw = len(voc.word_weight)
        cases.append(revisit(f"tree_of_{len(voc.parent)}_nodes", voc, 60 + m, nw // 3, 3, 5, 2,
                             list(range(nw // 3)) + list(range(2, 10)), dict(dislocal=5, k=1)))
    return cases


@functools.lru_cache(maxsize=None)
def all_cases():
    return tuple(sequence_cases() + shape_cases())


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement's Detection of a case, computed once."""
    case = next(c for c in all_cases() if c["name"] == name)
    return PR.detect(case["voc"], case["kp_ptr"], case["desc"], **case["options"])


@functools.lru_cache(maxsize=None)
def chain_case():
    """The planted revisit with geometry for the stages after it: the frames 30..41 repeat the descriptors of the frames
    27 earlier, shuffled and moved by 1/64 in four dimensions, and either frame of such a pair sees one 3-D scene of
    tests/pnp_cases.py (the later frame is camera 0).  dict: the case's keys, kp, obs_depth (the keypoints are the
    observations) and revisits ((query, match), ...)."""
    import pnp_cases as PC
    case = dict(revisit("chain", vocabularies()["tree8x3"], 10, 30, 12, 40, 12, REVISIT_PATH))
    rng = np.random.default_rng(70)
    ptr, desc = case["kp_ptr"], case["desc"].copy()
    n = len(ptr) - 1
    kp = np.stack([rng.uniform(200, 1000, ptr[-1]), rng.uniform(60, 300, ptr[-1])], axis=1)
    depth = rng.uniform(6.0, 40.0, ptr[-1])
    revisits = tuple((q, q - 27) for q in range(30, n))
    for q, m in revisits:
        size = ptr[m + 1] - ptr[m]
        perm = rng.permutation(size)
        rows = desc[ptr[m]:ptr[m + 1]][perm]
        for r in rows:
            r[rng.choice(64, size=4, replace=False)] += rng.choice([-1.0, 1.0], size=4) / 64.0
        desc[ptr[q]:ptr[q + 1]] = rows
        scene = PC.make_case(int(size), 300 + q)
        uv0 = PC._project(np.eye(3), np.zeros(3), scene["points"])
        kp[ptr[m]:ptr[m + 1]] = scene["uv1"]
        kp[ptr[q]:ptr[q + 1]] = uv0[perm]
        depth[ptr[q]:ptr[q + 1]] = scene["points"][perm, 2]
    case.update(desc=desc, kp=kp.astype(np.float32), obs_depth=depth.astype(np.float32), revisits=revisits)
    return case
