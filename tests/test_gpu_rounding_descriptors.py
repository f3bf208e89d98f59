"""Vocabulary training and place recognition on the GPU (sim3opt_amd/csrc/vocab_train.hip, place_batch.hip) bit for bit
against the order-exact restatement of include/sim3opt.h (vocab_ref.train(exact=True), place_ref.detect(exact=True),
tests/rounding_ref.py), on descriptors that round (tests/rounding_cases.py).  The committed lattice cases make every sum
exact in any order; here an FP32 accumulator, partial sums, squares in double, another scan, FSurf64's mean, a fused
multiply-add or another association of a term changes a double that is read out, as tests/test_rounding_ref.py shows
on the CPU for each of them.

Both sides follow one arithmetic, so every integer is equal and every double and FP32 is equal as bytes, with no mask
and no excused entry.  The one exception is the weights: log on the host, within 1e-14 (a few ulp of libm below log
16384 < 10); the restatement of place recognition is fed the device's weights, so everything after them is exact again.
The frames reach both handles through one FrameStore (set_frames_from).  PARITY UNPINNED, as the stages themselves."""
import functools

import numpy as np
import pytest

import place_ref as PR
import rounding_cases as RC
import rounding_ref as RR
import surf_cases as SC
import vocab_ref as VR
from sim3opt_amd import lib as L

pytestmark = pytest.mark.gpu

CASES = ("surf_like", "subnormal_squares", "device_surf")


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).reshape(-1).view(np.uint64)


def n_different(got, want):
    got, want = bits(got), bits(want)
    assert got.shape == want.shape
    return int((got != want).sum())


@functools.lru_cache(maxsize=None)
def frames_of(name):
    """(case, kp_ptr, desc) as host arrays; device_surf: the extractor's output read back from the store it filled.
    Computed once; do not modify."""
    if name != "device_surf":
        case = next(c for c in RC.cpu_cases() if c["name"] == name)
        return case, case["kp_ptr"], case["desc"]
    surf, store = L.SurfBatch(), L.FrameStore()
    surf.set_images(SC.mixed_batch())
    assert surf.solve_into(store) >= 2
    ptr, _, desc = store.get()
    surf.close()
    store.close()
    assert ptr[-1] > RR.RUN and ptr[1] == ptr[7] - ptr[6] > 0  # (several runs of 256; frames 0 and 6 are one image)
    return RC.DEVICE_SURF, ptr, desc


def store_of(name):
    """A FrameStore holding the case's frames (the keypoints are not read by either stage)"""
    _, ptr, desc = frames_of(name)
    s = L.FrameStore()
    s.set(ptr, np.zeros((len(desc), 2), dtype=np.float32), desc)
    assert same(s.get()[2], desc)
    return s


@functools.lru_cache(maxsize=None)
def training(name):
    """The exact restatement's Training on the case's frames, once; do not modify."""
    if name != "device_surf":
        return RC.training(name)
    case, ptr, desc = frames_of(name)
    return VR.train(ptr, desc, exact=True, **case["options"])


def train_on_device(name):
    """(trainer, store) after train(), fed through the store"""
    case, _, _ = frames_of(name)
    store = store_of(name)
    t = L.VocabularyTrainer(**case["options"])
    t.set_frames_from(store)
    t.train()
    return t, store


@pytest.mark.parametrize("name", CASES)
def test_training_bit_for_bit(name):
    case, ptr, desc = frames_of(name)
    R = training(name)
    k, D = case["options"]["k"], int(ptr[-1])
    t, store = train_on_device(name)
    parent, centre, weight, word_id = t.vocabulary()
    assert list(parent) == list(R.parent) and list(word_id) == list(R.word_id)
    a, d = t.assignment(descent=True)
    assert list(a) == list(R.assignment) and list(d) == list(R.descent)
    dims = t.dims()
    assert (dims["n_nodes"], dims["n_words"], dims["depth"], dims["n_unconverged"]) == \
        (len(R.parent), int((R.word_id >= 0).sum()), R.depth, R.n_unconverged)
    assert dims["passes"] == R.passes and dims["n_frames"] == len(ptr) - 1 and dims["total_descriptors"] == D
    print("centre coordinates that differ:", int((centre.view(np.uint32) != R.centre.view(np.uint32)).sum()), "of", centre.size)
    assert same(centre, R.centre)
    print("largest weight error:", np.abs(weight - R.weight).max())
    assert np.all(np.abs(weight - R.weight) <= 1e-14)
    # the seeding of every node: the chosen members, W and r of every round
    n_rounds = 0
    for node in range(len(R.parent)):
        s, ref = t.debug_seeding(node), R.seeding.get(node, dict(members=[], W=[], r=[]))
        assert list(s["members"]) == ref["members"], node
        assert same(s["W"], np.array(ref["W"], dtype=np.float64)), (node, list(s["W"]), ref["W"])
        assert same(s["r"], np.array(ref["r"], dtype=np.float64)), (node, list(s["r"]), ref["r"])
        n_rounds += len(ref["W"])
    assert n_rounds >= 1
    # the iterates: before the first pass, after pass 1 and after the last pass of every level
    for level in range(len(R.levels)):
        for n_pass in sorted({0, min(1, R.passes[level]), R.passes[level]}):
            got = t.debug_lloyd(level, n_pass)
            first, cluster, centres = VR.lloyd_state(R, level, n_pass, k, D)
            assert got["first_node"] == first and list(got["cluster"]) == list(cluster), (level, n_pass)
            assert same(got["centre"], centres), (level, n_pass)
    if name == "subnormal_squares":  # every square is a subnormal FP32: W > 0 and the seeding went on
        s = t.debug_seeding(0)
        assert 0 < s["W"][0] < 2.0 ** -126 and len(s["members"]) == 2 and dims["n_nodes"] > 3
    t.close()
    store.close()


@pytest.mark.parametrize("name", CASES)
def test_place_recognition_bit_for_bit_on_the_device_trained_tree(name):
    case, ptr, desc = frames_of(name)
    n = len(ptr) - 1
    t, store = train_on_device(name)
    voc = t.vocabulary()
    t.close()
    T = training(name)
    assert list(voc[0]) == list(T.parent) and same(voc[1], T.centre) and list(voc[3]) == list(T.word_id)
    tree = PR.Vocabulary(*voc)  # (the device's weights: everything below is exact)
    R = PR.detect(tree, ptr, desc, exact=True, **case["place_options"])
    b = L.PlaceBatch(**case["place_options"])
    b.set_vocabulary(*voc)
    b.set_frames_from(store)
    n_candidates = b.solve()
    # the words and the winning d2 of every level, of every descriptor
    words, path = b.debug_words(desc)
    assert list(words) == [w for f in R.words for w in f]
    want = np.array([p + [-1.0] * (tree.depth - len(p)) for p in R.paths], dtype=np.float64).reshape(len(desc), tree.depth)
    print("path_d2 values that differ:", n_different(path, want), "of", want.size)
    assert same(path, want)
    # the vectors
    bow_ptr, w, v = b.bow()
    assert list(np.diff(bow_ptr)) == [len(x) for x in R.vectors] and bow_ptr[0] == 0
    assert list(w) == [k for x in R.vectors for k in sorted(x)]
    want = np.array([x[k] for x in R.vectors for k in sorted(x)], dtype=np.float64)
    print("bow_value entries that differ:", n_different(v, want), "of", want.size)
    assert same(v, want)
    # per frame
    r = b.results()
    assert list(r["status"]) == R.status and list(r["match"]) == R.match
    assert list(r["n_consistent"]) == R.n_consistent and [tuple(x) for x in r["island"]] == R.island
    assert n_candidates == len(R.pairs) and [tuple(x) for x in b.pairs()] == R.pairs
    assert same(r["score"], np.array(R.score, dtype=np.float64)) and same(r["ns_factor"], np.array(R.ns_factor, dtype=np.float64))
    # every score row, the kept results and the islands of every query
    rows = np.stack([b.debug_scores(i) for i in range(n)])
    print("scores that differ:", n_different(rows, R.S), "of", R.S.size, "; non-zero:", int((R.S != 0).sum()))
    assert same(rows, R.S)
    for i in range(n):
        d = b.debug_islands(i)
        assert list(d["kept_j"]) == [j for j, _ in R.kept[i]]
        assert same(d["kept_score"], np.array([s for _, s in R.kept[i]], dtype=np.float64)), i
        assert [tuple(x) for x in d["island"]] == [(g["first"], g["last"], g["best_entry"], g["n"]) for g in R.islands[i]]
        assert same(d["island_score"], np.array([g["score"] for g in R.islands[i]], dtype=np.float64)), i
    if name == "surf_like":
        assert n_candidates >= 10 and max(len(x) for x in R.islands) >= 1
    if name == "device_surf":  # the repeated image is found
        assert (6, 0) in R.pairs
    b.close()
    store.close()


def test_a_descent_decided_by_a_subnormal_square():
    """Two leaves 2^-70 apart in one coordinate: each of the two descriptors is its own word by a d2 of 0 against one of
    2^-140; flushed, both d2 would be 0 and both words the lower child's."""
    voc, d, words = RC.subnormal_pair()
    b = L.PlaceBatch()
    b.set_vocabulary(*voc.arrays())
    got, path = b.debug_words(d)
    assert list(got) == words and path.tolist() == [[0.0], [0.0]]
    every = RC.subnormal_squares()["desc"]
    got, path = b.debug_words(every)
    ref = [PR.word_of(voc, x, d2=RR.d2) for x in every]
    assert list(got) == [w for w, _ in ref] and same(path, np.array([p for _, p in ref], dtype=np.float64))
    assert 0 < path.max() < 2.0 ** -126 and len(set(path.reshape(-1))) >= 5
    b.close()
