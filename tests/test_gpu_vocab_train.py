"""The batched vocabulary training on the GPU (sim3opt_vocabulary, sim3opt_amd/csrc/vocab_train.hip) against
tests/vocab_ref.py, an independent restatement of the definition in include/sim3opt.h.  PARITY UNPINNED (the reference
tree holds neither DBoW2's source nor a vocabulary file): what is compared is the restatement and planted truth.  The
cases are tests/vocab_cases.py's; tests/test_vocab_ref.py shows on the CPU that they keep every deciding comparison
1e-9 from a tie, reach the paths they were made for and catch the mistakes a kernel could make.

parent, word_id, assignment, dims and the seeding's members are equal; the centres are equal bit for bit (the
coordinates are multiples of 2^-8, so a double sum of them is exact in any order).  W and r are within 1e-12 relative:
double sums of at most a few thousand non-negative terms in another order.  The weights are within 1e-14 absolute: they
are below log 16384 < 10 and differ by a few ulp of libm."""
import numpy as np
import pytest

import place_ref as PR
import vocab_cases as VC
import vocab_ref as VR
from sim3opt_amd import lib as L

pytestmark = pytest.mark.gpu


def make(case, **opts):
    t = L.VocabularyTrainer(**dict(case["options"], **opts))
    t.set_frames(case["kp_ptr"], case["desc"])
    return t


def case_named(name):
    return next(c for c in VC.all_cases() if c["name"] == name)


def snapshot(t):
    a, d = t.assignment(descent=True)
    return tuple(x.tobytes() for x in t.vocabulary() + (a, d))


def check_against(t, R, case):
    n_nodes = t.train()
    k = case["options"]["k"]
    parent, centre, weight, word_id = t.vocabulary()
    assert n_nodes == len(R.parent) and list(parent) == list(R.parent) and list(word_id) == list(R.word_id)
    assert centre.tobytes() == R.centre.astype(np.float32).tobytes()
    print("largest weight error:", np.abs(weight - R.weight).max())
    assert np.all(np.abs(weight - R.weight) <= 1e-14)
    a, d = t.assignment(descent=True)
    assert list(a) == list(R.assignment) and list(d) == list(R.descent)
    dims = t.dims()
    assert (dims["n_nodes"], dims["n_words"], dims["depth"], dims["n_unconverged"]) == \
        (len(R.parent), int((R.word_id >= 0).sum()), R.depth, R.n_unconverged)
    assert dims["passes"] == R.passes and dims["n_frames"] == len(case["kp_ptr"]) - 1
    assert dims["total_descriptors"] == case["kp_ptr"][-1]
    # the seeding of every node
    for node in range(n_nodes):
        s, ref = t.debug_seeding(node), R.seeding.get(node, dict(members=[], W=[], r=[]))
        assert list(s["members"]) == ref["members"] and len(s["W"]) == len(ref["W"]), node
        for x, y in zip(list(s["W"]) + list(s["r"]), ref["W"] + ref["r"]):
            assert abs(x - y) <= 1e-12 * abs(y), (node, x, y)
    return parent, centre, weight, word_id


@pytest.mark.parametrize("case", VC.all_cases(), ids=lambda c: c["name"])
def test_case_against_the_restatement(case):
    R = VC.reference(case["name"])
    t = make(case)
    voc = check_against(t, R, case)
    k, D = case["options"]["k"], int(case["kp_ptr"][-1])
    # the iterates: before the first pass, after pass 1 and after the last pass of every level
    for level in range(len(R.levels)):
        for n_pass in sorted({0, min(1, R.passes[level]), R.passes[level]}):
            got = t.debug_lloyd(level, n_pass)
            first, cluster, centres = VR.lloyd_state(R, level, n_pass, k, D)
            assert got["first_node"] == first and list(got["cluster"]) == list(cluster), (level, n_pass)
            assert got["centre"].tobytes() == centres.tobytes(), (level, n_pass)
    # the trained tree goes into place recognition as it is, and its descent is the one the weights were counted from
    p = L.PlaceBatch()
    p.set_vocabulary(*voc)
    words, _ = p.debug_words(case["desc"])
    assert list(words) == [int(R.word_id[i]) for i in R.descent]
    if case["converged"]:
        assert list(words) == [int(R.word_id[i]) for i in R.assignment]
    p.close()
    t.close()


def test_tile_sizes_are_the_ones_the_cases_straddle():
    t = L.VocabularyTrainer()
    d = t.dims()
    assert {k: d[k] for k in VC.TILES} == VC.TILES
    t.close()


def test_planted_groups_end_in_one_leaf_each():
    case, label = VC.planted()
    t = make(case)
    assert t.train() == 21 and t.dims()["n_words"] == 16 and t.dims()["n_unconverged"] == 0
    assert VC.one_group_per_leaf(t.assignment(), label)
    t.close()


def test_trainings_are_reproducible_bit_for_bit():
    """Two trainings of one handle, a training on a fresh handle, and one after another set of frames on the same
    handle: the same bits."""
    case = case_named("k10_L3")
    t = make(case)
    t.train()
    first = snapshot(t)
    t.train()
    assert snapshot(t) == first
    other = case_named("k2_L3")
    t.set_frames(other["kp_ptr"], other["desc"])
    t.train()
    t.set_frames(case["kp_ptr"], case["desc"])
    t.train()
    assert snapshot(t) == first
    u = make(case)
    u.train()
    assert snapshot(u) == first
    t.close()
    u.close()


def test_descriptors_appended_to_a_frame():
    """The last frame grows in a second set_frames: the result changes as the restatement says."""
    case = case_named("n_around_k")
    extra = case_named("k2_L1")["desc"][:7]
    t = make(case)
    check_against(t, VC.reference(case["name"]), case)
    kp_ptr = case["kp_ptr"].copy()
    kp_ptr[-1] += len(extra)
    longer = dict(case, kp_ptr=kp_ptr, desc=np.concatenate([case["desc"], extra]))
    t.set_frames(longer["kp_ptr"], longer["desc"])
    R = VR.train(longer["kp_ptr"], longer["desc"], **case["options"])
    assert VR.signature(R) != VR.signature(VC.reference(case["name"]))
    check_against(t, R, longer)
    t.close()


def test_end_to_end_through_place_recognition():
    """Train on the planted revisit, detect on the trained tree: status and match of every frame as place_ref.detect
    on the restatement's trained tree, which finds the planted revisits."""
    E = VC.end_to_end()
    case, R = E["case"], E["detection"]
    assert len(R.pairs) >= 1 and all(q - m == 27 for q, m in R.pairs)
    t = make(case)
    voc = check_against(t, E["training"], case)
    p = L.PlaceBatch(**case["place_options"])
    p.set_vocabulary(*voc)
    p.set_frames(case["kp_ptr"], case["desc"])
    assert p.solve() == len(R.pairs)
    r = p.results()
    assert list(r["status"]) == R.status and list(r["match"]) == R.match
    assert [tuple(x) for x in p.pairs()] == R.pairs
    p.close()
    t.close()


def test_save_and_load_keep_the_tree(tmp_path):
    case = case_named("k2_L3")
    t = make(case)
    t.train()
    voc = t.vocabulary()
    path = str(tmp_path / "voc.bin")
    L.vocabulary_save(path, *voc)
    back = L.vocabulary_load(path)
    assert all(x.tobytes() == y.tobytes() and x.dtype == y.dtype for x, y in zip(voc, back))
    t.close()


def test_refusals_and_device_memory():
    """Every refusal leaves the handle and the device memory as they were; all memory is back after close(); repeated
    trainings of one size and the read-outs keep none."""
    start = L.device_memory_in_use()
    case = case_named("k10_L3")
    t = make(case)
    t.train()
    held = L.device_memory_in_use()
    assert held[1] > start[1]
    first = snapshot(t)
    for _ in range(2):
        t.train()
        assert L.device_memory_in_use() == held
    t.debug_seeding(0)
    t.debug_lloyd(0, 1)
    t.debug_lloyd(1, 0)
    assert L.device_memory_in_use() == held and snapshot(t) == first
    for bad, msg in ((dict(k=1), "k outside 2..64"), (dict(k=65), "k outside 2..64"), (dict(levels=0), "levels outside 1..8"),
                     (dict(levels=9), "levels outside 1..8"), (dict(max_iters=0), "max_iters < 1"),
                     (dict(idf=2), "idf is neither 0 nor 1")):
        with pytest.raises(L.Sim3OptError) as e:
            t.set_options(**dict(case["options"], **bad))
        assert e.value.code == L.ERR_ARG and str(e.value).endswith("vocabulary_set_options: " + msg)
    same = np.tile(case["desc"][:1], (5, 1))
    nan = case["desc"][:5].copy()
    nan[3, 7] = np.nan
    for ptr, d, msg in (([0, 5], same, "fewer than two distinct descriptors"), ([0, 1], same, "fewer than two distinct descriptors"),
                        ([0, 0], same, "fewer than two distinct descriptors"), ([0, 5], nan, "a non-finite descriptor"),
                        ([1, 5], nan, "kp_ptr[0] must be 0"), ([0, 3, 2, 5], case["desc"], "kp_ptr is not monotone at frame 1")):
        with pytest.raises(L.Sim3OptError) as e:
            t.set_frames(ptr, d)
        assert e.value.code == L.ERR_ARG and str(e.value).endswith("vocabulary_set_frames: " + msg)
    with pytest.raises(L.Sim3OptError):
        t.debug_seeding(10 ** 6)
    with pytest.raises(L.Sim3OptError):
        t.debug_lloyd(0, 1000)
    with pytest.raises(L.Sim3OptError):
        t.debug_lloyd(7, 0)
    assert L.device_memory_in_use() == held and snapshot(t) == first and t.options()["k"] == 10
    t.close()
    assert L.device_memory_in_use() == start
    fresh = L.VocabularyTrainer()
    with pytest.raises(L.Sim3OptError) as e:
        fresh.train()
    assert e.value.code == L.ERR_STATE
    with pytest.raises(L.Sim3OptError):
        fresh.vocabulary()
    fresh.close()
    assert L.device_memory_in_use() == start
