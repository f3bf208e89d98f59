"""The device-resident frame store (sim3opt_frames, sim3opt_amd/csrc/frames.hip): the ordered compaction as an operator
against a numpy boolean mask; SurfBatch.solve_into against a plain solve(); every consumer fed by set_frames_from
against the same handle type fed by set_frames; the snapshot's lifetime; the accounting of device memory; the chain on
poisoned memory.  Everything is compared byte for byte: the store moves data and computes none."""
import functools
import gc

import numpy as np
import pytest

import match_cases as MC
import place_cases as PCS
import surf_cases as SC
import vocab_cases as VC
from sim3opt_amd import lib as L

pytestmark = pytest.mark.gpu
SURF_SMALL = ("size", "angle", "response", "octave", "laplacian")


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_dict(x, y):
    return sorted(x) == sorted(y) and all(same(x[k], y[k]) for k in x)


@pytest.fixture
def accounted():
    """device memory in use is back where it started once the test's handles are gone"""
    gc.collect()
    start = L.device_memory_in_use()
    yield start
    gc.collect()
    assert L.device_memory_in_use() == start


def refused(code, call, *words):
    """`call` raises the library's error `code`, its message holds `words`, and no device memory moved"""
    before = L.device_memory_in_use()
    with pytest.raises(L.Sim3OptError) as e:
        call()
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)
    assert L.device_memory_in_use() == before


# ---- the compaction as an operator -----------------------------------------------------------------------------------
def slots(lengths, rng, all_kept=(), none_kept=()):
    cand_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    n = int(cand_ptr[-1])
    state = rng.choice(np.array([0, 2, 3], dtype=np.int32), size=n)
    for i in all_kept:
        state[cand_ptr[i]:cand_ptr[i + 1]] = 2
    for i in none_kept:
        state[cand_ptr[i]:cand_ptr[i + 1]] = rng.choice(np.array([0, 3], dtype=np.int32), size=lengths[i])
    kp = rng.uniform(0, 1000, (n, 2)).astype(np.float32)
    desc = rng.standard_normal((n, 64)).astype(np.float32)
    return cand_ptr, state, kp, desc


def masked(cand_ptr, state, kp, desc):
    keep = state == 2
    counts = [int(keep[cand_ptr[i]:cand_ptr[i + 1]].sum()) for i in range(len(cand_ptr) - 1)]
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), kp[keep], desc[keep]


def test_compaction_against_a_boolean_mask(accounted):
    s = L.FrameStore()
    d = s.dims()
    T = d["compact_tile"]
    assert (T, d["row_lanes"]) == (256, 16) and (d["n_frames"], d["total_keypoints"], d["device"]) == (0, 0, -1)
    # an empty first and last image; lengths on both sides of one tile and past two; all kept; none kept
    lengths = [0, 1, T - 1, T, T + 1, 2 * T + 1, T + 3, 2 * T - 5, 0]
    assert {T - 1, T, T + 1} <= set(lengths) and max(lengths) > 2 * T and lengths[0] == lengths[-1] == 0
    a = slots(lengths, np.random.default_rng(5), all_kept=(6,), none_kept=(7,))
    assert set(np.unique(a[1])) == {0, 2, 3}
    s.debug_compact(*a)
    ptr, kp, desc = s.get()
    want = masked(*a)
    assert np.diff(want[0])[6] == T + 3 and np.diff(want[0])[7] == 0 and 0 < np.diff(want[0])[5] < 2 * T + 1
    assert same(ptr, want[0]) and same(kp, want[1]) and same(desc, want[2])
    assert same(s.kp_ptr(), want[0])
    d = s.dims()
    assert (d["n_frames"], d["total_keypoints"], d["desc_bytes"]) == (len(lengths), len(want[1]), 256 * len(want[1]))
    # a single image of no slots; then a refill of one kept slot
    s.debug_compact(np.zeros(2, np.int32), np.zeros(0, np.int32), np.zeros((0, 2), np.float32), np.zeros((0, 64), np.float32))
    ptr, kp, desc = s.get()
    assert list(ptr) == [0, 0] and kp.shape == (0, 2) and desc.shape == (0, 64)
    b = slots([1], np.random.default_rng(6), all_kept=(0,))
    s.debug_compact(*b)
    assert all(same(x, y) for x, y in zip(s.get(), masked(*b)))
    # what the operator refuses changes nothing
    refused(L.ERR_ARG, lambda: s.debug_compact(a[0], np.where(a[1] == 3, 4, a[1]), a[2], a[3]), "no such state")
    refused(L.ERR_ARG, lambda: s.debug_compact(a[0][::-1].copy(), a[1], a[2], a[3]), "cand_ptr")
    assert all(same(x, y) for x, y in zip(s.get(), masked(*b)))
    s.close()


def test_set_and_get_and_their_refusals(accounted):
    c = MC.frame_arrays(MC.boundaries()["frames"])
    s = L.FrameStore()
    refused(L.ERR_STATE, s.get, "not filled")
    s.set(c["kp_ptr"], c["kp"], c["desc"])
    ptr, kp, desc = s.get()
    assert same(ptr, c["kp_ptr"]) and same(kp, c["kp"]) and same(desc, c["desc"])
    bad = c["desc"].copy()
    bad[3, 5] = np.inf
    refused(L.ERR_ARG, lambda: s.set(c["kp_ptr"], c["kp"], bad), "a non-finite descriptor")
    refused(L.ERR_ARG, lambda: s.set(c["kp_ptr"][::-1].copy(), c["kp"], c["desc"]), "kp_ptr")
    lib = L.load()
    one = np.zeros(2, np.int32)
    assert lib.sim3opt_frames_set(s._b, 0, L._p(one, L._ip), L._p(c["kp"], L._fp), L._p(c["desc"], L._fp)) == L.ERR_ARG
    assert lib.sim3opt_frames_set(s._b, 1, L._p(one, L._ip), None, L._p(c["desc"], L._fp)) == L.ERR_ARG
    # a total over the int32 offsets of the descriptor floats (the arrays are not reached)
    big = np.array([0, 2 ** 31 // 64 + 1], dtype=np.int32)
    assert lib.sim3opt_frames_set(s._b, 1, L._p(big, L._ip), L._p(c["kp"], L._fp), L._p(c["desc"], L._fp)) == L.ERR_ARG
    assert b"too many keypoints" in lib.sim3opt_frames_last_error(s._b)
    assert same(s.get()[2], c["desc"])
    s.close()


# ---- the extractor fills the store -----------------------------------------------------------------------------------
def capped_batch():
    """slots of state 0 behind max_keypoints: the large textured image between two others of its size"""
    return np.stack([SC.image("textured_large"), SC.image("mixed_blobs"), SC.image("textured_large")])


SURF_BATCHES = dict(mixed=(SC.mixed_batch, {}), capped=(capped_batch, dict(max_keypoints=50)),
                    constant=(lambda: np.stack([SC.image("mixed_constant")] * 3), {}))


@functools.lru_cache(maxsize=None)
def plain_solve(name):
    """solve() of a batch with the default images_per_pass: once, shared; do not modify"""
    make, opts = SURF_BATCHES[name]
    b = L.SurfBatch(**opts)
    b.set_images(make())
    n_ok = b.solve()
    out = dict(n_ok=n_ok, kp_ptr=b.kp_ptr(), keypoints=b.keypoints(), summary=b.summary())
    b.close()
    return out


@pytest.mark.parametrize("per_pass", [1, 3, 64])
@pytest.mark.parametrize("name", list(SURF_BATCHES))
def test_solve_into_against_a_plain_solve(name, per_pass, accounted):
    ref = plain_solve(name)
    make, opts = SURF_BATCHES[name]
    if name == "mixed":
        n = ref["summary"]["n_candidates"]
        assert len(n) == 7 and n.max() > 2 * 256 and (np.diff(ref["kp_ptr"]) == 0).sum() == 3
        assert ref["kp_ptr"][-1] < n.sum()  # (holes of state 0: candidates the interpolation did not keep)
    if name == "capped":
        assert list(np.diff(ref["kp_ptr"]))[::2] == [50, 50] and ref["summary"]["n_interpolated"][0] > 50
    if name == "constant":
        assert list(ref["kp_ptr"]) == [0, 0, 0, 0]
    b, s = L.SurfBatch(images_per_pass=per_pass, **opts), L.FrameStore()
    b.set_images(make())
    assert b.solve_into(s) == ref["n_ok"]
    ptr, kp, desc = s.get()
    assert same(ptr, ref["kp_ptr"]) and same(kp, ref["keypoints"]["kp"]) and same(desc, ref["keypoints"]["desc"])
    assert s.dims()["n_frames"] == len(ptr) - 1 and s.dims()["total_keypoints"] == ptr[-1]
    # the handle's own results: everything but the descriptors
    assert same(b.kp_ptr(), ref["kp_ptr"]) and same_dict(b.summary(), ref["summary"])
    small = b.keypoints(desc=False)
    assert sorted(small) == sorted(("kp",) + SURF_SMALL)
    assert all(same(small[k], ref["keypoints"][k]) for k in small)
    refused(L.ERR_STATE, b.keypoints, "sim3opt_frames_get")
    # a plain solve afterwards gives the descriptors back to the handle; the store keeps what it has
    assert b.solve() == ref["n_ok"] and same_dict(b.keypoints(), ref["keypoints"])
    assert same(s.get()[2], ref["keypoints"]["desc"])
    b.close()
    s.close()


def test_solve_into_refusals(accounted):
    b = L.SurfBatch()
    b.set_images(SC.image("blobs"))
    refused(L.ERR_ARG, lambda: b.solve_into(None), "NULL store")
    s = L.FrameStore(device=1)  # (the ordinal is only compared: the extractor runs on device 0)
    b.set_options(device=0)
    refused(L.ERR_ARG, lambda: b.solve_into(s), "device")
    assert s.dims()["n_frames"] == 0
    b.close()
    s.close()


# ---- the consumers read the store ------------------------------------------------------------------------------------
def store_of(kp_ptr, desc, kp=None):
    s = L.FrameStore()
    s.set(kp_ptr, np.zeros((len(desc), 2), np.float32) if kp is None else kp, desc)
    return s


def vocabulary_record(t):
    return dict(zip(("parent", "centre", "weight", "word_id"), t.vocabulary()),
                **dict(zip(("assignment", "descent"), t.assignment(descent=True))),
                **{k: np.asarray(v) for k, v in t.dims().items()})


@pytest.mark.parametrize("name", ["n_around_k", "k2_L1", "exact_tie"])
def test_vocabulary_trainer_from_a_store(name, accounted):
    case = next(c for c in VC.all_cases() if c["name"] == name)
    a = L.VocabularyTrainer(**case["options"])
    a.set_frames(case["kp_ptr"], case["desc"])
    n = a.train()
    want, seeding = vocabulary_record(a), a.debug_seeding(0)
    a.close()
    s = store_of(case["kp_ptr"], case["desc"])
    t = L.VocabularyTrainer(**case["options"])
    t.set_frames_from(s)
    s.close()  # (the trainer keeps the snapshot)
    assert t.train() == n and same_dict(vocabulary_record(t), want)
    assert same_dict(t.debug_seeding(0), seeding)
    t.close()


def place_record(b):
    ptr, w, v = b.bow()
    return dict(b.results(), pairs=b.pairs(), bow_ptr=ptr, bow_word=w, bow_value=v)


def smallest_place_cases(k=2):
    return sorted((c for c in PCS.all_cases() if c["kp_ptr"][-1] > 0), key=lambda c: int(c["kp_ptr"][-1]))[:k]


@pytest.mark.parametrize("case", smallest_place_cases(), ids=lambda c: c["name"])
def test_place_batch_from_a_store(case, accounted):
    a = L.PlaceBatch(**case["options"])
    a.set_vocabulary(*case["voc"].arrays())
    a.set_frames(case["kp_ptr"], case["desc"])
    n = a.solve()
    want, row = place_record(a), a.debug_scores(len(case["kp_ptr"]) - 2)
    a.close()
    s = store_of(case["kp_ptr"], case["desc"])
    b = L.PlaceBatch(**case["options"])
    b.set_vocabulary(*case["voc"].arrays())
    b.set_frames_from(s)
    assert b.solve() == n and same_dict(place_record(b), want)
    assert same(b.debug_scores(len(case["kp_ptr"]) - 2), row)
    assert b.dims()["n_frames"] == len(case["kp_ptr"]) - 1 and b.dims()["total_descriptors"] == case["kp_ptr"][-1]
    b.close()
    s.close()


def match_record(b):
    return dict(match_ptr=b.match_ptr(), **b.matches(), **b.summary())


@pytest.mark.parametrize("case_fn", [MC.boundaries, MC.ratio], ids=lambda f: f.__name__)
def test_match_batch_from_a_store(case_fn, accounted):
    case = case_fn()
    arr = MC.frame_arrays(case["frames"])
    a = L.MatchBatch(**case["options"])
    a.set_frames(**arr, **case["intr"])
    a.set_pairs(case["pairs"])
    n = a.solve()
    want, nn = match_record(a), a.debug_nn(0)
    assert want["match_ptr"][-1] > 0
    a.close()
    s = store_of(arr["kp_ptr"], arr["desc"], arr["kp"])
    b = L.MatchBatch(**case["options"])
    b.set_frames_from(s, arr["obs_ptr"], arr["obs_uv"], arr["obs_depth"], **case["intr"])
    b.set_pairs(case["pairs"])
    assert b.solve() == n and same_dict(match_record(b), want) and same_dict(b.debug_nn(0), nn)
    d = b.dims()
    assert (d["n_frames"], d["total_keypoints"]) == (len(case["frames"]), arr["kp_ptr"][-1])
    # obs_ptr of another frame count; a bad intrinsic: refused, the handle as it was
    refused(L.ERR_ARG, lambda: b.set_frames_from(s, arr["obs_ptr"][:-1], arr["obs_uv"], arr["obs_depth"], **case["intr"]),
            "frames")
    refused(L.ERR_ARG, lambda: b.set_frames_from(s, arr["obs_ptr"], arr["obs_uv"], arr["obs_depth"],
                                                 **dict(case["intr"], focal=0.0)), "focal")
    assert b.solve() == n and same_dict(match_record(b), want)
    b.close()
    s.close()


def test_consumer_refusals(accounted):
    case = next(c for c in VC.all_cases() if c["name"] == "n_around_k")
    empty, filled = L.FrameStore(), store_of(case["kp_ptr"], case["desc"])
    t, p, m = L.VocabularyTrainer(), L.PlaceBatch(), L.MatchBatch()
    obs = (np.zeros(len(case["kp_ptr"]), np.int32), np.zeros((0, 2), np.float32), np.zeros(0, np.float32))
    for call in (lambda s: t.set_frames_from(s), lambda s: p.set_frames_from(s), lambda s: m.set_frames_from(s, *obs)):
        refused(L.ERR_ARG, lambda: call(None), "NULL store")
        refused(L.ERR_STATE, lambda: call(empty), "not filled")
    # the trainer asks for two distinct descriptors, as its set_frames does
    same_rows = store_of(np.array([0, 3], np.int32), np.ones((3, 64), np.float32))
    refused(L.ERR_ARG, lambda: t.set_frames_from(same_rows), "fewer than two distinct descriptors")
    refused(L.ERR_STATE, t.train, "no frames set")
    # a handle on another device than the snapshot's; another device while a snapshot is held
    other = filled.dims()["device"] + 1
    for h in (L.VocabularyTrainer(device=other), L.PlaceBatch(device=other)):
        refused(L.ERR_ARG, lambda: h.set_frames_from(filled), "device")
        h.close()
    t.set_frames_from(filled)
    refused(L.ERR_ARG, lambda: t.set_options(device=other), "snapshot")
    for h in (t, p, m, empty, filled, same_rows):
        h.close()


# ---- one store, the whole chain --------------------------------------------------------------------------------------
def chain_observations(n_frames):
    rng = np.random.default_rng(31)
    counts = rng.integers(20, 60, n_frames)
    obs_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    uv = rng.uniform([0, 0], [SC.MIXED_W, SC.MIXED_H], (obs_ptr[-1], 2)).astype(np.float32)
    return obs_ptr, uv, rng.uniform(5, 50, obs_ptr[-1]).astype(np.float32)


CHAIN_INTR = dict(focal=300.0, cx=160.0, cy=120.0, image_width=SC.MIXED_W, image_height=SC.MIXED_H)
CHAIN_VOC = dict(k=4, levels=2, seed=3)
CHAIN_PAIRS = [(0, 6), (6, 0), (1, 1), (0, 2), (5, 3)]  # (whatever place recognition finds, these are matched too)


def chain(from_store, on_live=None):
    """images -> SURF -> vocabulary -> places -> matches; with from_store through one FrameStore, else through host
    arrays and set_frames.  The record of every stage's results."""
    surf = L.SurfBatch(images_per_pass=3)
    surf.set_images(SC.mixed_batch())
    voc, place, match = L.VocabularyTrainer(**CHAIN_VOC), L.PlaceBatch(), L.MatchBatch()
    obs = chain_observations(7)
    if from_store:
        store = L.FrameStore()
        rec = [("extract", surf.solve_into(store)), ("kp_ptr", surf.kp_ptr()), ("frames", store.get())]
        voc.set_frames_from(store)
        place.set_frames_from(store)
        match.set_frames_from(store, *obs, **CHAIN_INTR)
    else:
        store = None
        rec = [("extract", surf.solve()), ("kp_ptr", surf.kp_ptr())]
        kp = surf.keypoints()
        rec.append(("frames", (surf.kp_ptr(), kp["kp"], kp["desc"])))
        voc.set_frames(surf.kp_ptr(), kp["desc"])
        place.set_frames(surf.kp_ptr(), kp["desc"])
        match.set_frames(surf.kp_ptr(), obs[0], kp["kp"], kp["desc"], obs[1], obs[2], **CHAIN_INTR)
    rec += [("train", voc.train()), ("vocabulary", voc.vocabulary())]
    place.set_vocabulary(*voc.vocabulary())
    rec += [("detect", place.solve()), ("places", place_record(place))]
    match.set_pairs(np.concatenate([place.pairs().reshape(-1, 2), np.array(CHAIN_PAIRS, np.int32)]))
    rec += [("match", match.solve()), ("matches", match_record(match))]
    if on_live:
        on_live(store, voc, place, match)
    for h in (surf, voc, place, match) + ((store,) if store else ()):
        h.close()
    return rec


def test_the_chain_from_one_store_equals_the_host_array_chain(accounted):
    from test_gpu_stale_memory import first_difference
    a, b = chain(False), chain(True)
    assert first_difference(a, b) is None, first_difference(a, b)
    assert dict(b)["matches"]["match_ptr"][-1] > 0 and dict(b)["frames"][0][-1] > 500


def test_one_copy_of_the_descriptors_not_three(accounted):
    start = accounted
    seen = {}

    def on_live(store, voc, place, match):
        seen["bytes"] = L.device_memory_in_use()[1] - start[1]
        seen["desc"] = store.dims()["desc_bytes"] if store else None

    chain(False, on_live)
    host_leg = dict(seen)
    chain(True, on_live)
    n_desc = seen["desc"]
    assert n_desc == 256 * plain_solve("mixed")["kp_ptr"][-1] > 100000
    print(f"[frames] live bytes with three consumers: host-array leg {host_leg['bytes']}, store leg {seen['bytes']}, "
          f"descriptors {n_desc}")
    # the host-array leg holds the descriptors three times and the store leg once; rounding of a block is at most 12.5 %
    assert host_leg["bytes"] - seen["bytes"] >= 2 * n_desc
    # and per consumer: what set_frames_from plus the first solve allocates excludes a descriptor-sized block
    case = next(c for c in VC.all_cases() if c["name"] == "k10_L3")
    N = int(case["kp_ptr"][-1])
    deltas = {}
    for how in ("set_frames", "set_frames_from"):
        s = store_of(case["kp_ptr"], case["desc"]) if how == "set_frames_from" else None
        before = L.device_memory_in_use()[1]
        p = L.PlaceBatch()
        p.set_vocabulary(*next(c for c in PCS.all_cases() if c["kp_ptr"][-1] > 0)["voc"].arrays())
        if s:
            p.set_frames_from(s)
            assert L.device_memory_in_use()[1] == before  # (nothing is allocated at the hand-over)
        else:
            p.set_frames(case["kp_ptr"], case["desc"])
        p.solve()
        deltas[how] = L.device_memory_in_use()[1] - before
        p.close()
        if s:
            s.close()
    assert deltas["set_frames"] - deltas["set_frames_from"] >= 256 * N, deltas


# ---- lifetime ----------------------------------------------------------------------------------------------------------
def test_a_consumer_keeps_its_snapshot(accounted):
    c1 = MC.boundaries()
    a1 = MC.frame_arrays(c1["frames"])
    obs1 = (a1["obs_ptr"], a1["obs_uv"], a1["obs_depth"])
    ref = L.MatchBatch(**c1["options"])
    ref.set_frames(**a1, **c1["intr"])
    ref.set_pairs(c1["pairs"])
    ref.solve()
    want1 = match_record(ref)
    # the store is destroyed before the consumer's solve
    s = store_of(a1["kp_ptr"], a1["desc"], a1["kp"])
    m = L.MatchBatch(**c1["options"])
    m.set_frames_from(s, *obs1, **c1["intr"])
    m.set_pairs(c1["pairs"])
    s.close()
    m.solve()
    assert same_dict(match_record(m), want1)
    m.close()
    # the store is refilled after a consumer took it: that consumer is unchanged, a second one sees the new contents
    c2 = MC.ratio()
    a2 = MC.frame_arrays(c2["frames"])
    s = store_of(a1["kp_ptr"], a1["desc"], a1["kp"])
    m1 = L.MatchBatch(**c1["options"])
    m1.set_frames_from(s, *obs1, **c1["intr"])
    m1.set_pairs(c1["pairs"])
    s.set(a2["kp_ptr"], a2["kp"], a2["desc"])
    m2 = L.MatchBatch(**c2["options"])
    m2.set_frames_from(s, a2["obs_ptr"], a2["obs_uv"], a2["obs_depth"], **c2["intr"])
    m2.set_pairs(c2["pairs"])
    m1.solve()
    m2.solve()
    assert same_dict(match_record(m1), want1)
    ref.set_options(**c2["options"])
    ref.set_frames(**a2, **c2["intr"])
    ref.set_pairs(c2["pairs"])
    ref.solve()
    want2 = match_record(ref)
    assert same_dict(match_record(m2), want2)
    # set_frames after set_frames_from drops the snapshot, and back
    held = L.device_memory_in_use()
    m1.set_frames(**a2, **c2["intr"])
    assert L.device_memory_in_use()[0] == held[0] - 3  # (the first snapshot's three blocks: m1 was its last holder)
    m1.set_options(**c2["options"])
    m1.set_pairs(c2["pairs"])
    m1.solve()
    assert same_dict(match_record(m1), want2)
    m1.set_options(device=0, **c2["options"])  # (no snapshot held: the device may be named again)
    m1.set_frames_from(s, a2["obs_ptr"], a2["obs_uv"], a2["obs_depth"], **c2["intr"])
    m1.set_pairs(c2["pairs"])
    m1.solve()
    assert same_dict(match_record(m1), want2)
    for h in (ref, m1, m2, s):
        h.close()


# ---- poisoned memory ---------------------------------------------------------------------------------------------------
def test_the_chain_on_poisoned_memory():
    from test_gpu_stale_memory import held, three_runs
    three_runs("frame_store_chain", lambda: chain(True, lambda *handles: held()))
