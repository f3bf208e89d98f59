"""The batched bag-of-words place recognition on the GPU (sim3opt_place_batch, sim3opt_amd/csrc/place_batch.hip)
against tests/place_ref.py, an independent restatement of the definition in include/sim3opt.h.  PARITY UNPINNED (the
reference tree holds neither DLoopDetector nor DBoW2, no vocabulary, no descriptors and no detection results): what
is compared is the restatement and planted truth.  The cases are tests/place_cases.py's; tests/test_place_ref.py
shows on the CPU that they keep every deciding comparison 1e-9 from a tie and reach the mistakes a kernel could make.

Integer outputs are equal.  Floating-point outputs are within 1e-12 absolute: the vectors are L1-normalised, so the
absolute terms of a score sum to at most 2; with at most 2048 common words a double sum in any order is within
2048 * 2^-53 * 2 = 4.5e-13 (the one case with longer vectors has 2049: 4.6e-13)."""
import gc

import numpy as np
import pytest

import place_cases as PCS
import place_ref as PR
from sim3opt_amd import lib as L

pytestmark = pytest.mark.gpu
TOL = 1e-12


def make(case, **opts):
    b = L.PlaceBatch(**dict(case["options"], **opts))
    b.set_vocabulary(*case["voc"].arrays())
    b.set_frames(case["kp_ptr"], case["desc"])
    return b


def snapshot(b):
    ptr, w, v = b.bow()
    return dict(b.results(), pairs=b.pairs(), bow_ptr=ptr, bow_word=w, bow_value=v)


def same_bits(x, y, n=None):
    return all(x[k][:n].tobytes() == y[k][:n].tobytes() for k in x if k != "pairs" and not k.startswith("bow_"))


def case_named(name):
    return next(c for c in PCS.all_cases() if c["name"] == name)


def test_tile_sizes_are_the_ones_the_cases_straddle():
    b = L.PlaceBatch()
    d = b.dims()
    assert {k: d[k] for k in PCS.TILES} == PCS.TILES
    b.close()


@pytest.mark.parametrize("case", PCS.all_cases(), ids=lambda c: c["name"])
def test_case_against_the_restatement(case):
    R = PCS.reference(case["name"])
    n = len(case["kp_ptr"]) - 1
    b = make(case)
    n_candidates = b.solve()
    # words, through the descent code, and the winning d2 of every level of the first descriptors
    words, path = b.debug_words(case["desc"])
    assert list(words) == [w for f in R.words for w in f]
    for t in range(min(40, len(words))):
        ref = PR.word_of(case["voc"], case["desc"][t])[1]
        assert list(path[t]) == ref + [-1.0] * (case["voc"].depth - len(ref))
    # vectors
    ptr, w, v = b.bow()
    assert list(np.diff(ptr)) == [len(x) for x in R.vectors]
    assert list(w) == [k for x in R.vectors for k in sorted(x)]
    ref_v = np.array([x[k] for x in R.vectors for k in sorted(x)])
    print("largest value error:", np.abs(v - ref_v).max() if len(v) else 0.0)
    assert np.all(np.abs(v - ref_v) <= TOL)
    # per frame
    r = b.results()
    assert list(r["status"]) == R.status
    assert list(r["match"]) == R.match
    assert list(r["n_consistent"]) == R.n_consistent
    assert [tuple(x) for x in r["island"]] == R.island
    assert n_candidates == len(R.pairs) and [tuple(x) for x in b.pairs()] == R.pairs
    err = max(np.abs(r["score"] - R.score).max(), np.abs(r["ns_factor"] - R.ns_factor).max())
    # every score, the kept results and the islands of every query
    for i in range(n):
        row = b.debug_scores(i)
        err = max(err, np.abs(row - R.S[i]).max())
        assert np.all((row == 0) == (R.S[i] == 0))
        d = b.debug_islands(i)
        assert list(d["kept_j"]) == [j for j, _ in R.kept[i]]
        assert [tuple(x) for x in d["island"]] == [(g["first"], g["last"], g["best_entry"], g["n"]) for g in R.islands[i]]
        if len(d["kept_j"]):
            err = max(err, np.abs(d["kept_score"] - [s for _, s in R.kept[i]]).max())
        if len(d["island"]):
            err = max(err, np.abs(d["island_score"] - [g["score"] for g in R.islands[i]]).max())
    print("largest score error:", err)
    assert err <= TOL
    b.close()


def test_debug_words_on_supplied_descriptors():
    """The exact tie (the lower child), the descriptor whose nearest leaf is not under its nearest first-level node (a
    greedy descent must not find it), and a tie between two leaves."""
    voc = PCS.vocabularies()["trap"]
    d, expect = PCS.trap_descriptors()
    b = L.PlaceBatch()
    b.set_vocabulary(*voc.arrays())
    words, path = b.debug_words(d)  # (no frames and no solve)
    assert list(words) == expect
    assert path.tolist() == [PR.word_of(voc, x)[1] for x in d]
    assert path[0, 0] == 1.0 and path[2, 1] == 0.25
    leaves = [i for i in range(13) if not voc.children[i]]
    nearest = leaves[int(np.argmin(PR.d2(d[1], voc.centre[leaves])))]
    assert voc.word_id[nearest] != words[1]
    # an unbalanced tree: paths of one, two and three levels, -1 past the leaf
    voc = PCS.vocabularies()["unbalanced"]
    b.set_vocabulary(*voc.arrays())
    assert b.dims()["depth"] == 3 and b.dims()["n_words"] == 67
    rng = np.random.default_rng(3)
    ws = np.arange(67)
    words, path = b.debug_words(PCS.descriptors(voc, ws, rng))
    assert list(words) == list(ws)
    assert sorted(set((row >= 0).sum() for row in path)) == [1, 2, 3]
    b.close()


def test_debug_scores_are_symmetric_bit_for_bit():
    case = case_named("revisit")
    b = make(case)
    b.solve()
    n = len(case["kp_ptr"]) - 1
    S = np.stack([b.debug_scores(i) for i in range(n)])
    assert S.tobytes() == np.ascontiguousarray(S.T).tobytes()
    assert np.all(np.abs(np.diag(S) - 1.0) <= 1e-15)  # a frame against itself
    assert S[0, 15] == 0.0 and not np.signbit(S[0, 15]) and S[20, 3] == 0.0  # no common word: exactly 0
    assert S[33, 6] > 0.3
    # ... and between vectors longer than a wavefront's round and than the part kept in LDS
    case = case_named("frame_sizes")
    b.set_vocabulary(*case["voc"].arrays())
    b.set_frames(case["kp_ptr"], case["desc"])
    b.solve()
    n = len(case["kp_ptr"]) - 1
    S = np.stack([b.debug_scores(i) for i in range(n)])
    assert S.tobytes() == np.ascontiguousarray(S.T).tobytes()
    # a vector of m values against itself is the sum of its values, one after the other: every value carries the
    # rounding of its division (their sum: 2^-53 of 1) and each of the m - 1 additions at most 2^-53 of a partial sum
    # below 1.  (The 1e-15 above is for the at most 24 words of the revisit's frames.)
    m = np.diff(b.bow()[0])
    assert m.max() == PCS.TILES["score_lds"] + 1
    assert np.all(np.abs(np.diag(S) - 1.0) <= m * 2.0 ** -53)
    b.close()


def test_frames_are_independent_of_the_batch():
    """Two solves of one handle; a batch and its first 36 of 42 frames; the same frames after another sequence on the same
    handle; a pair of frames at other places of another batch: the same bits."""
    case = case_named("revisit")
    ptr, desc = case["kp_ptr"], case["desc"]
    n = len(ptr) - 1
    b = make(case)
    b.solve()
    first = snapshot(b)
    row33 = b.debug_scores(33)
    b.solve()
    again = snapshot(b)
    assert all(first[k].tobytes() == again[k].tobytes() for k in first)
    # the first 36 frames alone: every earlier frame's outcome and vector
    half = 36
    b.set_frames(ptr[:half + 1], desc[:ptr[half]])
    b.solve()
    part = snapshot(b)
    assert same_bits(part, first, half)
    assert part["bow_ptr"].tobytes() == first["bow_ptr"][:half + 1].tobytes()
    m = int(part["bow_ptr"][-1])
    assert part["bow_word"].tobytes() == first["bow_word"][:m].tobytes()
    assert part["bow_value"].tobytes() == first["bow_value"][:m].tobytes()
    assert b.debug_scores(33).tobytes() == row33[:half].tobytes()
    # another sequence and vocabulary on the handle, then the first again
    other = case_named("unbalanced_revisit")
    b.set_vocabulary(*other["voc"].arrays())
    b.set_frames(other["kp_ptr"], other["desc"])
    b.set_options(**other["options"])
    b.solve()
    b.set_options(**case["options"])
    b.set_vocabulary(*case["voc"].arrays())
    b.set_frames(ptr, desc)
    b.solve()
    back = snapshot(b)
    assert all(first[k].tobytes() == back[k].tobytes() for k in first)
    # frames 33 and 6 at other places, in the other order, among other frames
    order = [6, 40, 33, 2]
    kp = np.concatenate([[0], np.cumsum([ptr[f + 1] - ptr[f] for f in order])])
    b.set_frames(kp, np.concatenate([desc[ptr[f]:ptr[f + 1]] for f in order]))
    b.solve()
    assert b.debug_scores(0)[2] == row33[6] and b.debug_scores(2)[0] == row33[6]
    assert b.debug_scores(1)[2] == row33[40]
    b.close()


def test_refusals_change_nothing():
    case = case_named("revisit")
    voc = case["voc"]
    b = make(case)
    b.solve()
    first, dims = snapshot(b), b.dims()

    def unchanged():
        now = snapshot(b)
        return b.dims() == dims and all(now[k].tobytes() == first[k].tobytes() for k in first)

    for kw in (dict(alpha=-0.1), dict(alpha=float("nan")), dict(min_nss_factor=float("inf")), dict(use_nss=2),
               dict(accumulate=-1), dict(k=-1), dict(dislocal=0), dict(max_db_results=0), dict(max_db_results=1025),
               dict(max_intragroup_gap=0), dict(min_matches_per_group=0), dict(max_distance_between_queries=-1),
               dict(max_distance_between_groups=-1)):
        with pytest.raises(L.Sim3OptError) as e:
            b.set_options(**kw)
        assert e.value.code == L.ERR_ARG, kw
    assert b.options()["max_db_results"] == 50 and unchanged()

    def voc_with(**kw):
        a = dict(parent=voc.parent.copy(), centre=voc.centre.copy(), weight=voc.weight.copy(), word_id=voc.word_id.copy())
        for k, (idx, val) in kw.items():
            a[k][idx] = val
        return a
    leaf = int(np.flatnonzero(voc.word_id >= 0)[-1])
    inner = int(np.flatnonzero(voc.word_id < 0)[-1])
    other = int(voc.word_id[np.flatnonzero(voc.word_id >= 0)[0]])
    for kw in (dict(parent=(0, 0)), dict(parent=(5, 5)), dict(parent=(5, 9)), dict(parent=(3, -1)),
               dict(centre=((leaf, 63), np.nan)), dict(centre=((0, 0), np.inf)), dict(weight=(leaf, -1.0)),
               dict(weight=(leaf, np.nan)), dict(word_id=(leaf, -1)), dict(word_id=(inner, 3)),
               dict(word_id=(leaf, other)), dict(word_id=(leaf, 512))):
        with pytest.raises(L.Sim3OptError) as e:
            b.set_vocabulary(**voc_with(**kw))
        assert e.value.code == L.ERR_ARG, kw
    # a node with 65 children; a tree of one node
    star = np.zeros(66, dtype=np.int32)
    star[0] = -1
    ids = np.arange(-1, 65, dtype=np.int32)
    for parent, word_id in ((star, ids), (star[:1], ids[:1])):
        with pytest.raises(L.Sim3OptError) as e:
            b.set_vocabulary(parent, np.zeros((len(parent), 64), np.float32), np.ones(len(parent)), word_id)
        assert e.value.code == L.ERR_ARG
    b.set_vocabulary(star[:65], np.zeros((65, 64), np.float32), np.ones(65), ids[:65])  # 64 children are allowed
    b.set_vocabulary(*voc.arrays())
    b.solve()
    assert unchanged()
    ptr, desc = case["kp_ptr"], case["desc"]
    for bad_ptr, bad_desc in ((np.r_[1, ptr[1:]], desc), (np.r_[ptr[:3], ptr[1], ptr[4:]], desc), (ptr[:1], desc),
                              (ptr, np.where(np.arange(desc.size).reshape(desc.shape) == desc.size - 1, np.nan, desc)),
                              (np.zeros(16386, np.int32), desc)):
        with pytest.raises(L.Sim3OptError) as e:
            b.set_frames(bad_ptr, bad_desc)
        assert e.value.code == L.ERR_ARG
    L_ = L.load()  # NULL arrays, which the wrapper cannot produce
    P = lambda a, t: a.ctypes.data_as(t)
    pa, ce, we, wi = (np.ascontiguousarray(x) for x in voc.arrays())
    for null in range(4):
        a = [P(pa, L._ip), P(ce, L._fp), P(we, L._dp), P(wi, L._ip)]
        a[null] = None
        assert L_.sim3opt_place_batch_set_vocabulary(b._b, len(pa), *a) == L.ERR_ARG
    assert L_.sim3opt_place_batch_set_frames(b._b, 1, None, P(ce, L._fp)) == L.ERR_ARG
    assert L_.sim3opt_place_batch_set_frames(b._b, 1, P(pa, L._ip), None) == L.ERR_ARG
    n = L.C.c_int32(-7)
    assert L_.sim3opt_place_batch_get_pairs(b._b, 2, L.C.byref(n), P(pa, L._ip)) == L.ERR_ARG and n.value == 9
    for q in (-1, 42):
        with pytest.raises(L.Sim3OptError) as e:
            b.debug_scores(q)
        assert e.value.code == L.ERR_ARG
        with pytest.raises(L.Sim3OptError) as e:
            b.debug_islands(q)
        assert e.value.code == L.ERR_ARG
    with pytest.raises(L.Sim3OptError) as e:
        b.debug_words(np.full((1, 64), np.nan))
    assert e.value.code == L.ERR_ARG
    assert unchanged()
    b.close()
    # state errors: nothing set, a vocabulary alone, frames alone
    b = L.PlaceBatch()
    for step in (lambda: None, lambda: b.set_vocabulary(*voc.arrays())):
        step()
        with pytest.raises(L.Sim3OptError) as e:
            b.solve()
        assert e.value.code == L.ERR_STATE
        with pytest.raises(L.Sim3OptError) as e:
            b.results()
        assert e.value.code == L.ERR_STATE
    b.close()
    b = L.PlaceBatch()
    b.set_frames(ptr, desc)
    with pytest.raises(L.Sim3OptError) as e:
        b.solve()
    assert e.value.code == L.ERR_STATE
    with pytest.raises(L.Sim3OptError) as e:
        b.debug_words(desc[:2])
    assert e.value.code == L.ERR_STATE
    b.close()


def test_device_memory():
    """All of it is back after close(); repeated solves and every diagnostic keep none; a change of options.device
    releases the handle's memory, and it solves again afterwards."""
    gc.collect()
    start = L.device_memory_in_use()
    case = case_named("revisit")
    b = make(case)
    b.solve()
    held = L.device_memory_in_use()
    assert held[1] > start[1]
    first = snapshot(b)
    for _ in range(3):
        b.solve()
        assert L.device_memory_in_use() == held
    b.debug_words(case["desc"][:300])
    b.debug_scores(33)
    b.debug_islands(33)
    assert L.device_memory_in_use() == held
    b.set_options(device=0)
    assert L.device_memory_in_use() == start
    assert all(snapshot(b)[k].tobytes() == first[k].tobytes() for k in first)  # the getters hold the last results
    with pytest.raises(L.Sim3OptError) as e:
        b.debug_scores(33)
    assert e.value.code == L.ERR_STATE
    b.solve()
    assert L.device_memory_in_use() == held
    assert all(snapshot(b)[k].tobytes() == first[k].tobytes() for k in first)
    b.close()
    assert L.device_memory_in_use() == start


def test_candidates_through_matching_and_the_essential_matrix():
    """The chain the stage closes: descriptors -> pairs() -> MatchBatch.set_pairs -> EssentialBatch.  Every planted
    revisit ends with at least 12 inliers, DLoopDetector's geometric check."""
    case = PCS.chain_case()
    R = PR.detect(case["voc"], case["kp_ptr"], case["desc"])
    planted = [p for p in case["revisits"] if p[0] >= 33]
    assert set(planted) <= set(R.pairs)
    place = make(case)
    place.solve()
    pairs = place.pairs()
    assert [tuple(p) for p in pairs] == R.pairs
    match = L.MatchBatch()
    match.set_frames(case["kp_ptr"], case["kp_ptr"], case["kp"], case["desc"], case["kp"], case["obs_depth"])
    match.set_pairs(pairs)
    assert match.solve() == len(pairs)
    m = match.matches()
    ess = L.EssentialBatch()
    ess.set_problems(match.match_ptr(), m["uv0"], m["uv1"])
    ess.solve()
    inliers = ess.inliers()[1]
    print("matches:", np.diff(match.match_ptr()), "inliers:", inliers)
    for k, p in enumerate(pairs):
        if tuple(p) in planted:
            assert inliers[k] >= 12, (p, inliers[k])
    for h in (place, match, ess):
        h.close()
