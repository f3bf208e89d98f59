"""The restatement of the bag-of-words place recognition (tests/place_ref.py) and its cases (tests/place_cases.py),
checked without a GPU: the planted truth, the statuses the forced cases were built for, the margin every deciding
comparison keeps, and that the cases catch one-line defects of the restatement.  tests/test_gpu_place_batch.py holds
the library to the same restatement on the same cases."""
import numpy as np
import pytest

import place_cases as PCS
import place_ref as PR

MARGIN = 1e-9


def test_planted_revisit_gives_the_planted_candidates():
    R = PCS.reference("revisit")
    assert {i: s for i, s in enumerate(R.status)} == PCS.REVISIT_EXPECT
    for i, m in PCS.REVISIT_MATCH.items():
        assert R.match[i] == m, (i, R.match[i], m)
    assert R.pairs == [(i, i - 27) for i in range(33, 42)]
    thr = [m for what, m in R.margins if what == "score against threshold"]
    print("smallest distance of a score from its threshold:", min(thr))
    assert min(thr) > 0.01


def test_every_status_occurs_and_the_forced_cases_are_what_they_were_built_for():
    seen = set()
    for case in PCS.all_cases():
        R = PCS.reference(case["name"])
        seen |= set(R.status)
        for i, s in case["expect"].items():
            assert R.status[i] == s, (case["name"], i, R.status[i], s)
    assert seen == set(range(7))
    R = PCS.reference("no_groups")
    assert R.match[5] == 0 and R.score[5] == 6 / 32
    R = PCS.reference("two_islands_later_wins")
    assert [(g["first"], g["last"]) for g in R.islands[8]] == [(0, 0), (3, 4)] and R.match[8] == 4
    R = PCS.reference("island_tie")
    assert [g["score"] for g in R.islands[8]] == [4 / 32, 4 / 32] and R.match[8] == 0 and R.island[8] == (0, 0)
    R = PCS.reference("max_db_results_cuts")
    assert R.kept[8] == [(1, 5 / 32), (2, 4 / 32)] and R.S[8, 0] == 3 / 32 > 0.3 * R.ns_factor[8]
    R = PCS.reference("query_gap")
    assert [R.n_consistent[i] for i in (6, 7, 10, 11)] == [1, 2, 1, 2]
    R = PCS.reference("group_gap")
    assert [R.island[i] for i in (8, 9, 10, 11)] == [(0, 0), (3, 3), (7, 7), (1, 1)]
    assert [R.n_consistent[i] for i in (8, 9, 10, 11)] == [1, 2, 1, 1]
    R = PCS.reference("empty_and_single_frames")
    assert R.vectors[3] == {} and len(R.vectors[5]) == 1 and R.status[3] == PR.NO_DB_RESULTS
    R = PCS.reference("threshold_met_exactly")
    assert R.S[7, 0] == R.ns_factor[7] == 6 / 32 and R.kept[7] == [(0, 6 / 32)]
    R = PCS.reference("identical_database_frames")
    assert R.S[6, 0] == R.S[6, 1] == 4 / 32 and R.kept[6] == [(0, 4 / 32)]
    R = PCS.reference("revisit_no_nss")
    assert all(x in (0.0, 1.0) for x in R.ns_factor) and PR.LOW_NSS_FACTOR not in R.status


def test_trap_descriptors_descend_greedily_and_take_the_lower_child_on_a_tie():
    voc = PCS.vocabularies()["trap"]
    d, words = PCS.trap_descriptors()
    got = [PR.word_of(voc, x) for x in d]
    assert [w for w, _ in got] == words
    assert got[0][1][0] == 1.0 and list(PR.d2(d[0], voc.centre[[1, 2]])) == [1.0, 1.0]  # the exact tie
    # the nearest leaf of the second descriptor is not under its nearest first-level node
    leaves = [i for i in range(13) if not voc.children[i]]
    nearest = leaves[int(np.argmin(PR.d2(d[1], voc.centre[leaves])))]
    assert voc.parent[nearest] == 2 and voc.word_id[nearest] != words[1]
    assert list(PR.d2(d[2], voc.centre[[10, 11]])) == [0.25, 0.25]


def test_shape_cases_stand_at_the_tile_sizes():
    T = PCS.TILES
    sizes = set(np.diff(next(c for c in PCS.all_cases() if c["name"] == "frame_sizes")["kp_ptr"]))
    for t in ("wavefront", "workgroup", "bow_chunk", "score_lds"):
        assert {T[t] - 1, T[t], T[t] + 1} <= sizes
    R = PCS.reference("frame_sizes")
    assert {len(v) for v in R.vectors} >= {T["score_lds"] - 1, T["score_lds"], T["score_lds"] + 1}
    counts = {len(c["kp_ptr"]) - 1 for c in PCS.all_cases()}
    for t in ("score_frames", "workgroup"):
        assert {T[t] - 1, T[t], T[t] + 1} <= counts
    assert {len(c["voc"].parent) for c in PCS.all_cases()} >= {T["lds_nodes"] - 1, T["lds_nodes"], T["lds_nodes"] + 1}


@pytest.mark.parametrize("case", PCS.all_cases(), ids=lambda c: c["name"])
def test_every_deciding_comparison_keeps_its_margin(case):
    """Score against threshold, score against score in an order or an arg-max, island sum against island sum, ns
    against min_nss_factor: at least 1e-9 apart unless equal by construction (identical vectors)."""
    R = PCS.reference(case["name"])
    close = [(what, m) for what, m in R.margins if not m >= MARGIN]
    assert not close, close[:5]


@pytest.mark.parametrize("defect", PR.DEFECTS)
def test_the_cases_catch_a_one_line_defect(defect):
    caught = []
    for case in PCS.sequence_cases():
        D = PR.detect(case["voc"], case["kp_ptr"], case["desc"], defect=defect, **case["options"])
        if PR.signature(D) != PR.signature(PCS.reference(case["name"])):
            caught.append(case["name"])
    print(defect, "caught by", caught)
    assert caught
