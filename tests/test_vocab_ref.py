"""CPU side of the batched vocabulary training (sim3opt_vocabulary, include/sim3opt.h): the restatement's own checks on
the cases the GPU tests compare against.  Every deciding comparison keeps a relative margin of 1e-9 or is equal by
construction (the cases are quantised: an equal d2 is exactly equal), the trees pass place recognition's own
validation, the cases catch fifteen one-line defects of the restatement, every case reaches the path it was made for,
and on planted Gaussian groups every leaf holds one group.  PARITY UNPINNED: the restatement follows
include/sim3opt.h, not DBoW2's source, which the reference tree does not hold."""
import numpy as np
import pytest

import place_ref as PR
import vocab_cases as VC
import vocab_ref as VR

NAMES = [c["name"] for c in VC.all_cases()]


def case_of(name):
    return next(c for c in VC.all_cases() if c["name"] == name)


@pytest.mark.parametrize("name", NAMES)
def test_margins_and_tree(name):
    case, R = case_of(name), VC.reference(name)
    worst = min((m for _, m in R.margins), default=1.0)
    assert worst >= 1e-9, min(R.margins, key=lambda m: m[1])
    # the tree is one place recognition accepts: its own validation, breadth-first numbering, words in node order
    voc = PR.Vocabulary(R.parent, R.centre, R.weight, R.word_id)
    assert R.parent[0] == -1 and all(0 <= R.parent[i] < i for i in range(1, len(R.parent)))
    assert list(R.parent[1:]) == sorted(R.parent[1:]) and not R.centre[0].any()
    leaves = [i for i in range(len(R.parent)) if not voc.children[i]]
    assert [int(R.word_id[i]) for i in leaves] == list(range(len(leaves))) and len(leaves) >= 2
    assert all(len(ch) <= case["options"]["k"] for ch in voc.children) and voc.depth <= case["options"]["levels"]
    assert np.isfinite(R.weight).all() and (R.weight >= 0).all()
    assert set(R.assignment) <= set(leaves) and set(R.descent) <= set(leaves)
    if case["converged"]:
        assert R.n_unconverged == 0 and np.array_equal(R.assignment, R.descent)
    # every coordinate is a multiple of 2^-8 in [-1, 1]
    q = case["desc"].astype(np.float64) * 256
    assert np.array_equal(q, np.round(q)) and np.abs(case["desc"]).max() <= 1


def sizes(R, level):
    return sorted(len(rec["members"]) for rec in R.levels[level])


def test_every_case_reaches_its_path():
    R = VC.reference("n_around_k")
    assert sizes(R, 1) == [3, 4, 5, 9] and [rec["kind"] for rec in sorted(R.levels[1], key=lambda r: len(r["members"]))] \
        == ["small", "small", "big", "big"]
    T = VC.TILES
    assert sizes(VC.reference("tile_sizes"), 1) == sorted(t + m for t in T.values() for m in (-1, 0, 1))
    assert all(rec["kind"] == "big" for rec in VC.reference("tile_sizes").levels[1])
    R = VC.reference("duplicates_unbalanced")
    assert sizes(R, 1) == [1, 3, 12, 12, 25, 30]
    kinds = {len(rec["members"]): rec["kind"] for rec in R.levels[1] if len(rec["members"]) in (1, 3)}
    assert kinds == {1: "leaf", 3: "small"}
    ended = [v for v in R.seeding.values() if v["W"][-1] == 0]
    assert sorted(len(v["members"]) for v in ended) == [1, 2]           # all equal: a leaf; two values: two children
    assert R.depth == 3 and sum(rec["kind"] == "leaf" for rec in R.levels[1]) == 2  # leaves at level 1 beside subtrees
    voc = PR.Vocabulary(R.parent, R.centre, R.weight, R.word_id)
    leaves = [i for i in range(len(R.parent)) if not voc.children[i]]
    unreached = [i for i in leaves if i not in set(R.descent)]          # the later copies among children of one centre
    assert len(unreached) >= 2 and all(R.weight[i] == 0 for i in unreached)
    n_with = 4
    every = [i for i in leaves if all(i in R.descent[a:b] for a, b in zip(case_of("duplicates_unbalanced")["kp_ptr"][:-1],
                                                                         case_of("duplicates_unbalanced")["kp_ptr"][1:]) if b > a)]
    assert every and all(R.weight[i] == 0 for i in every) and n_with == 4
    assert set(VC.reference("duplicates_idf0").weight[leaves]) == {1.0}
    R = VC.reference("empty_cluster")
    its = R.levels[0][0]["iterates"]
    assert len(set(its[1][0])) == 3 and any(len(set(cl)) < 3 for cl, _ in its[2:])
    assert VC.reference("exact_tie").exact_ties > 0
    R = VC.reference("capped")
    assert R.n_unconverged > 0 and R.passes[0] == 2 and not np.array_equal(R.assignment, R.descent)
    assert VC.reference("k2_L1").depth == 1 and VC.reference("k2_L3").depth == 3 and VC.reference("k10_L3").depth >= 2
    assert len(VC.reference("k64_L2").seeding[0]["members"]) == 64


@pytest.mark.parametrize("defect", VR.DEFECTS)
def test_the_cases_catch_each_defect(defect):
    caught = []
    for case in VC.all_cases():
        if len(case["desc"]) > 1000:
            continue  # (the large case adds no path of the restatement)
        R = VR.train(case["kp_ptr"], case["desc"], defect=defect, **case["options"])
        if VR.signature(R) != VR.signature(VC.reference(case["name"])):
            caught.append(case["name"])
    assert caught, defect
    if defect == "weights_by_membership":
        assert "capped" in caught


def test_planted_groups_end_in_one_leaf_each():
    case, label = VC.planted()
    R = VR.train(case["kp_ptr"], case["desc"], **case["options"])
    assert R.n_unconverged == 0 and VC.one_group_per_leaf(R.assignment, label)
    assert int((R.word_id >= 0).sum()) == 16 and R.depth == 2
    assert min(m for _, m in R.margins) >= 1e-9
