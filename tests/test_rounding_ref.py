"""CPU side of the bit-for-bit tests of vocabulary training and place recognition on descriptors that round
(tests/test_gpu_rounding_descriptors.py): the order-exact mode of the restatements (vocab_ref.train(exact=True),
place_ref.detect(exact=True), computing with tests/rounding_ref.py) (a) contradicts no committed lattice case, (b) agrees
with exact rational arithmetic within the bounds its operation counts give, (c) is driven by tests/rounding_cases.py
through every order the definition names, and (d) changes a compared read-out under every deviation of the arithmetic
that the lattice cases cannot see.

Not testable by the read-outs there are: the order of the mean's double sum.  It changed 0 of 640 centre coordinates
when measured on synthetic descriptors, and changes none here: the addends are FP32, so the double sum of a few thousand
of them is exact in any order (test_the_order_of_the_means_double_sum_is_below_the_fp32_rounding asserts that).  No
read-out is added for it."""
from fractions import Fraction

import numpy as np
import pytest

import place_cases as PCS
import place_ref as PR
import rounding_cases as RC
import rounding_ref as RR
import vocab_cases as VC
import vocab_ref as VR

U = 2.0 ** -53  # the unit roundoff of a double


def gamma(n):
    """Higham's gamma_n = n u / (1 - n u): the relative error of n roundings in a row"""
    return n * U / (1 - n * U)


def exact_sum(x):
    return sum((Fraction(float(v)) for v in x), Fraction(0))


# ---- (a) the exact mode contradicts no committed test -----------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in VC.all_cases()])
def test_exact_training_gives_what_the_lattice_cases_expect(name):
    """The integers and the centre bytes of today's restatement, W and r within the 1e-12 relative and the weights
    within the 1e-14 of tests/test_gpu_vocab_train.py."""
    case = next(c for c in VC.all_cases() if c["name"] == name)
    R, E = VC.reference(name), VR.train(case["kp_ptr"], case["desc"], exact=True, **case["options"])
    assert list(E.parent) == list(R.parent) and list(E.word_id) == list(R.word_id)
    assert E.centre.tobytes() == R.centre.tobytes()
    assert list(E.assignment) == list(R.assignment) and list(E.descent) == list(R.descent)
    assert (E.depth, E.n_unconverged, E.passes) == (R.depth, R.n_unconverged, R.passes)
    assert np.all(np.abs(E.weight - R.weight) <= 1e-14)
    assert sorted(E.seeding) == sorted(R.seeding)
    for node, s in R.seeding.items():
        assert E.seeding[node]["members"] == s["members"] and len(E.seeding[node]["W"]) == len(s["W"])
        for x, y in zip(E.seeding[node]["W"] + E.seeding[node]["r"], s["W"] + s["r"]):
            assert abs(x - y) <= 1e-12 * abs(y)
    for le, lr in zip(E.levels, R.levels):
        for a, b in zip(le, lr):
            assert (a["node"], a["kind"], a["members"]) == (b["node"], b["kind"], b["members"])
            assert len(a["iterates"]) == len(b["iterates"])
            for (ca, xa), (cb, xb) in zip(a["iterates"], b["iterates"]):
                assert ca == cb and xa.tobytes() == xb.tobytes()


@pytest.mark.parametrize("name", [c["name"] for c in PCS.all_cases()])
def test_exact_detection_gives_what_the_lattice_cases_expect(name):
    """The integers of today's restatement and the floats within the 1e-12 of tests/test_gpu_place_batch.py."""
    case = next(c for c in PCS.all_cases() if c["name"] == name)
    R, E = PCS.reference(name), PR.detect(case["voc"], case["kp_ptr"], case["desc"], exact=True, **case["options"])
    assert E.words == R.words and E.status == R.status and E.match == R.match
    assert E.n_consistent == R.n_consistent and E.island == R.island and E.pairs == R.pairs
    assert [sorted(v) for v in E.vectors] == [sorted(v) for v in R.vectors]
    for a, b in zip(E.vectors, R.vectors):
        assert all(abs(a[w] - b[w]) <= 1e-12 for w in a)
    assert np.abs(E.S - R.S).max(initial=0.0) <= 1e-12 and np.array_equal(E.S == 0, R.S == 0)
    assert np.abs(np.subtract(E.score, R.score)).max() <= 1e-12
    assert np.abs(np.subtract(E.ns_factor, R.ns_factor)).max() <= 1e-12
    for i in range(len(E.status)):
        assert [j for j, _ in E.kept[i]] == [j for j, _ in R.kept[i]]
        key = lambda g: (g["first"], g["last"], g["best_entry"], g["n"])
        assert [key(g) for g in E.islands[i]] == [key(g) for g in R.islands[i]]
        assert all(abs(a["score"] - b["score"]) <= 1e-12 for a, b in zip(E.islands[i], R.islands[i]))
    # the paths of the first descriptors are compared exactly today, and stay so
    for t in range(min(40, len(E.paths))):
        assert E.paths[t] == PR.word_of(case["voc"], case["desc"][t])[1]


# ---- (b) the exact primitives against exact rationals -----------------------------------------------------------------
def test_d2_against_exact_rationals():
    """The difference and the square are one FP32 rounding each: within 2^-24 relative of the exact result of their
    operands (2^-150 absolute where the square is subnormal).  The sum is 0 + 64 terms: the first addition is exact, 63
    round, all terms are non-negative, so it is within gamma_63 of the exact sum of the FP32 squares."""
    case = RC.surf_like()
    a, rows = case["desc"][7], case["desc"][100:140]
    got = RR.d2(a, rows)
    for b, g in zip(rows, got):
        d = [np.float32(x) - np.float32(y) for x, y in zip(a, b)]
        for x, y, dk in zip(a, b, d):
            true = Fraction(float(x)) - Fraction(float(y))
            assert abs(Fraction(float(dk)) - true) <= Fraction(2.0 ** -24) * abs(true)
        sq = [dk * dk for dk in d]
        for dk, s in zip(d, sq):
            true = Fraction(float(dk)) ** 2
            assert isinstance(s, np.float32) and abs(Fraction(float(s)) - true) <= Fraction(2.0 ** -24) * true + Fraction(2.0 ** -150)
        true = exact_sum(sq)
        assert abs(Fraction(float(g)) - true) <= Fraction(gamma(63)) * true
    # subnormal squares survive: 2^-140 is 2^9 of the smallest subnormal
    sub = RC.subnormal_squares()["desc"]
    assert RR.d2(sub[1], sub[3:4])[0] == 2.0 ** -140 and RR.d2(sub[1], sub[1:2])[0] == 0.0


def test_prefix_against_exact_rationals():
    """A member's prefix is its run's scan value (a tree of at most log2 256 = 8 additions above any term) plus the
    carry (at most R additions for R runs, the one that adds the carry included); the terms are non-negative, so prefix
    and W are within gamma_(8 + R) of the exact prefix sums.  W is the carry after the last run."""
    rng = np.random.default_rng(3)
    for n in (1, 2, 3, 255, 256, 257, 300, 2 * 256 + 44, N_ROOT):
        w = RR.d2(RC.surf_like()["desc"][0], RC.surf_like()["desc"][rng.permutation(N_ROOT)[:n]])
        p, W = RR.prefix(w)
        runs = -(-n // RR.RUN)
        run = Fraction(0)
        for i in range(n):
            run += Fraction(float(w[i]))
            assert abs(Fraction(float(p[i])) - run) <= Fraction(gamma(8 + runs)) * run, (n, i)
        assert abs(Fraction(W) - run) <= Fraction(gamma(8 + runs)) * run
    # the scan as the header states it, on values whose sums are exact: the plain prefix sums
    x = np.arange(1, 301, dtype=np.float64)
    assert np.array_equal(RR.scan_run(x[:256]), np.cumsum(x[:256])) and np.array_equal(RR.prefix(x)[0], np.cumsum(x))
    # ... and on three values that round: member 2 and the run's total are two associations of one sum
    y = np.array([1.0, 2.0 ** -53, 2.0 ** -53])
    p, W = RR.prefix(y)
    assert p[2] == (y[2] + y[1]) + y[0] == 1.0 + 2.0 ** -52 and W == y[2] + (y[1] + y[0]) == 1.0
    # ... so W may lie below the last prefix, or above it: then no prefix exceeds an r just below W
    z = np.array([2.0 ** -53, 2.0 ** -53, 1.0])
    p, W = RR.prefix(z)
    assert p[2] == (z[2] + z[1]) + z[0] == 1.0 and W == z[2] + (z[1] + z[0]) == 1.0 + 2.0 ** -52 and not np.any(p > 1.0)


N_ROOT = RC.N_SURF_LIKE


def test_mean_against_exact_rationals():
    """A coordinate's double sum is 0 + n terms in R runs of at most 1024: no term passes more than 1023 + R rounding
    additions, then one division and one rounding to FP32: |c - m| <= 2^-24 |m| + 2^-150 + 2 gamma_(1024 + R) sum |x| /
    n for the exact mean m."""
    case = RC.surf_like()
    rows = case["desc"]
    cluster = np.arange(len(rows)) % 3
    runs = -(-len(rows) // RR.MEAN_RUN)
    got = RR.mean(rows, cluster, 1)
    assert got.dtype == np.float32
    mine = rows[cluster == 1]
    for k in range(0, 64, 7):
        m = exact_sum(mine[:, k]) / len(mine)
        mag = exact_sum(np.abs(mine[:, k])) / len(mine)
        bound = Fraction(2.0 ** -24) * abs(m) + Fraction(2.0 ** -150) + 2 * Fraction(gamma(1024 + runs)) * mag
        assert abs(Fraction(float(got[k])) - m) <= bound
    # a cluster with no member in the middle run, and a node of one run
    cluster = np.where((np.arange(len(rows)) >= 1024) & (np.arange(len(rows)) < 2048), 0, 1)
    first, last = (RR.serial_sum(rows[lo:hi].astype(np.float64), axis=0) for lo, hi in ((0, 1024), (2048, len(rows))))
    want = ((first + last) / float(len(rows) - 1024)).astype(np.float32)
    assert RR.mean(rows, cluster, 1).tobytes() == want.tobytes()
    one = RR.mean(rows[:900], np.zeros(900, dtype=int), 0)
    assert one.tobytes() == (RR.serial_sum(rows[:900].astype(np.float64), axis=0) / 900.0).astype(np.float32).tobytes()


def test_vector_and_score_against_exact_rationals():
    """A value is one multiplication, the total m - 1 rounding additions of positive values, the quotient one division:
    within gamma_(m + 1) of count weight / sum.  A score's term is three roundings on magnitudes of at most x + y each
    (|x - y|, x + y and their difference, itself at most 2 (x + y)): 5 u (x + y); the sum of m terms adds gamma_(m - 1)
    of sum |term| <= 2 sum (x + y); the product with -0.5 is exact: |s - s_exact| <= (2.5 u + gamma_m) sum (x + y)."""
    R, T = RC.detection("surf_like"), RC.training("surf_like")
    weight = RC.vocabulary_of(T).word_weight
    for f in (0, 13, 30):
        v, words = R.vectors[f], R.words[f]
        count = {w: words.count(w) for w in set(words)}
        total = sum(count[w] * Fraction(float(weight[w])) for w in v)
        assert sorted(v) == sorted(w for w in count if weight[w] > 0)
        for w in v:
            true = count[w] * Fraction(float(weight[w])) / total
            assert abs(Fraction(v[w]) - true) <= Fraction(gamma(len(v) + 1)) * true
    pairs = [(i, j) for i in range(36) for j in range(i) if len(R.vectors[i].keys() & R.vectors[j].keys()) >= 3]
    assert len(pairs) >= 20 and (30, 6) in pairs
    for i, j in pairs[::len(pairs) // 10] + [(30, 6)]:
        a, b = R.vectors[i], R.vectors[j]
        common = sorted(a.keys() & b.keys())
        true = sum((abs(Fraction(a[w]) - Fraction(b[w])) - (Fraction(a[w]) + Fraction(b[w])) for w in common)) / -2
        mag = sum(Fraction(a[w]) + Fraction(b[w]) for w in common)
        assert abs(Fraction(float(R.S[i, j])) - true) <= (Fraction(2.5 * U) + Fraction(gamma(len(common)))) * mag
        assert R.S[i, j] == R.S[j, i] == RR.score(b, a)
    # an island score: n - 1 rounding additions of positive scores
    for i in range(len(R.status)):
        for g, (lo, hi) in ((g, (g["first"], g["last"])) for g in R.islands[i]):
            terms = [s for j, s in R.kept[i] if lo <= j <= hi]
            assert len(terms) == g["n"]
            assert abs(Fraction(g["score"]) - exact_sum(terms)) <= Fraction(gamma(max(1, g["n"] - 1))) * exact_sum(terms)


# ---- (c) what the cases reach ------------------------------------------------------------------------------------------
def test_the_cases_reach_every_order_the_definition_names():
    case, T, R = RC.surf_like(), RC.training("surf_like"), RC.detection("surf_like")
    n = len(case["desc"])
    assert n == RC.N_SURF_LIKE == int(case["kp_ptr"][-1]) and len(case["kp_ptr"]) - 1 == 36
    assert -(-n // RR.RUN) >= 3 and n % RR.RUN != 0 and -(-n // RR.MEAN_RUN) >= 3  # the root's runs, one of them partial
    assert len(T.seeding[0]["W"]) == 3 and min(T.seeding[0]["W"]) > 0
    big1 = [rec for rec in T.levels[1] if rec["kind"] == "big"]
    assert any(len(rec["members"]) > RR.RUN for rec in big1) and any(len(rec["members"]) > RR.MEAN_RUN for rec in big1)
    assert any(len(rec["members"]) % RR.RUN for rec in big1) and T.depth == 3 and T.n_unconverged == 0
    # unit norm in FP32, entries over several binades, the second pair of every four non-negative and above the first
    d = case["desc"].astype(np.float64)
    assert np.abs(np.sqrt((d * d).sum(1)) - 1).max() <= 1e-6
    cells = d.reshape(n, 16, 4)
    assert np.all(cells[:, :, 2:] >= np.abs(cells[:, :, :2]) - 1e-7)
    assert np.median(np.log2(np.abs(d).max(1) / np.median(np.abs(d), axis=1))) >= 3
    assert len(np.unique(np.frexp(d[np.abs(d) > 0])[1])) >= 12
    # place recognition: a candidate, queries stopped at step 4 and at step 5 or 6, an island of several results
    assert PR.CANDIDATE in R.status and PR.LOW_SCORES in R.status
    assert PR.NO_GROUPS in R.status or PR.NO_TEMPORAL_CONSISTENCY in R.status
    assert max(g["n"] for x in R.islands for g in x) >= 2
    assert all(R.match[i] == i - 24 for i in range(25, 36)) and all(R.status[i] == PR.CANDIDATE for i in range(25, 36))
    assert max(len(v) for v in R.vectors) >= 10 and len(set(T.weight[T.word_id >= 0])) >= 5
    # subnormal squares: W > 0, the seeding goes on, more than one centre; every d2 below the smallest normal FP32
    case, T = RC.subnormal_squares(), RC.training("subnormal_squares")
    assert len(case["desc"]) > case["options"]["k"]
    s = T.seeding[0]
    assert len(s["members"]) == 2 and 0 < s["W"][0] < 8 * 49 * 2.0 ** -140 and T.levels[0][0]["kind"] == "big"
    assert len(T.parent) > 3 and T.depth == 3
    every = np.stack([RR.d2(a, case["desc"]) for a in case["desc"]])
    assert every.max() < 2.0 ** -126 and (every > 0).sum() == 56
    flushed = VR.train(case["kp_ptr"], case["desc"] * (np.arange(64) != 5), **case["options"])  # (what W = 0 gives)
    assert len(flushed.parent) == 1 and flushed.seeding[0]["W"] == [0.0]
    voc, d, words = RC.subnormal_pair()
    assert [PR.word_of(voc, x, d2=RR.d2) for x in d] == [(0, [0.0]), (1, [0.0])]
    assert sorted(RR.d2(d[0], voc.centre[1:])) == [0.0, 2.0 ** -140]
    R = RC.detection("subnormal_squares")
    assert len({w for f in R.words for w in f}) >= 6


# ---- (d) the deviations the lattice cases cannot see -------------------------------------------------------------------
def seeding_doubles(T):
    return {node: (tuple(s["W"]), tuple(s["r"])) for node, s in T.seeding.items()}


def trained_with(defect):
    case = RC.surf_like()
    return VR.train(case["kp_ptr"], case["desc"], exact=True, defect=defect, **case["options"])


def detected_with(defect):
    """On the reference's tree: the read-outs of place recognition alone."""
    case = RC.surf_like()
    voc = RC.vocabulary_of(RC.training("surf_like"))
    return PR.detect(voc, case["kp_ptr"], case["desc"], exact=True, defect=defect, **case["place_options"])


def bow_values(R):
    return [v[w] for v in R.vectors for w in sorted(v)]


def island_scores(R):
    return [g["score"] for x in R.islands for g in x]


@pytest.mark.parametrize("defect", RR.DEFECTS)
def test_the_cases_show_each_deviation_of_the_arithmetic(defect):
    """Each deviation changes, on surf_like, a read-out that tests/test_gpu_rounding_descriptors.py compares bit for
    bit; the read-out is named here."""
    T, R = RC.training("surf_like"), RC.detection("surf_like")
    assert defect in RR.DEFECTS and defect not in VR.DEFECTS + PR.DEFECTS
    if defect.startswith("d2_"):
        D = detected_with(defect)
        n_path = sum(a != b for p, q in zip(D.paths, R.paths) for a, b in zip(p, q))
        root_W = (trained_with(defect).seeding[0]["W"][0], T.seeding[0]["W"][0])  # (round 1 of the root: the same members)
        print(defect, "path_d2 values changed:", n_path, "of", sum(len(p) for p in R.paths), "W of the root:", root_W)
        if defect == "d2_in_four_partial_sums":
            assert n_path >= 1 or root_W[0] != root_W[1]   # path_d2 (PlaceBatch.debug_words) or W (debug_seeding)
        else:
            assert n_path >= 1000 and root_W[0] != root_W[1]  # path_d2 and W
    elif defect == "serial_prefix":
        assert seeding_doubles(trained_with(defect))[0] != seeding_doubles(T)[0]  # W or r of debug_seeding, at the root
    elif defect == "mean_of_fp32_quotients":
        E = trained_with(defect)
        a, b = E.levels[0][0]["iterates"][1][1], T.levels[0][0]["iterates"][1][1]  # debug_lloyd's centres after pass 1
        assert E.levels[0][0]["iterates"][1][0] == T.levels[0][0]["iterates"][1][0]
        print(defect, "centre coordinates changed after the root's pass 1:", int((a != b).sum()), "of", a.size)
        assert (a != b).sum() >= a.size // 2
    elif defect in ("weight_added_count_times", "l1_total_fused"):
        D = detected_with(defect)
        assert D.words == R.words
        n = sum(a != b for a, b in zip(bow_values(D), bow_values(R)))
        print(defect, "bow_value entries changed:", n, "of", len(bow_values(R)))
        assert n >= 1  # bow_value of PlaceBatch.bow()
    elif defect in ("term_left_to_right", "terms_in_descending_word_id"):
        D = detected_with(defect)
        assert bow_values(D) == bow_values(R)
        print(defect, "scores changed:", int((D.S != R.S).sum()), "of", int((R.S != 0).sum()))
        assert (D.S != R.S).sum() >= 1  # the rows of PlaceBatch.debug_scores
    else:
        assert defect == "island_score_in_descending_j"
        D = detected_with(defect)
        assert np.array_equal(D.S, R.S)
        n = sum(a != b for a, b in zip(island_scores(D), island_scores(R)))
        print(defect, "island scores changed:", n, "of", len(island_scores(R)))
        assert n >= 1  # island_score of PlaceBatch.debug_islands


def test_the_order_of_the_means_double_sum_is_below_the_fp32_rounding():
    """Why no read-out shows the order of the mean's double sum: the addends are FP32, 24 bits each, so a double sum of
    a few thousand of them within some 25 binades is exact, in any order.  Asserted here for the root's clusters after
    pass 1 (every sum equals the exact rational one); one serial sum over the whole cluster instead of runs of 1024
    then changes no centre, and the counts are printed."""
    T, rows = RC.training("surf_like"), RC.surf_like()["desc"]
    cluster = np.asarray(T.levels[0][0]["iterates"][1][0])
    changed_double = changed_fp32 = 0
    for c in range(4):
        for k in range(0, 64, 5):
            total = RR.serial_sum(rows[cluster == c][:, k].astype(np.float64))
            assert Fraction(float(total)) == exact_sum(rows[cluster == c][:, k])
        n = float((cluster == c).sum())
        whole = RR.serial_sum(rows[cluster == c].astype(np.float64), axis=0)
        runs = np.zeros(64)
        for lo in range(0, len(rows), RR.MEAN_RUN):
            runs = runs + RR.serial_sum(rows[lo:lo + RR.MEAN_RUN][cluster[lo:lo + RR.MEAN_RUN] == c].astype(np.float64), axis=0)
        assert (runs / n).astype(np.float32).tobytes() == RR.mean(rows, cluster, c).tobytes()
        changed_double += int((whole != runs).sum())
        changed_fp32 += int(((whole / n).astype(np.float32) != (runs / n).astype(np.float32)).sum())
    print("double sums changed:", changed_double, "of 256; FP32 centre coordinates changed:", changed_fp32, "of 256")
    assert changed_fp32 == 0
