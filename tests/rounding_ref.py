"""The arithmetic of vocabulary training and place recognition in the order include/sim3opt.h states it, operation by
operation, in numpy IEEE double and float32: what vocab_ref.train(exact=True) and place_ref.detect(exact=True) compute
with, so that their doubles are the definition's bits and not a value near them.  Written from the header ("batched
bag-of-words place recognition", "batched vocabulary training"), not from the kernels.

Only elementwise operations and serial sums are used: np.cumsum adds one element after the other (np.sum is pairwise
and appears nowhere), a scan is log-step shifted adds on a copy, and every scalar is a Python float, which is an IEEE
double.  Every serial sum starts from +0, as an accumulator does, so that a sum of -0 terms is +0.

`defect` names a deviation of the arithmetic alone, one a kernel could make without any committed lattice case
noticing; tests/test_rounding_ref.py asserts that tests/rounding_cases.py makes each of them visible in a read-out the
GPU test compares."""
from fractions import Fraction

import numpy as np

RUN, MEAN_RUN = 256, 1024  # the runs of the seeding's prefix sums and of the mean's double sum

DEFECTS = ("d2_in_an_fp32_accumulator", "d2_in_four_partial_sums", "d2_squares_in_double", "serial_prefix",
           "mean_of_fp32_quotients", "weight_added_count_times", "l1_total_fused", "term_left_to_right",
           "terms_in_descending_word_id", "island_score_in_descending_j")


def serial_sum(x, axis=-1, dtype=np.float64):
    """0 + x_0 + x_1 + ... along `axis`, one after the other, every addition rounded to `dtype`."""
    x = np.asarray(x, dtype=dtype)
    zero = np.zeros(x.shape[:axis % x.ndim] + (1,) + x.shape[axis % x.ndim + 1:], dtype=dtype)
    return np.take(np.cumsum(np.concatenate([zero, x], axis=axis), axis=axis, dtype=dtype), -1, axis=axis)


def d2(a, centres, defect=None):
    """d2(a, b) = sum_k (double) fl32(fl32(a_k - b_k) * fl32(a_k - b_k)) for every row b of centres: difference and
    square in FP32, each rounded once, the 64 terms added in double in ascending k."""
    a, centres = np.asarray(a, dtype=np.float32), np.asarray(centres, dtype=np.float32).reshape(-1, 64)
    d = a[None, :] - centres  # (float32 - float32: one rounding)
    if defect == "d2_squares_in_double":
        return serial_sum(d.astype(np.float64) * d.astype(np.float64))
    sq = d * d
    assert d.dtype == np.float32 and sq.dtype == np.float32
    if defect == "d2_in_an_fp32_accumulator":
        return serial_sum(sq, dtype=np.float32).astype(np.float64)
    if defect == "d2_in_four_partial_sums":
        p = [serial_sum(sq[:, j::4]) for j in range(4)]
        return (p[0] + p[1]) + (p[2] + p[3])
    return serial_sum(sq)


def scan_run(x):
    """The inclusive scan within one run: the run's values followed by zeros up to RUN entries; then, for s = 1, 2, 4,
    ..., RUN / 2, every entry i >= s becomes itself plus entry i - s, all entries from the values before the step."""
    s = np.zeros(RUN)
    s[:len(x)] = x
    step = 1
    while step < RUN:
        t = s.copy()
        t[step:] = s[step:] + s[:-step]
        s, step = t, 2 * step
    return s


def prefix(w, defect=None):
    """(the inclusive prefix sum of every member, W): runs of RUN members in member order; a member's prefix is its
    run's scan value plus the carry, the carry being 0 + the totals of the runs before, one after the other; a run's
    total is the scan's last entry (entry RUN - 1, also of a partial run); W is the carry after the last run."""
    w = np.asarray(w, dtype=np.float64)
    if defect == "serial_prefix":
        p = np.cumsum(w)
        return p, float(p[-1])
    out, carry = np.empty(len(w)), 0.0
    for lo in range(0, len(w), RUN):
        s = scan_run(w[lo:lo + RUN])
        m = min(RUN, len(w) - lo)
        out[lo:lo + m] = s[:m] + carry
        carry = carry + float(s[RUN - 1])
    return out, carry


def mean(rows, cluster, c, defect=None):
    """The centre of cluster c of a node: rows (n x 64, FP32) are the node's members in member order, cluster their
    clusters.  Per run of MEAN_RUN node members the cluster's coordinates added in double one member after the other;
    the runs' sums added one after the other; one division by the count; one rounding to FP32."""
    rows, cluster = np.asarray(rows, dtype=np.float32), np.asarray(cluster)
    count = int((cluster == c).sum())
    if defect == "mean_of_fp32_quotients":  # (FSurf64::meanValue: FP32 quotients added one after the other)
        return serial_sum(rows[cluster == c] / np.float32(count), axis=0, dtype=np.float32)
    total = np.zeros(64)
    for lo in range(0, len(rows), MEAN_RUN):
        mine = rows[lo:lo + MEAN_RUN][cluster[lo:lo + MEAN_RUN] == c]
        total = total + serial_sum(mine.astype(np.float64), axis=0)
    return (total / float(count)).astype(np.float32)


def fma(a, b, c):
    """fl(a * b + c), rounded once (through exact rationals)"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def bow_vector(word_weight, words, accumulate=1, defect=None, zero_weight_kept=False, norm_by_word_count=False):
    """The bag-of-words vector of a frame as a dict word -> value: value = count * weight, one multiplication; the L1
    total 0 + the values one after the other in ascending word id; every value divided by it."""
    count = {}
    for w in words:
        count[w] = count.get(w, 0) + 1
    v = {}
    total = 0.0
    for w in sorted(count):
        ww = float(word_weight[w])
        if not (ww > 0 or (zero_weight_kept and ww >= 0)):
            continue
        if not accumulate:
            v[w] = ww
        elif defect == "weight_added_count_times":  # (as DBoW2 does)
            v[w] = 0.0
            for _ in range(count[w]):
                v[w] += ww
        else:
            v[w] = float(count[w]) * ww
        if defect == "l1_total_fused" and accumulate:
            total = fma(float(count[w]), ww, total)
        else:
            total += v[w]
    if norm_by_word_count:
        total = float(len(v))
    return {w: x / total for w, x in v.items()} if v and total > 0 else {}


def score(a, b, defect=None, no_half=False):
    """s(a, b): the terms fabs(a_w - b_w) - (fabs(a_w) + fabs(b_w)) added to 0 one after the other in ascending common
    word id, then one multiplication by -0.5; +0 without a common word or for a sum of 0."""
    common = sorted(a.keys() & b.keys(), reverse=defect == "terms_in_descending_word_id")
    acc = 0.0
    for w in common:
        x, y = a[w], b[w]
        if defect == "term_left_to_right":
            acc += (abs(x - y) - abs(x)) - abs(y)
        else:
            acc += abs(x - y) - (abs(x) + abs(y))
    if acc == 0:
        return 0.0
    return -acc if no_half else -0.5 * acc


def island_score(scores, defect=None):
    """The scores of an island's results, given in ascending j, added one after the other starting from the first."""
    scores = list(scores)[::-1] if defect == "island_score_in_descending_j" else list(scores)
    total = scores[0]
    for s in scores[1:]:
        total += s
    return total
