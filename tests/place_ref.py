"""An independent restatement, in numpy and plain Python, of the batched bag-of-words place recognition as
include/sim3opt.h defines it ("batched bag-of-words place recognition"): the word of a descriptor, the vector of a
frame (a dict), the score (long-double sums), the per-query tests (sorted()), the temporal window.  `defect` names a
one-line deviation; tests/test_place_ref.py asserts that the cases of tests/place_cases.py catch each of them.
While it runs it records every comparison that decides anything with its margin (Detection.margins).
detect(exact=True) takes the vectors, the scores and the island scores from tests/rounding_ref.py, in the order the
header states to the bit, for descriptors off the lattice (tests/rounding_cases.py); the default is unchanged."""
import numpy as np

import rounding_ref as RR

CANDIDATE, CLOSE_MATCHES_ONLY, NO_DB_RESULTS, LOW_NSS_FACTOR, LOW_SCORES, NO_GROUPS, NO_TEMPORAL_CONSISTENCY = range(7)

DEFAULTS = dict(alpha=0.3, min_nss_factor=0.005, use_nss=1, k=3, dislocal=20, max_db_results=50,
                max_intragroup_gap=3, min_matches_per_group=1, max_distance_between_queries=2,
                max_distance_between_groups=3, accumulate=1)

DEFECTS = ("higher_child_on_tie", "zero_weight_kept", "norm_by_word_count", "no_half", "j_lt_i_minus_dislocal",
           "i_lt_dislocal", "strict_threshold", "cut_after_threshold_on_j", "gap_le", "island_score_max",
           "last_island_on_tie", "n_ge_k", "window_not_updated_on_non_fit", "query_distance_ignored")


class Vocabulary:
    def __init__(self, parent, centre, weight, word_id):
        self.parent = np.asarray(parent, dtype=np.int32)
        self.centre = np.asarray(centre, dtype=np.float32).reshape(-1, 64)
        self.weight = np.asarray(weight, dtype=np.float64)
        self.word_id = np.asarray(word_id, dtype=np.int32)
        self.children = [[] for _ in self.parent]
        for i, p in enumerate(self.parent):
            if p >= 0:
                self.children[p].append(i)  # ascending node index
        self.word_weight = np.zeros(int((self.word_id >= 0).sum()))
        for i, w in enumerate(self.word_id):
            if w >= 0:
                self.word_weight[w] = self.weight[i]
        self.depth = max(self._level(i) for i in range(len(self.parent)) if not self.children[i])

    def _level(self, i):
        n = 0
        while self.parent[i] >= 0:
            i, n = self.parent[i], n + 1
        return n

    def arrays(self):
        return self.parent, self.centre, self.weight, self.word_id


def d2(a, centres):
    """FSurf64::distance of descriptor a to each row of centres: FP32 difference and square, added in double in
    ascending k (cumsum adds one after the other)."""
    d = (a[None, :].astype(np.float32) - centres.astype(np.float32)).astype(np.float32)
    sq = (d * d).astype(np.float32)
    return np.cumsum(sq.astype(np.float64), axis=1)[:, -1]


def word_of(voc, a, defect=None, d2=d2):
    """(word id, [winning d2 of every level]); d2: the distance, this module's by default"""
    node, path = 0, []
    while voc.children[node]:
        ch = voc.children[node]
        dist = d2(np.asarray(a, dtype=np.float32), voc.centre[ch])
        best = min(range(len(ch)), key=lambda c: (dist[c], -c if defect == "higher_child_on_tie" else c))
        path.append(float(dist[best]))
        node = ch[best]
    return int(voc.word_id[node]), path


def bow_vector(voc, words, accumulate=1, defect=None):
    count = {}
    for w in words:
        count[w] = count.get(w, 0) + 1
    v = {}
    for w in sorted(count):
        ww = float(voc.word_weight[w])
        if ww > 0 or (defect == "zero_weight_kept" and ww >= 0):
            v[w] = count[w] * ww if accumulate else ww
    total = 0.0
    for w in sorted(v):
        total += v[w]
    if defect == "norm_by_word_count":
        total = float(len(v))
    return {w: x / total for w, x in v.items()} if v and total > 0 else {}


def score(a, b, defect=None):
    s = np.longdouble(0)
    for w in sorted(a.keys() & b.keys()):
        x, y = np.longdouble(a[w]), np.longdouble(b[w])
        s += abs(x - y) - abs(x) - abs(y)
    return float(-s if defect == "no_half" else -s / 2)


class Detection:
    """What detect() returns: per-frame lists status, match, score, ns_factor, n_consistent, island; the words
    (per frame), paths (per descriptor: the winning d2 of every level), vectors (dicts), S (the full score matrix),
    kept and islands per query (for the diagnostics),
    pairs, and margins: (what, margin) of every deciding comparison that is not an equality by construction."""


def detect(voc, kp_ptr, desc, defect=None, exact=False, **options):
    """exact=True: every double in the order the header states (tests/rounding_ref.py), so that the vectors, the scores
    and the island scores are the definition's bits; `defect` may then also be one of rounding_ref.DEFECTS.  The
    default sums the scores in long double and is compared within a tolerance."""
    o = dict(DEFAULTS, **options)
    kp_ptr = np.asarray(kp_ptr)
    desc = np.asarray(desc, dtype=np.float32).reshape(-1, 64)
    n = len(kp_ptr) - 1
    R = Detection()
    if exact:
        found = [word_of(voc, desc[t], defect, d2=lambda a, c: RR.d2(a, c, defect)) for t in range(kp_ptr[-1])]
    else:
        found = [word_of(voc, desc[t], defect) for t in range(kp_ptr[-1])]
    all_words, R.paths = [w for w, _ in found], [p for _, p in found]
    R.words = [all_words[kp_ptr[f]:kp_ptr[f + 1]] for f in range(n)]
    if exact:
        R.vectors = [RR.bow_vector(voc.word_weight, w, o["accumulate"], defect, defect == "zero_weight_kept",
                                   defect == "norm_by_word_count") for w in R.words]
    else:
        R.vectors = [bow_vector(voc, w, o["accumulate"], defect) for w in R.words]
    S = np.zeros((n, n))
    for i in range(n):
        for j in range(i + 1):
            if exact:
                S[i, j] = S[j, i] = RR.score(R.vectors[i], R.vectors[j], defect, defect == "no_half")
            else:
                S[i, j] = S[j, i] = score(R.vectors[i], R.vectors[j], defect)
    R.S = S
    R.margins = []
    R.status, R.match, R.score, R.ns_factor = [CANDIDATE] * n, [-1] * n, [0.0] * n, [0.0] * n
    R.n_consistent, R.island, R.island_score = [0] * n, [(-1, -1)] * n, [0.0] * n
    R.kept, R.islands = [[] for _ in range(n)], [[] for _ in range(n)]
    same = lambda a, b: R.vectors[a] == R.vectors[b]
    for i in range(n):
        if (i < o["dislocal"]) if defect == "i_lt_dislocal" else (i <= o["dislocal"]):
            R.status[i] = CLOSE_MATCHES_ONLY
            continue
        hi = i - o["dislocal"] - (1 if defect == "j_lt_i_minus_dislocal" else 0)
        found = sorted(((S[i, j], j) for j in range(0, hi + 1) if S[i, j] > 0), key=lambda r: (-r[0], r[1]))
        R.margins += [("score > 0", s) for s, _ in found]
        R.margins += [("score order", a[0] - b[0]) for a, b in zip(found, found[1:])
                      if not (a[0] == b[0] and same(a[1], b[1]))]
        res = found if defect == "cut_after_threshold_on_j" else found[:o["max_db_results"]]
        if not res:
            R.status[i] = NO_DB_RESULTS
            continue
        ns = S[i, i - 1] if o["use_nss"] else 1.0
        R.ns_factor[i] = ns
        if o["use_nss"]:
            R.margins.append(("ns against min_nss_factor", abs(ns - o["min_nss_factor"])))
            if ns < o["min_nss_factor"]:
                R.status[i] = LOW_NSS_FACTOR
                continue
        thr = o["alpha"] * ns
        R.margins += [("score against threshold", abs(s - thr)) for s, j in res
                      if not (s == thr and o["alpha"] == 1.0 and same(j, i - 1))]
        kept = [r for r in res if (r[0] > thr if defect == "strict_threshold" else r[0] >= thr)]
        if defect == "cut_after_threshold_on_j":
            kept = sorted(kept, key=lambda r: r[1])[:o["max_db_results"]]
        if not kept:
            R.status[i] = LOW_SCORES
            continue
        kept = sorted(kept, key=lambda r: r[1])
        R.kept[i] = [(j, s) for s, j in kept]
        groups, cur = [], [kept[0]]
        for r in kept[1:]:
            gap = r[1] - cur[-1][1]
            if (gap <= o["max_intragroup_gap"]) if defect == "gap_le" else (gap < o["max_intragroup_gap"]):
                cur.append(r)
            else:
                groups.append(cur)
                cur = [r]
        groups.append(cur)
        islands = []
        for g in groups:
            if len(g) < o["min_matches_per_group"]:
                continue
            total = np.longdouble(0)
            for s, _ in g:
                total += np.longdouble(s)
            if exact:
                total = RR.island_score([s for s, _ in g], defect)
            total = max(s for s, _ in g) if defect == "island_score_max" else float(total)
            best = min(g, key=lambda r: (-r[0], r[1]))
            islands.append(dict(first=g[0][1], last=g[-1][1], score=total, best_entry=best[1], best_score=best[0],
                                n=len(g), scores=sorted(s for s, _ in g)))
        R.islands[i] = islands
        if not islands:
            R.status[i] = NO_GROUPS
            R.match[i], R.score[i] = res[0][1], res[0][0]
            continue
        R.margins += [("island score", abs(a["score"] - b["score"])) for k, a in enumerate(islands)
                      for b in islands[k + 1:] if not (a["score"] == b["score"] and a["scores"] == b["scores"])]
        if defect == "last_island_on_tie":
            chosen = min(islands, key=lambda g: (-g["score"], -g["first"]))
        else:
            chosen = min(islands, key=lambda g: (-g["score"], g["first"]))
        R.match[i], R.score[i] = chosen["best_entry"], chosen["best_score"]
        R.island[i], R.island_score[i] = (chosen["first"], chosen["last"]), chosen["score"]
    # the temporal window
    a1 = a2 = last_query = cnt = 0
    for i in range(n):
        if R.status[i] != CANDIDATE:
            continue
        first, last = R.island[i]
        far = i - last_query > o["max_distance_between_queries"] and defect != "query_distance_ignored"
        fits = True
        if cnt == 0 or far:
            cnt = 1
        else:
            fits = (first <= a2 and a1 <= last) or max(a1 - last, first - a2) <= o["max_distance_between_groups"]
            cnt = cnt + 1 if fits else 1
        if fits or defect != "window_not_updated_on_non_fit":
            a1, a2, last_query = first, last, i
        R.n_consistent[i] = cnt
        if not ((cnt >= o["k"]) if defect == "n_ge_k" else (cnt > o["k"])):
            R.status[i] = NO_TEMPORAL_CONSISTENCY
    R.pairs = [(i, R.match[i]) for i in range(n) if R.status[i] == CANDIDATE]
    return R


def signature(R):
    """What a defect must change in at least one case: the integer outcome and the floats rounded well above the
    rounding of a sum."""
    return (tuple(R.status), tuple(R.match), tuple(R.n_consistent), tuple(R.island), tuple(map(tuple, R.words)),
            tuple(round(x, 9) for x in R.score), tuple(round(x, 9) for x in R.island_score),
            tuple(tuple(sorted((w, round(x, 9)) for w, x in v.items())) for v in R.vectors))
