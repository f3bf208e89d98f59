"""An independent restatement, in numpy and plain Python, of the batched vocabulary training as include/sim3opt.h defines
it ("batched vocabulary training"): per-node Python lists in a queue, numpy double sums, sorted(), place_ref.d2 for the
distance and place_ref.word_of for the descent the weights are counted from.  It is not a port of the kernels: there is
no permutation, no chunk and no level-wide pass in it.  `defect` names a one-line deviation; tests/test_vocab_ref.py
asserts that the cases of tests/vocab_cases.py catch each of them.  While it runs it records every comparison that
decides anything with its margin (Training.margins).  PARITY UNPINNED: only the distance and the mean's operands are
the reference's (FSurf64.cpp:23-58); the rest restates DBoW2's create from memory.  train(exact=True) takes d2, the
seeding's prefix sums and the mean from tests/rounding_ref.py, in the order the header states to the bit, for
descriptors off the lattice (tests/rounding_cases.py); the default is unchanged."""
import math

import numpy as np

import place_ref as PR
import rounding_ref as RR

DEFAULTS = dict(k=10, levels=5, max_iters=100, idf=1, seed=0)

DEFECTS = ("tie_to_higher_cluster", "exclusive_prefix", "mean_in_fp32", "empty_cluster_zeroed", "n_counts_empty_frames",
           "depth_first_numbering", "weights_by_membership", "small_node_strict", "key_without_node", "w_is_last_distance",
           "split_at_the_last_level", "one_pass_more", "unreached_leaf_weighs_log_n", "first_centre_is_member_0",
           "r_from_the_round_before")

M64 = (1 << 64) - 1


def splitmix64(x):
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw(seed, node, c, defect=None):
    if defect == "key_without_node":
        node = 0
    return splitmix64((seed + (64 * node + c + 1) * 0x9E3779B97F4A7C15) & M64)


class Training:
    """What train() returns: parent, centre, weight, word_id (the tree), assignment and descent (per descriptor: the leaf
    node by clustering and by the descent rule), n_unconverged, passes (per level), depth, seeding (node -> dict members,
    W, r), levels (per level: the nodes in order, dicts node, kind, members, iterates [(clusters, centres) after pass 0,
    1, ...]), margins [(what, relative margin)]."""


def _mean(rows, defect):
    if defect == "mean_in_fp32":
        return (rows.astype(np.float32) / np.float32(len(rows))).sum(axis=0, dtype=np.float32)  # (FP32 quotients added)
    return (np.sum(rows.astype(np.float64), axis=0) / len(rows)).astype(np.float32)


def train(kp_ptr, desc, defect=None, exact=False, **options):
    """exact=True: d2, the seeding's prefix sums with W, and the mean in the order the header states
    (tests/rounding_ref.py), so that W, r and the centres are the definition's bits on any descriptors; `defect` may
    then also be one of rounding_ref.DEFECTS.  The default sums with numpy and is exact on lattice cases only."""
    o = dict(DEFAULTS, **options)
    d2 = (lambda a, rows: RR.d2(a, rows, defect)) if exact else PR.d2
    k, L, seed = o["k"], o["levels"], o["seed"]
    kp_ptr = np.asarray(kp_ptr)
    desc = np.asarray(desc, dtype=np.float32).reshape(-1, 64)
    D = int(kp_ptr[-1])
    R = Training()
    R.margins, R.seeding, R.levels, R.n_unconverged, R.exact_ties = [], {}, [[] for _ in range(L + 2)], 0, 0
    passes = [0] * 8
    parent, centre, is_leaf = [-1], [np.zeros(64, dtype=np.float32)], [False]
    assignment = np.full(D, -1, dtype=np.int64)
    queue = [(0, list(range(D)), 0)]  # (node, members ascending, level): first in, first out is breadth first
    while queue:
        node, members, level = queue.pop(0)
        n = len(members)
        rec = dict(node=node, kind="leaf", members=members, iterates=[])
        R.levels[level].append(rec)
        children = []  # (members, centre)
        last_level = level > L if defect == "split_at_the_last_level" else level >= L
        if n <= 1 or last_level:
            pass
        elif (n < k) if defect == "small_node_strict" else (n <= k):
            rec["kind"] = "small"
            children = [([m], desc[m].copy()) for m in members]
            rec["iterates"] = [(list(range(n)), np.stack([c for _, c in children]))]
        else:
            rows = desc[members]
            first = 0 if defect == "first_centre_is_member_0" else draw(seed, node, 0, defect) % n
            chosen, w, Ws, rs = [members[first]], None, [], []
            for c in range(1, k):
                dist = d2(desc[chosen[-1]], rows)
                w = dist if (w is None or defect == "w_is_last_distance") else np.minimum(w, dist)
                prefix, W = RR.prefix(w, defect) if exact else (np.cumsum(w), float(np.sum(w)))
                if W == 0:
                    Ws.append(0.0)
                    rs.append(0.0)
                    break
                u = (draw(seed, node, c - 1 if defect == "r_from_the_round_before" else c, defect) >> 11) * 2.0 ** -53
                r = u * W
                R.margins.append(("r against a prefix boundary", float(np.abs(prefix - r).min()) / W))
                above = np.nonzero((prefix - w if defect == "exclusive_prefix" else prefix) > r)[0]
                chosen.append(members[int(above[0]) if len(above) else n - 1])
                Ws.append(W)
                rs.append(r)
            R.seeding[node] = dict(members=chosen, W=Ws, r=rs)
            if len(chosen) > 1:
                rec["kind"] = "big"
                centres = desc[chosen].copy()
                cluster = [-1] * n
                rec["iterates"].append((list(cluster), centres.copy()))
                limit = o["max_iters"] + (1 if defect == "one_pass_more" else 0)
                converged = False
                for p in range(1, limit + 1):
                    dist = np.stack([d2(centres[c], rows) for c in range(len(centres))], axis=1)  # (n, centres)
                    order = np.sort(dist, axis=1)
                    gap = order[:, 1] - order[:, 0]
                    R.margins += [("d2 against d2", float(g / s)) for g, s in zip(gap, order[:, 1]) if g > 0]
                    R.exact_ties += int((gap == 0).sum())
                    if defect == "tie_to_higher_cluster":
                        new = [int(len(centres) - 1 - np.argmin(row[::-1])) for row in dist]
                    else:
                        new = [int(np.argmin(row)) for row in dist]  # (the first of the smallest: the lower cluster)
                    passes[level] = max(passes[level], p)
                    if new == cluster:
                        converged = True
                        rec["iterates"].append((list(cluster), centres.copy()))
                        break
                    cluster = new
                    for c in range(len(centres)):
                        mine = rows[[i for i in range(n) if cluster[i] == c]]
                        if len(mine) and exact:
                            centres[c] = RR.mean(rows, cluster, c, defect)
                        elif len(mine):
                            centres[c] = _mean(mine, defect)
                        elif defect == "empty_cluster_zeroed":
                            centres[c] = 0
                    rec["iterates"].append((list(cluster), centres.copy()))
                R.n_unconverged += not converged
                for c in range(len(centres)):
                    mine = [members[i] for i in range(n) if cluster[i] == c]
                    if mine:
                        children.append((mine, centres[c].copy()))
        if not children:
            is_leaf[node] = True
            assignment[members] = node
        for mine, cen in children:
            parent.append(node)
            centre.append(cen)
            is_leaf.append(False)
            queue.append((len(parent) - 1, mine, level + 1))
    N = len(parent)
    word_id = np.full(N, -1, dtype=np.int32)
    word_id[[i for i in range(N) if is_leaf[i]]] = np.arange(sum(is_leaf))
    R.parent, R.centre, R.word_id = np.asarray(parent, dtype=np.int32), np.stack(centre), word_id
    voc = PR.Vocabulary(R.parent, R.centre, np.zeros(N), word_id)
    leaf_of_word = {int(w): i for i, w in enumerate(word_id) if w >= 0}
    R.descent = np.asarray([leaf_of_word[PR.word_of(voc, desc[t], d2=d2)[0]] for t in range(D)], dtype=np.int64)
    R.assignment, R.depth, R.passes = assignment, voc.depth, passes
    # the weights
    counted = assignment if defect == "weights_by_membership" else R.descent
    n_frames = len(kp_ptr) - 1
    with_desc = [f for f in range(n_frames) if kp_ptr[f + 1] > kp_ptr[f] or defect == "n_counts_empty_frames"]
    Ni = {}
    for f in range(n_frames):
        for i in sorted(set(int(x) for x in counted[kp_ptr[f]:kp_ptr[f + 1]])):
            Ni[i] = Ni.get(i, 0) + 1
    R.weight = np.zeros(N)
    for i in range(N):
        if not is_leaf[i]:
            continue
        if not o["idf"]:
            R.weight[i] = 1.0
        elif i in Ni:
            R.weight[i] = math.log(len(with_desc) / Ni[i])
        elif defect == "unreached_leaf_weighs_log_n":
            R.weight[i] = math.log(len(with_desc))
    if defect == "depth_first_numbering":
        renumber_depth_first(R)
    R.levels = [lv for lv in R.levels if lv]
    return R


def renumber_depth_first(R):
    """All children of a node, then each child's subtree (the order DBoW2 creates nodes in)."""
    N = len(R.parent)
    kids = [[] for _ in range(N)]
    for i in range(1, N):
        kids[R.parent[i]].append(i)
    order = [0]

    def visit(i):
        order.extend(kids[i])
        for c in kids[i]:
            visit(c)

    visit(0)
    new = {old: i for i, old in enumerate(order)}
    R.parent = np.asarray([-1 if R.parent[old] < 0 else new[int(R.parent[old])] for old in order], dtype=np.int32)
    R.centre, R.weight = R.centre[order], R.weight[order]
    leaves = R.word_id[order] >= 0
    R.word_id = np.full(N, -1, dtype=np.int32)
    R.word_id[leaves] = np.arange(int(leaves.sum()))
    R.assignment = np.asarray([new[int(x)] for x in R.assignment])
    R.descent = np.asarray([new[int(x)] for x in R.descent])


def lloyd_state(R, level, n_pass, k, n_desc):
    """What sim3opt_vocabulary_debug_lloyd returns for (level, n_pass): (first_node, cluster per descriptor, centres
    (nodes of the level, k, 64))."""
    nodes = R.levels[level]
    cluster = np.full(n_desc, -1, dtype=np.int32)
    centres = np.zeros((len(nodes), k, 64), dtype=np.float32)
    for t, rec in enumerate(nodes):
        if not rec["iterates"]:
            continue
        cl, cen = rec["iterates"][0] if rec["kind"] == "small" else rec["iterates"][min(n_pass, len(rec["iterates"]) - 1)]
        cluster[rec["members"]] = cl
        centres[t, :len(cen)] = cen
    return nodes[0]["node"], cluster, centres


def signature(R):
    """What a defect must change in at least one case."""
    return (tuple(R.parent), tuple(R.word_id), R.centre.tobytes(), tuple(round(float(x), 9) for x in R.weight),
            tuple(int(x) for x in R.assignment), R.n_unconverged)
