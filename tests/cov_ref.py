"""Helpers of the covariance tests (test_covariance_paths.py, test_gpu_covariances.py): the elimination tree of a
marginal plan, the classes of vertex pairs the tests must cover, the graphs they share and a numpy replay of the
root-path recursion k_cov_paths / k_cov_pairs run (sim3opt_amd/csrc/cov_kernels.hpp)."""
import numpy as np

from sim3opt_amd import synth
import kitti_graph as K

CLASSES = ("on_pattern", "off_ancestor", "off_common", "different_bottom_groups", "both_top")


def two_chains():
    """Two disconnected chains (a forest: two roots), ids shifted, one fixed vertex each."""
    a, b = synth.chain_loop(30, 34), synth.chain_loop(25, 28)
    na = a["states"].shape[0]
    return dict(states=np.concatenate([a["states"], b["states"]]),
                fixed=np.concatenate([a["fixed"], b["fixed"]]),
                v0=np.concatenate([a["v0"], b["v0"] + na]).astype(np.int32),
                v1=np.concatenate([a["v1"], b["v1"] + na]).astype(np.int32),
                meas=np.concatenate([a["meas"], b["meas"]]))


GRAPHS = {
    "chain_40": lambda: synth.chain_loop(40, 46),
    "manhattan_300": lambda: synth.manhattan(300, 1500, dims=(8, 8, 3)),
    "kitti_all_loops": lambda: K.build_direct_graph(False),
    "two_chains": two_chains,
}


class Tree:
    """Elimination tree and schedule of a plan of Graph.marginal_plan(), by column (elimination position)."""

    def __init__(self, P):
        nb = P["nb"]
        self.nb, self.colptr, self.lrow = nb, P["colptr"], P["lrow"]
        self.pos = np.empty(nb, dtype=np.int64)  # block row of the system -> column
        self.pos[P["perm"]] = np.arange(nb)
        self.parent = np.full(nb, -1, dtype=np.int64)
        self.depth = np.zeros(nb, dtype=np.int64)
        for j in range(nb - 1, -1, -1):  # parents have larger indices
            if self.colptr[j + 1] - self.colptr[j] > 1:
                self.parent[j] = self.lrow[self.colptr[j] + 1]
                assert self.parent[j] > j
                self.depth[j] = self.depth[self.parent[j]] + 1
        self.group = np.empty(nb, dtype=np.int64)
        self.ngroups = P["ngroups"]
        for g in range(self.ngroups):
            c0, c1 = P["lcolp"][P["gptr"][g]], P["lcolp"][P["gptr"][g + 1]]
            self.group[c0:c1] = g
        lcol = np.repeat(np.arange(nb), np.diff(self.colptr))
        self.stored = set(zip(self.lrow.tolist(), lcol.tolist()))

    def path(self, j):
        out = [j]
        while self.parent[out[-1]] >= 0:
            out.append(int(self.parent[out[-1]]))
        return out

    def lca(self, a, b):
        """lowest common ancestor of two columns (either one included), or -1 across two trees"""
        pa = set(self.path(a))
        for k in self.path(b):
            if k in pa:
                return k
        return -1

    def classes(self, ra, rb):
        """the classes (a subset of CLASSES) of the pair of block rows (ra, rb) of the system"""
        a, b = int(self.pos[ra]), int(self.pos[rb])
        out = set()
        if (max(a, b), min(a, b)) in self.stored:
            out.add("on_pattern")
        else:
            k = self.lca(a, b)
            if k in (a, b):
                out.add("off_ancestor")
            elif k >= 0:
                out.add("off_common")
            else:
                out.add("off_disconnected")
        top = self.ngroups - 1
        if self.group[a] == top and self.group[b] == top:
            out.add("both_top")
        elif self.group[a] != top and self.group[b] != top and self.group[a] != self.group[b]:
            out.add("different_bottom_groups")
        return out

    def classes_of(self, ra, rb):
        out = set()
        for a, b in zip(ra, rb):
            out |= self.classes(a, b)
        return out


def seeded_pairs(T, n, seed, strata=16):
    """Ordered pairs of block rows, self pairs possible: n drawn uniformly, then `strata` with both vertices in the
    top group of the schedule and `strata` with both below it (a uniform draw on a large graph rarely has both in the
    top group: a few dozen columns of hundreds)."""
    rng = np.random.default_rng(seed)
    row_of = np.empty(T.nb, dtype=np.int64)  # column -> block row
    row_of[T.pos] = np.arange(T.nb)
    top = row_of[T.group == T.ngroups - 1]
    low = row_of[T.group != T.ngroups - 1]
    ra, rb = [rng.integers(0, T.nb, n)], [rng.integers(0, T.nb, n)]
    for pool in (top, low):
        if pool.size:
            ra.append(rng.choice(pool, strata))
            rb.append(rng.choice(pool, strata))
    return np.concatenate(ra), np.concatenate(rb)


def replay_paths(T, Lb, Dinv, cols):
    """W(., j) = column j of L^-1 on the root path of j, for the columns asked: {j: (path, blocks)} by the recursion
    of k_cov_paths, asserting that every stored row of a path column is on the path again."""
    out = {}
    for j in cols:
        path = T.path(j)
        at = {k: t for t, k in enumerate(path)}
        acc = np.zeros((len(path), 7, 7))
        acc[0] = np.eye(7)
        for t, m in enumerate(path):
            acc[t] = Dinv[m] @ acc[t]
            for s in range(T.colptr[m] + 1, T.colptr[m + 1]):
                k = int(T.lrow[s])
                assert k in at and at[k] > t, "a stored row of a path column is off the path"
                assert at[k] == T.depth[j] - T.depth[k]  # the kernel's position rule
                acc[at[k]] -= Lb[s] @ acc[t]
        out[j] = (path, acc)
    return out


def replay_pair(T, W, a, b):
    """Z(a, b) = sum over the common suffix of the two paths of W(k, a)^T W(k, b), ascending"""
    k = T.lca(a, b)
    Z = np.zeros((7, 7))
    if k < 0:
        return Z
    n = int(T.depth[k]) + 1
    (pa, wa), (pb, wb) = W[a], W[b]
    assert pa[len(pa) - n:] == pb[len(pb) - n:]
    for t in range(n):
        Z += wa[len(pa) - n + t].T @ wb[len(pb) - n + t]
    return Z
