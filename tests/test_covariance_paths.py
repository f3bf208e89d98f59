"""The maths behind sim3opt_covariances' blocks outside the factor's pattern (cov_kernels.hpp), no GPU needed.

With H = L L^T in the plan's elimination order and W = L^-1, Z(i, j) = sum_k W(k, i)^T W(k, j), and column j of W
lives on the root path of j in the elimination tree.  The recursion the kernel runs is replayed in numpy on a random
SPD matrix with the system's pattern (helpers of test_marginal_plan.py), factored in the plan's order; every stored
row of a path column must be on the path again, and seeded pairs must match the dense inverse to the bound
test_marginal_plan.py uses.  The sampled pairs must contain every class of pair the device tests rely on."""
import numpy as np
import pytest

from sim3opt_amd import lib as L
import cov_ref as R
from test_marginal_plan import graph_of, random_spd


def plan_and_factor(name, seed=11):
    G = graph_of(R.GRAPHS[name]())
    try:
        P = G.marginal_plan()
        rowptr, colidx = G.system_pattern()
    finally:
        G.close()
    A = random_spd(rowptr, colidx, np.random.default_rng(seed))
    idx = (7 * P["perm"][:, None] + np.arange(7)).ravel()
    Ap = A[np.ix_(idx, idx)]
    Lf = np.linalg.cholesky(Ap)
    lcol = np.repeat(np.arange(P["nb"]), np.diff(P["colptr"]))
    Lb = np.stack([Lf[7 * i:7 * i + 7, 7 * j:7 * j + 7] for i, j in zip(P["lrow"], lcol)])
    Dinv = np.stack([np.linalg.inv(Lb[P["colptr"][j]]) for j in range(P["nb"])])
    return P, R.Tree(P), Ap, Lb, Dinv


@pytest.mark.parametrize("name", sorted(R.GRAPHS))
def test_path_recursion_matches_dense_inverse(name):
    P, T, Ap, Lb, Dinv = plan_and_factor(name)
    nb = P["nb"]
    if nb <= 60:  # every ordered pair, self pairs included
        ra, rb = (x.ravel() for x in np.meshgrid(np.arange(nb), np.arange(nb)))
    else:
        ra, rb = R.seeded_pairs(T, 300, 3)
    seen = T.classes_of(ra, rb)
    assert set(R.CLASSES) <= seen, set(R.CLASSES) - seen
    Zd = np.linalg.inv(Ap)
    scale = np.abs(Zd).max()
    W = R.replay_paths(T, Lb, Dinv, sorted(set(T.pos[ra].tolist()) | set(T.pos[rb].tolist())))
    worst = 0.0
    for a, b in zip(T.pos[ra], T.pos[rb]):
        a, b = int(a), int(b)
        Z = R.replay_pair(T, W, a, b)
        ref = Zd[7 * a:7 * a + 7, 7 * b:7 * b + 7]
        worst = max(worst, np.abs(Z - ref).max())
        if T.lca(a, b) < 0:
            assert np.all(Z == 0.0)
    print(f"{name}: {ra.size} pairs, max|err| / max|ref| {worst / scale:.2e}")
    assert worst <= 1e-10 * scale


def test_class_counts_of_the_smallest_graph():
    """Over all unordered pairs of distinct vertices of the 40-chain every class is there (the device test asks the
    same of what it requests)."""
    P, T, *_ = plan_and_factor("chain_40")
    nb = P["nb"]
    count = dict.fromkeys(R.CLASSES, 0)
    for a in range(nb):
        for b in range(a):
            for c in T.classes(a, b):
                count[c] += 1
    print(count)
    assert count["on_pattern"] + count["off_ancestor"] + count["off_common"] == nb * (nb - 1) // 2
    assert all(count[c] > 0 for c in R.CLASSES)


def test_components_share_no_ancestor():
    P, T, Ap, _, _ = plan_and_factor("two_chains")
    g = R.two_chains()
    free = np.flatnonzero(g["fixed"] == 0)
    first = int((free < 30).sum())  # block rows of the first chain (insertion order)
    roots = np.flatnonzero(T.parent < 0)
    assert roots.size == 2
    Zd = np.linalg.inv(Ap)
    for ra in range(first):
        for rb in range(first, P["nb"]):
            a, b = int(T.pos[ra]), int(T.pos[rb])
            assert T.lca(a, b) < 0 and T.classes(ra, rb) >= {"off_disconnected"}
            assert np.all(Zd[7 * a:7 * a + 7, 7 * b:7 * b + 7] == 0.0)
    # ... and within a component every pair has one
    assert all(T.lca(int(T.pos[a]), int(T.pos[b])) >= 0 for a in range(first) for b in range(a))


def test_workspace_option():
    """options.cov_workspace_mb: 256 by default, at least 1, kept by the handle"""
    assert L.default_options().cov_workspace_mb == 256.0
    G = L.Graph(cov_workspace_mb=1.0)
    try:
        assert G.options().cov_workspace_mb == 1.0
        for bad in (0.5, 0.0, -1.0, float("inf"), float("nan")):
            with pytest.raises(L.Sim3OptError) as e:
                G.set_options(cov_workspace_mb=bad)
            assert e.value.code == L.ERR_ARG
        assert G.options().cov_workspace_mb == 1.0
    finally:
        G.close()
