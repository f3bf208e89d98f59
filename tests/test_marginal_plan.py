"""Host-side plan of the block selected inversion behind the marginal covariances
(sim3opt_amd/csrc/selinv.cpp; g2o's SparseOptimizer::computeMarginals), no GPU needed.

The plan's product lists are replayed here in numpy, in their order and in the kernel's walk (groups
top-down, levels descending, off-diagonal blocks of a level before its diagonal ones), on a random SPD
matrix with the system's block pattern, factored in numpy in the plan's elimination order.  The result
must match a dense inverse; every block a list reads must exist (the pattern is closed under the
recursion) and be final when it is read."""
import numpy as np
import pytest

from sim3opt_amd import lib as L, synth
import kitti_graph as K


def graph_of(g):
    G = L.Graph()
    G.add_vertices(g["states"], g["fixed"])
    G.add_edges(g["v0"], g["v1"], g["meas"])
    return G


def random_spd(rowptr, colidx, rng, shift=0.5):
    """sum over the pattern's off-diagonal blocks of J^T J (random 7 x 14 Jacobians) + shift I"""
    nb = len(rowptr) - 1
    A = np.zeros((7 * nb, 7 * nb))
    for i in range(nb):
        for j in sorted(set(colidx[rowptr[i]:rowptr[i + 1]].tolist())):
            if j <= i:
                continue
            J = rng.standard_normal((7, 14))
            G = J.T @ J
            ii, jj = slice(7 * i, 7 * i + 7), slice(7 * j, 7 * j + 7)
            A[ii, ii] += G[:7, :7]
            A[ii, jj] += G[:7, 7:]
            A[jj, ii] += G[7:, :7]
            A[jj, jj] += G[7:, 7:]
    return A + shift * np.eye(7 * nb)


def replay(P, A):
    """Z on the pattern of L, walked as k_selinv walks it; returns (Z blocks, permuted A)"""
    nb, nL = P["nb"], P["nL"]
    idx = (7 * P["perm"][:, None] + np.arange(7)).ravel()
    Ap = A[np.ix_(idx, idx)]
    Lf = np.linalg.cholesky(Ap)
    lcol = np.repeat(np.arange(nb), np.diff(P["colptr"]))
    lrow = P["lrow"]
    Lb = np.stack([Lf[7 * lrow[s]:7 * lrow[s] + 7, 7 * lcol[s]:7 * lcol[s] + 7] for s in range(nL)])
    Dinv = np.stack([np.linalg.inv(Lb[P["colptr"][j]]) for j in range(nb)])
    Z = np.zeros((nL, 7, 7))
    done = np.zeros(nL, bool)

    def block(s, diag):
        j, i = lcol[s], lrow[s]
        acc = np.zeros((7, 7))
        for p in range(P["zptr"][s], P["zptr"][s + 1]):
            za, zt, zl = P["za"][p], P["zt"][p], P["zl"][p]
            assert 0 <= za < nL and 0 <= zl < nL
            k = lrow[zl]
            assert lcol[zl] == j and k > j  # L(k, j), k in S_j
            if diag:
                assert za == zl and zt == 1  # Z(k, j)^T
            else:  # Z(i, k) as stored: block (max, min), transposed when k > i
                assert (lrow[za], lcol[za]) == (max(i, k), min(i, k)) and zt == int(k > i)
            assert done[za], "the walk reads a block of Z before it is final"
            acc += (Z[za].T if zt else Z[za]) @ Lb[zl]
        Z[s] = ((Dinv[j].T if diag else 0.0) - acc) @ Dinv[j]
        done[s] = True

    ng = P["ngroups"]
    for g in [ng - 1] + list(range(ng - 1)):  # the top group first, then the subtrees
        for l in range(P["gptr"][g + 1] - 1, P["gptr"][g] - 1, -1):
            c0, c1 = P["lcolp"][l], P["lcolp"][l + 1]
            for s in range(P["colptr"][c0], P["colptr"][c1]):
                if lrow[s] != lcol[s]:
                    block(s, False)
            for j in range(c0, c1):
                block(P["colptr"][j], True)
    assert done.all()
    return Z, Ap, lrow, lcol


GRAPHS = {
    "chain_200": lambda: synth.chain_loop(200, 230),
    "tiny_5": lambda: synth.chain_loop(5, 6, min_gap=2),
    "manhattan_300": lambda: synth.manhattan(300, 1500, dims=(8, 8, 3)),
    "kitti_one_loop": lambda: K.build_direct_graph(True),
}


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_selected_inverse_plan_matches_dense_inverse(name):
    G = graph_of(GRAPHS[name]())
    try:
        P = G.marginal_plan()
        rowptr, colidx = G.system_pattern()
    finally:
        G.close()
    nb = P["nb"]
    assert nb == len(rowptr) - 1 and sorted(P["perm"]) == list(range(nb))
    # one list per block of L, |S_j| products each
    ncol = np.diff(P["colptr"]) - 1
    assert np.array_equal(np.diff(P["zptr"]), np.repeat(ncol, ncol + 1))
    assert P["nprod"] == int((ncol * (ncol + 1)).sum())
    A = random_spd(rowptr, colidx, np.random.default_rng(7))
    Z, Ap, lrow, lcol = replay(P, A)
    Zd = np.linalg.inv(Ap)
    ref = np.stack([Zd[7 * lrow[s]:7 * lrow[s] + 7, 7 * lcol[s]:7 * lcol[s] + 7] for s in range(P["nL"])])
    assert np.abs(Z - ref).max() <= 1e-10 * np.abs(ref).max()
    # every edge of the system is in the pattern (the pairs sim3opt_marginals promises)
    pos = np.empty(nb, dtype=np.int64)
    pos[P["perm"]] = np.arange(nb)
    stored = set(zip(lrow.tolist(), lcol.tolist()))
    for i in range(nb):
        for j in colidx[rowptr[i]:rowptr[i + 1]]:
            a, b = pos[i], pos[j]
            assert (max(a, b), min(a, b)) in stored


def test_selected_inverse_order_does_not_depend_on_the_schedule(monkeypatch):
    """The bottom-subtree size renumbers the columns; the products of every block of Z, written in block
    rows of the system, must come in the same order (that is what makes the device result the same bits
    under every schedule)."""
    g = K.build_direct_graph(False)

    def lists():
        G = graph_of(g)
        try:
            P = G.marginal_plan()
        finally:
            G.close()
        perm, lrow = P["perm"], P["lrow"]
        lcol = np.repeat(np.arange(P["nb"]), np.diff(P["colptr"]))
        rc = lambda s: (int(perm[lrow[s]]), int(perm[lcol[s]]))  # noqa: E731
        out = {}
        for s in range(P["nL"]):
            ps = range(P["zptr"][s], P["zptr"][s + 1])
            out[rc(s)] = [(rc(P["za"][p]), int(P["zt"][p]), rc(P["zl"][p])) for p in ps]
        return out, P["ngroups"]

    ref, groups = None, set()
    for subtree in ("16", "48", "128"):
        monkeypatch.setenv("SIM3OPT_DIRECT_SUBTREE", subtree)
        cur, ng = lists()
        groups.add(ng)
        if ref is None:
            ref = cur
        assert cur == ref
    assert len(groups) > 1
