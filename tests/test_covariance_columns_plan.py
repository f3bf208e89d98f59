"""The host side of options.cov_solver (blocks of (H + lambda I)^-1 by columns of the inverse), no GPU needed: the two
option fields and sim3opt_covariance_columns_plan -- the vertices whose seven columns a request needs.  Every requested
unordered pair must have an endpoint among them (block (a, b) is rows a of the columns of b); the cover is greedy and
deterministic: the vertex that covers the most pairs not yet covered, ties to the lowest block row."""
import numpy as np
import pytest

from sim3opt_amd import lib as L, synth


def graph(ids=None):
    g = synth.chain_loop(40, 46)
    G = L.Graph()
    ids = np.arange(40, dtype=np.int32) if ids is None else ids
    G.add_vertices(g["states"], g["fixed"], ids)
    G.add_edges(ids[g["v0"]], ids[g["v1"]], g["meas"])
    return G, g, ids


def greedy(pairs, row_of):
    """the cover restated: most uncovered pairs first, ties to the lowest block row"""
    left = {(min(a, b), max(a, b)) for a, b in pairs}
    out = []
    while left:
        cnt = {}
        for a, b in left:
            for v in {a, b}:
                cnt[v] = cnt.get(v, 0) + 1
        v = min(cnt, key=lambda u: (-cnt[u], row_of[u]))
        out.append(v)
        left = {p for p in left if v not in p}
    return out


def test_option_defaults_and_validation():
    o = L.default_options()
    assert o.cov_solver == 0 and o.cov_rel_tol == 1e-8
    G = L.Graph(cov_solver=1, cov_rel_tol=1e-6)
    try:
        assert G.options().cov_solver == 1 and G.options().cov_rel_tol == 1e-6
        for bad in (0.0, -1e-8, 2e-2, 1.0, float("nan"), float("inf")):
            with pytest.raises(L.Sim3OptError) as e:
                G.set_options(cov_rel_tol=bad)
            assert e.value.code == L.ERR_ARG
            assert G.options().cov_rel_tol == 1e-6
        G.set_options(cov_rel_tol=1e-2)  # the upper end is allowed
        assert G.options().cov_rel_tol == 1e-2
        for bad in (-1, 3):
            with pytest.raises(L.Sim3OptError) as e:
                G.set_options(cov_solver=bad)
            assert e.value.code == L.ERR_ARG
            assert G.options().cov_solver == 1
        G.set_options(cov_solver=2)
        assert G.options().cov_solver == 2
    finally:
        G.close()


def test_plan_of_a_block_column_and_of_the_diagonal():
    ids = (np.arange(40) * 5 + 2).astype(np.int32)
    G, g, ids = graph(ids)
    try:
        free = ids[np.asarray(g["fixed"]) == 0]
        b = int(free[17])
        column = [(int(a), b) for a in free]
        assert G.covariance_columns_plan(column).tolist() == [b]
        assert G.covariance_columns_plan([(y, x) for x, y in column]).tolist() == [b]
        diag = [(int(a), int(a)) for a in free[::-1]]
        assert G.covariance_columns_plan(diag).tolist() == free.tolist()  # every vertex once, block rows ascending
        assert G.covariance_columns_plan(np.zeros((0, 2), dtype=np.int32)).tolist() == []
    finally:
        G.close()


def test_plan_covers_seeded_pairs_and_ignores_duplicates():
    G, g, ids = graph()
    try:
        free = ids[np.asarray(g["fixed"]) == 0]
        row_of = {int(v): r for r, v in enumerate(free)}
        rng = np.random.default_rng(7)
        pairs = np.stack([rng.choice(free, 200), rng.choice(free, 200)], axis=1)
        plan = G.covariance_columns_plan(pairs).tolist()
        assert len(set(plan)) == len(plan) and set(plan) <= set(free.tolist())
        chosen = set(plan)
        assert all(int(a) in chosen or int(b) in chosen for a, b in pairs)
        assert plan == greedy(pairs.tolist(), row_of)
        # duplicates, reversed copies and the order of the request do not matter
        dup = np.concatenate([pairs, pairs[::3, ::-1], pairs[:50]])
        assert G.covariance_columns_plan(dup).tolist() == plan
        assert G.covariance_columns_plan(pairs[rng.permutation(200)]).tolist() == plan
        # ... nor whether the graph has been initialised (host only); a sparse request costs fewer vertices than pairs
        few = pairs[:12]
        assert len(G.covariance_columns_plan(few)) <= len({(min(a, b), max(a, b)) for a, b in few.tolist()})
    finally:
        G.close()


def test_plan_refuses_fixed_and_unknown_vertices():
    G, g, ids = graph()
    try:
        fixed_id = int(ids[np.flatnonzero(g["fixed"])[0]])
        for bad in ([(fixed_id, 5)], [(5, fixed_id)], [(5, 100000)], [(-7, 5)], [(fixed_id, fixed_id)]):
            with pytest.raises(L.Sim3OptError) as e:
                G.covariance_columns_plan(bad)
            assert e.value.code == L.ERR_ARG
    finally:
        G.close()
