"""The graphs of tests/test_gpu_lm_operators.py: the smallest shapes at which each path of the LM set-up and update
kernels (lm_kernels.hpp) can go wrong.  Every case names the PATH CONDITION it exists for; check_path asserts it on what
the device reports (the read-out's active list, slots and incidences), tests/test_lm_ref.py asserts on the CPU what
follows from the inputs alone (branch coverage, both sides of every kernel's threshold, the share of ill-conditioned
residuals).

A case is a dict: states (nv, 8), fixed (nv,), ids (nv,) or None, v0, v1 (vertex INDICES), meas (ne, 8), info (ne, 7, 7)
or None, kinds / deltas (ne,) or None, options (Graph options the case needs)."""
import functools
import json
import os

import numpy as np

from sim3opt_amd import sim3np as S3
import kitti_graph as K
import lm_ref as LR

CASES = ("tail_1", "tail_7", "fixed_ends", "parallel", "info", "kernels", "info_kernels", "dof_0x78", "branches_b0",
         "branches_b1", "big_e", "rows_8193")
EPB = 8                 # edges per workgroup of the linearisation kernels
REDUCE_STRIDE = 8192    # block rows beyond which k_diag_reduce's grid (2048 workgroups of 4 rows) strides
UNROLL_PARTIALS = 1024  # partial sums from which sum_partials' four-way loop runs (i + 3 * 256 < n)
PARTIAL_COUNTS = (1, 255, 256, 257, 1023, 1024, 1025, 2048)
GOLD = os.path.join(os.path.dirname(__file__), "golden", "oracle_golden.json")


def _generic_xi(rng, m, rot=(0.3, 1.0), trans=1.0, sig=(0.01, 0.3)):
    """Residuals away from every branch threshold: theta in `rot`, |sigma| in `sig`."""
    ax = rng.standard_normal((m, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    th = rng.uniform(*rot, (m, 1))
    sg = rng.uniform(*sig, (m, 1)) * rng.choice([-1.0, 1.0], (m, 1))
    return np.concatenate([ax * th, rng.standard_normal((m, 3)) * trans, sg], axis=1)


def _states(rng, n):
    xi = np.concatenate([rng.standard_normal((n, 3)) * 0.8, rng.standard_normal((n, 3)) * 3, rng.uniform(-0.3, 0.3, (n, 1))], 1)
    return S3.exp(xi, fix_b=True)


def _graph(rng, nv, v0, v1, xi=None, fixed=(0,), **kw):
    """Random estimates; measurements C = exp(xi) S1 S0^-1, so that the residual log(C S0 S1^-1) is xi."""
    v0, v1 = np.asarray(v0, dtype=np.int32), np.asarray(v1, dtype=np.int32)
    st = _states(rng, nv)
    xi = _generic_xi(rng, v0.shape[0]) if xi is None else xi
    meas = S3.mul(S3.exp(xi, fix_b=True), S3.mul(st[v1], S3.inv(st[v0])))
    fx = np.zeros(nv, dtype=np.uint8)
    fx[list(fixed)] = 1
    g = dict(states=st, fixed=fx, ids=None, v0=v0, v1=v1, meas=meas, info=None, kinds=None, deltas=None, options={})
    g.update(kw)
    return g


def _chain(n):
    return np.arange(1, n), np.arange(0, n - 1)


def spd_info(rng, m):
    """SPD, non-diagonal, exactly symmetric, weights spread over four orders of magnitude (weak edges beside strong)."""
    M = rng.standard_normal((m, 7, 7)) * 0.3
    A = np.einsum("kij,klj->kil", M, M) + np.eye(7)
    A = (A + A.transpose(0, 2, 1)) / 2
    return A * (10.0 ** rng.uniform(-2, 2, (m, 1, 1)))


def _with_kernels(g, rng):
    """Every robust kind on two edges at least: one residual below its threshold, one above (Tukey above: w = 0); the
    deltas follow from the edges' own chi2 = e^T Omega e (float64 restatement)."""
    m = g["v0"].shape[0]
    o = LR.mopts(**g["options"])
    e = LR.edge_error(g["meas"], g["states"][g["v0"]], g["states"][g["v1"]], o, np.float64)
    chi, _, _ = LR.chi_rho_w(e, g["info"], None, None, np.float64)
    kinds = np.zeros(m, dtype=np.int32)
    deltas = np.zeros(m)
    above = np.zeros(m, dtype=bool)
    order = rng.permutation(m)
    for j, k in enumerate(order):
        kind = j % 10  # NONE included: an edge without a kernel among edges with one
        kinds[k] = kind
        above[k] = (j // 10) % 2 == 1
        ratio = 4.0 if above[k] else 0.25  # chi / threshold
        thr = chi[k] / ratio
        # HUBER, PSEUDO_HUBER, CAUCHY, WELSCH, FAIR, TUKEY, SATURATED: chi against delta^2; GEMAN_MCCLURE, DCS: delta
        deltas[k] = 0.0 if kind == 0 else (thr if kind in (4, 9) else np.sqrt(thr))
    g["kinds"], g["deltas"], g["above"] = kinds, deltas, above
    return g


def _mixed(seed, info, kernels):
    rng = np.random.default_rng(seed)
    nv = 30
    c0, c1 = _chain(nv)
    l0 = rng.integers(0, nv, 31)
    l1 = (l0 + rng.integers(2, nv - 2, 31)) % nv
    g = _graph(rng, nv, np.concatenate([c0, l0]), np.concatenate([c1, l1]))
    if info:
        g["info"] = spd_info(rng, g["v0"].shape[0])
    return _with_kernels(g, rng) if kernels else g


def _fixed_ends():
    rng = np.random.default_rng(41)
    nv = 12
    c0, c1 = _chain(nv)
    # vertices 3 and 8 fixed: chain edges (3, 2) and (8, 7) have endpoint 0 fixed, (4, 3) and (9, 8) endpoint 1; the
    # extra edge (3, 8) joins the two fixed vertices
    v0 = np.concatenate([c0, [3, 5, 8]])
    v1 = np.concatenate([c1, [8, 3, 10]])
    ids = (np.arange(nv) * 13 - 100).astype(np.int32)  # arbitrary, negative among them
    return _graph(rng, nv, v0, v1, fixed=(3, 8), ids=ids)


def _parallel():
    rng = np.random.default_rng(42)
    nv = 48  # vertex 0 fixed, vertex 1 the hub, leaves 2 ... 47 with ONE incidence each
    leaves = np.arange(2, nv)
    v0 = np.concatenate([[1], leaves[::2], np.ones(leaves[1::2].shape[0], dtype=int)])
    v1 = np.concatenate([[0], np.ones(leaves[::2].shape[0], dtype=int), leaves[1::2]])
    g = _graph(rng, nv, v0, v1)
    # edge 5 again (a parallel edge: its own slots) and reversed (v1 -> v0, the inverse measurement)
    a, b = int(g["v0"][5]), int(g["v1"][5])
    g["v0"] = np.concatenate([g["v0"], [a, b]]).astype(np.int32)
    g["v1"] = np.concatenate([g["v1"], [b, a]]).astype(np.int32)
    g["meas"] = np.concatenate([g["meas"], g["meas"][5:6], S3.inv(g["meas"][5:6])])
    g["dup"] = (5, g["v0"].shape[0] - 2, g["v0"].shape[0] - 1)
    return g


def _branches(fixb):
    """Residuals on every exp / log branch (the table of the parity test, tests/golden), every second estimate with a
    negative-w quaternion, diluted with generic edges so that the ill-conditioned share stays small."""
    xi_t = np.array(json.load(open(GOLD))["explog"]["xi"])
    rng = np.random.default_rng(11)
    mt = xi_t.shape[0]
    m = 12 * mt
    xi = np.concatenate([xi_t, _generic_xi(rng, m - mt)])
    nv = 2 * m
    g = _graph(rng, nv, np.arange(m), np.arange(m, 2 * m), xi=xi, options=dict(fix_small_angle_b=fixb))
    neg = np.arange(nv) % 2 == 1
    g["states"][neg, :4] *= -1.0
    g["table"] = mt
    return g


def _big_e():
    g = K.build_direct_graph(False)
    return dict(states=g["states"], fixed=g["fixed"], ids=None, v0=g["v0"], v1=g["v1"], meas=g["meas"], info=None,
                kinds=None, deltas=None, options={})


def _rows(nv, loops, seed):
    rng = np.random.default_rng(seed)
    c0, c1 = _chain(nv)
    l0 = rng.integers(100, nv, loops)
    l1 = l0 - rng.integers(50, 100, loops)
    m = nv - 1 + loops
    xi = _generic_xi(rng, m, rot=(0.3, 0.6), trans=0.3, sig=(0.01, 0.1))
    return _graph(rng, nv, np.concatenate([c0, l0]), np.concatenate([c1, l1]), xi=xi)


@functools.lru_cache(maxsize=None)
def graph(name):
    if name == "tail_1":
        return _graph(np.random.default_rng(31), 18, *_chain(18))  # 17 active edges: 2 workgroups + 1 edge
    if name == "tail_7":
        return _graph(np.random.default_rng(32), 8, *_chain(8))    # 7 active edges: less than one workgroup
    if name == "fixed_ends":
        return _fixed_ends()
    if name == "parallel":
        return _parallel()
    if name == "info":
        return _mixed(51, True, False)
    if name == "kernels":
        return _mixed(52, False, True)
    if name == "info_kernels":
        return _mixed(53, True, True)
    if name == "dof_0x78":
        g = _mixed(54, True, True)
        g["options"] = dict(dof_mask=0x78)
        return g
    if name in ("branches_b0", "branches_b1"):
        return _branches(int(name[-1]))
    if name == "big_e":
        return _big_e()
    if name == "rows_8193":
        return _rows(8194, 6, 61)
    if name == "partitioned":  # numeric mode, information matrices and kernels on a graph large enough to partition
        from sim3opt_amd import synth
        synth.DRIFT_TARGET = 0.05
        m = synth.manhattan(600, 3600, dims=(8, 8, 8), seed_graph=71, seed_noise=72)
        rng = np.random.default_rng(73)
        g = dict(states=m["states"], fixed=m["fixed"], ids=None, v0=m["v0"], v1=m["v1"], meas=m["meas"],
                 info=spd_info(rng, m["v0"].shape[0]), kinds=None, deltas=None, options={})
        return _with_kernels(g, rng)
    if name == "partials":
        return _rows(3001, 1000, 62)  # 4000 edges, 21000 scalars: a grid of 1 strides 16 and 83 times
    raise KeyError(name)


def make(L, g, **options):
    """The library's Graph of a case, initialised."""
    opts = dict(g["options"])
    opts.update(options)
    G = L.Graph(**opts)
    G.add_vertices(g["states"], g["fixed"], g["ids"])
    v0, v1 = g["v0"], g["v1"]
    if g["ids"] is not None:
        v0, v1 = g["ids"][v0], g["ids"][v1]
    if g["kinds"] is None:
        G.add_edges(v0, v1, g["meas"], info=g["info"])
    else:
        G.add_edges(v0, v1, g["meas"], info=g["info"], kernel=g["kinds"], kernel_delta=g["deltas"])
    G.initialize()
    return G


def check_path(name, g, d):
    """The path condition of a case, on the device's read-out d (Graph.debug_linearization) and the case's arrays."""
    na = d["active"].shape[0]
    nb = d["incptr"].shape[0] - 1
    act = np.zeros(g["v0"].shape[0], dtype=bool)
    act[d["active"]] = True
    fx0, fx1 = g["fixed"][g["v0"]] != 0, g["fixed"][g["v1"]] != 0
    # what holds for every case: the active edges are those with a free endpoint, slots and incidences follow `fixed`
    assert np.array_equal(act, ~(fx0 & fx1))
    assert np.array_equal(d["inc0"] < 0, fx0) and np.array_equal(d["inc1"] < 0, fx1)
    assert np.array_equal(d["slot01"] < 0, fx0 | fx1) and np.array_equal(d["slot10"] < 0, fx0 | fx1)
    inc = np.concatenate([d["inc0"][d["inc0"] >= 0], d["inc1"][d["inc1"] >= 0]])
    assert np.array_equal(np.sort(inc), np.arange(d["incptr"][-1]))  # every incidence slot owned by exactly one endpoint
    cnt = np.diff(d["incptr"])
    if name == "tail_1":
        assert na % EPB == 1 and na > EPB
    if name == "tail_7":
        assert na % EPB == 7 and na < EPB
    if name == "fixed_ends":
        assert (fx0 & ~fx1).any() and (~fx0 & fx1).any() and (fx0 & fx1).sum() == 1 and g["fixed"].sum() == 2
        assert (g["ids"] < 0).any() and na == g["v0"].shape[0] - 1
    if name == "parallel":
        k, kd, kr = g["dup"]
        assert g["v0"][k] == g["v0"][kd] == g["v1"][kr] and g["v1"][k] == g["v1"][kd] == g["v0"][kr]
        assert len({int(d["slot01"][k]), int(d["slot01"][kd]), int(d["slot10"][kr])}) == 3  # separate slots
        assert cnt.max() >= 40 and (cnt == 1).sum() >= 40
    if name == "rows_8193":
        assert nb > REDUCE_STRIDE and (nb + 3) // 4 > UNROLL_PARTIALS
    if name == "big_e":
        assert nb == 770 and na == g["v0"].shape[0] > 770  # KITTI-00 with all loops: one fixed vertex, every edge active
    return dict(n_active=na, rows=nb, max_incidences=int(cnt.max()))
