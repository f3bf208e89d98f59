"""Patterns and values for the operator tests of the exact block Cholesky (tests/test_factor_ref.py on the CPU,
tests/test_gpu_factor_operators.py on the device).  A case is a small pose graph chosen for the PATH its plan sends
k_ldl, ldl_back, k_selinv down (paths(): asserted from the host plan by test_factor_ref.py's PATHS, so a planner change
that moves a case off its path fails there), and injected values: edge Grams on the pattern scaled by powers of two per
vertex."""
import numpy as np

from sim3opt_amd import lib as L, sim3np as S3
import kitti_graph as K

LAMBDAS = (0.0, 1e-2, 1e3)
STAGE, WCH = 112, 14  # DirectPlan::STAGE_PRODUCTS and a wavefront's slice of it (direct_args.hpp)


def _graph(nv, edges, fixed=(0,), seed=5):
    """Vertices near random poses, measurements a small step off the relative pose: a graph that linearises to a
    well-posed system whatever its pattern."""
    rng = np.random.default_rng(seed)
    xi = rng.standard_normal((nv, 7)) * np.array([0.3] * 3 + [2.0] * 3 + [0.1])
    Sgt = S3.exp(xi, fix_b=True)
    e = np.asarray(edges, dtype=np.int32).reshape(-1, 2)
    v0, v1 = e[:, 0].copy(), e[:, 1].copy()
    noise = rng.standard_normal((len(e), 7)) * 0.02
    meas = S3.mul(S3.exp(noise, fix_b=True), S3.mul(Sgt[v1], S3.inv(Sgt[v0])))
    states = S3.mul(S3.exp(rng.standard_normal((nv, 7)) * 0.01, fix_b=True), Sgt)
    fx = np.zeros(nv, dtype=np.uint8)
    fx[list(fixed)] = 1
    return dict(states=states, fixed=fx, v0=v0, v1=v1, meas=meas)


def star(n):
    """vertex 0 fixed, hub 1, leaves 2 .. n + 1"""
    return _graph(n + 2, [(0, 1)] + [(1, k) for k in range(2, n + 2)])


def clique(n, tail=0):
    """vertex 0 fixed on vertex 1; all pairs of 1 .. n; a chain of `tail` vertices from n back round to vertex 2"""
    e = [(0, 1)] + [(a, c) for a in range(1, n + 1) for c in range(a + 1, n + 1)]
    if tail:
        ch = [n] + list(range(n + 1, n + tail + 1)) + [2]
        e += list(zip(ch[:-1], ch[1:]))
    return _graph(n + tail + 1, e)


def chain(n, loops=((3, 30), (10, 22), (1, 40))):
    return _graph(n + 1, [(k, k + 1) for k in range(n)] + list(loops))


def two_components():
    """two chains with a loop each, no edge between them, a fixed vertex on each"""
    a = [(0, 1)] + [(k, k + 1) for k in range(1, 9)] + [(2, 8)]
    c = [(10, 11)] + [(k, k + 1) for k in range(11, 23)] + [(12, 20), (14, 23)]
    return _graph(24, a + c, fixed=(0, 10))


CASES = {
    "one_free": lambda: _graph(2, [(0, 1)]),
    "two_free": lambda: _graph(3, [(0, 1), (1, 2)]),
    "parallel": lambda: _graph(4, [(0, 1), (1, 2), (1, 2), (2, 1), (2, 3), (3, 1)]),
    "star_16": lambda: star(16),
    "star_112": lambda: star(112),
    "star_113": lambda: star(113),
    "star_130": lambda: star(130),
    "clique_24": lambda: clique(24),
    "clique_66": lambda: clique(66),
    "clique_12_tail20": lambda: clique(12, 20),
    "chain_40": lambda: chain(40),
    "two_components": two_components,
    "kitti_one_loop": lambda: K.build_direct_graph(True),
    "kitti_all_loops": lambda: K.build_direct_graph(False),
}


def graph_of(g, **options):
    G = L.Graph(**options)
    G.add_vertices(g["states"], g["fixed"])
    G.add_edges(g["v0"], g["v1"], g["meas"])
    return G


def injected(g, rowptr, colidx, seed=3, scaled=True):
    """(vals (nnzb, 7, 7), b (nb, 7)): a Gram [Ja Jc]^T [Ja Jc] per edge between free vertices on the graph's own
    pattern (parallel edges keep separate blocks, as the linearisation leaves them), J^T J on the diagonal for an edge
    to a fixed vertex -- SPD at lambda = 0 -- scaled by 2^e(a) 2^e(c), e in -20 .. 20 per vertex: the blocks span
    2^-40 .. 2^40, 24 decimal decades, the matrix stays SPD, and powers of two commute with rounding.  b scaled likewise."""
    rng = np.random.default_rng(seed)
    nb = len(rowptr) - 1
    rows = np.repeat(np.arange(nb), np.diff(rowptr))
    hidx = np.cumsum(g["fixed"] == 0) - 1
    vals = np.zeros((len(colidx), 7, 7))
    slots = {}
    for k in range(len(colidx)):
        if rows[k] != colidx[k] or k != rowptr[rows[k]]:
            slots.setdefault((rows[k], colidx[k]), []).append(k)
    used = {}
    for a, c in zip(g["v0"], g["v1"]):
        fa, fc = g["fixed"][a] == 0, g["fixed"][c] == 0
        Ja, Jc = _jacs(rng)
        if fa:
            vals[rowptr[hidx[a]]] += Ja.T @ Ja
        if fc:
            vals[rowptr[hidx[c]]] += Jc.T @ Jc
        if fa and fc:
            ra, rc = hidx[a], hidx[c]
            # the blocks of row ra at column rc are sorted by edge, and so are those of row rc at column ra
            i = used.get((min(ra, rc), max(ra, rc)), 0)
            used[(min(ra, rc), max(ra, rc))] = i + 1
            vals[slots[(ra, rc)][i]] = Ja.T @ Jc
            vals[slots[(rc, ra)][i]] = Jc.T @ Ja
    b = rng.standard_normal((nb, 7))
    if scaled:
        sc = np.ldexp(1.0, rng.integers(-20, 21, nb))
        sc[rng.integers(0, nb)] = 2.0 ** 20  # (both ends of the range on every case with two vertices or more)
        sc[rng.integers(0, nb)] = 2.0 ** -20
        vals *= (sc[rows] * sc[colidx])[:, None, None]
        b *= sc[:, None]
    return vals, b


def _jacs(rng):
    """An edge's two 7x7 Jacobians: Ja with singular values in 0.5 .. 2, Jc = -Ja Q with Q orthogonal, as an adjoint
    relates the two ends of a pose-graph edge.  Jc^-1 Ja is then orthogonal, so uncertainty grows additively along a
    chain instead of exponentially (two independent random Jacobians per edge leave KITTI-00's chain of 770 without a
    positive pivot in float64 at lambda = 0)."""
    q = [np.linalg.qr(rng.standard_normal((7, 7)))[0] for _ in range(3)]
    Ja = (q[0] * rng.uniform(0.5, 2.0, 7)) @ q[1]
    return Ja, -Ja @ q[2]


def paths(P):
    """What the plan makes the kernels do, measured on the host plan: a dict of the numbers PATHS pins."""
    cp, pp = P["colptr"], P["pairptr"]
    npd = np.diff(pp)
    cells = P["cells"].reshape(-1, 18)
    rounds = cells[:, 17] - cells[:, 9]
    coop = rounds <= STAGE
    out = dict(nb=P["nb"], nL=P["nL"], npairs=P["npairs"], ngroups=P["ngroups"], height=P["height"],
               max_products=int(npd.max()), max_sources=int(np.diff(P["srcptr"]).max()),
               no_source_blocks=int((np.diff(P["srcptr"]) == 0).sum()),
               max_offdiag=int(np.diff(cp).max() - 1), max_round=int(rounds.max()),
               max_coop_round=int(rounds[coop].max()), wide_rounds=int((~coop).sum()),
               max_rounds_per_level=int(np.diff(P["rptr"]).max()),
               max_cell_blocks=int(np.diff(cells[:, :9], axis=1).max()), nprod=P.get("nprod", 0))
    # wide rounds: a wavefront stages its own products 14 at a time from the start of its cell
    span = cut = pieces = 0
    for q in np.nonzero(~coop)[0]:
        for w in range(8):
            s0, s1, k0 = cells[q, w], cells[q, w + 1], cells[q, 9 + w]
            for s in range(s0, s1):
                a, e = pp[s] - k0, pp[s + 1] - k0  # the block's products, relative to the cell's first
                if e > a:
                    first, last = a // WCH, (e - 1) // WCH
                    span += last > first
                    pieces = max(pieces, last - first + 1)
                    # a piece end inside the block after an odd number of its products cuts a pair
                    cut += sum(1 for t in range(first + 1, last + 1) if (t * WCH - a) % 2 == 1)
    out.update(blocks_spanning_pieces=int(span), pairs_cut=int(cut), max_pieces=int(pieces))
    depth = np.zeros(P["nb"], dtype=int)
    for j in range(P["nb"] - 1, -1, -1):
        if cp[j + 1] - cp[j] > 1:
            depth[j] = depth[P["lrow"][cp[j] + 1]] + 1
    out.update(max_root_path=int(depth.max()) + 1, roots=int((np.diff(cp) == 1).sum()))
    return out


def leaves_of(T):
    """columns without children in the elimination tree, deepest first: two of them are never on the pattern"""
    has = np.zeros(T.nb, bool)
    has[T.parent[T.parent >= 0]] = True
    lv = np.nonzero(~has)[0]
    return [int(j) for j in lv[np.argsort(-T.depth[lv], kind="stable")]]


def suffix_pairs(T, lengths=(1, 8, 9, 17)):
    """{n: (a, b)}: a pair of columns outside the pattern whose root paths share exactly n blocks (cov_ref.Tree):
    two leaves below different children of a column k of depth n - 1, or a leaf below k and k itself."""
    kids = [[] for _ in range(T.nb)]
    for j in range(T.nb):
        if T.parent[j] >= 0:
            kids[T.parent[j]].append(j)

    def leaf(j):
        while kids[j]:
            j = kids[j][0]
        return j

    out = {}
    for k in range(T.nb):
        n = int(T.depth[k]) + 1
        if n not in lengths or n in out:
            continue
        if len(kids[k]) >= 2:
            out[n] = (leaf(kids[k][0]), leaf(kids[k][1]))
        elif kids[k] and (k, leaf(k)) not in T.stored:
            out[n] = (leaf(k), k)
    return out
