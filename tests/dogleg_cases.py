"""The graphs, vectors and scalar sets of tests/test_gpu_dogleg_operators.py, tests/test_gpu_column_vectors.py and
tests/test_dogleg_rule.py: the smallest shapes at which each path of the dogleg kernels (algo_kernels.hpp), of the
column kernels (col_kernels.hpp) and of the step rule (dogleg_rule.hpp) can go wrong.  As in lm_cases.py every case
names the PATH CONDITION it exists for, and check_* asserts it from the inputs alone.

A graph is a dict as in lm_cases.py (states, fixed, ids, v0, v1, meas, info, kinds, deltas, options)."""
import functools

import numpy as np

import lm_cases as C

WG = 256            # threads of a workgroup: entries per workgroup of k_dl_dots, vertices per workgroup of k_dogleg_oplus
MAX_GRID = 2048     # grid cap of the streaming kernels = most partials of a dot
UNROLL = 1024       # partials from which sum_partials' four-way loop runs (i + 3 * 256 < n)
LD = np.longdouble


# ------------------------------------------------------------------------------------------------ graphs
def _loops(nv, loops, seed, fixed):
    rng = np.random.default_rng(seed)
    c0, c1 = C._chain(nv)
    l0 = rng.integers(8, nv, loops)
    l1 = l0 - rng.integers(2, 8, loops)
    m = nv - 1 + loops
    xi = C._generic_xi(rng, m, rot=(0.3, 0.6), trans=0.3, sig=(0.01, 0.1))
    return C._graph(rng, nv, np.concatenate([c0, l0]), np.concatenate([c1, l1]), xi=xi, fixed=fixed)


DOT_GRAPHS = ("rows_36", "rows_37", "partials", "rows_8193")
UPDATE_GRAPHS = ("nv_255", "nv_256", "nv_257")


@functools.lru_cache(maxsize=None)
def graph(name):
    if name == "rows_36":   # 252 entries: one workgroup of k_dl_dots, partly filled (KITTI-size: 7 x 36 rows)
        return _loops(37, 9, 81, (0,))
    if name == "rows_37":   # 259 entries: a second workgroup with 3 entries; an odd row count
        return _loops(38, 9, 82, (0,))
    if name in ("partials", "rows_8193"):  # 3000 rows: every grid of PARTIAL_COUNTS; 8193 rows: every span_grid class
        return C.graph(name)
    if name in UPDATE_GRAPHS:  # vertices either side of one workgroup of k_dogleg_oplus; fixed first, interior, last
        nv = int(name[3:])
        return _loops(nv, 40, 83 + nv, (0, nv // 3, nv - 1))
    if name == "columns":   # 80 rows, 560 entries: room for every vector length of the column cases, PCG path
        return _loops(81, 20, 90, (0,))
    raise KeyError(name)


def hidx_of(g):
    h = np.full(g["fixed"].shape[0], -1)
    h[g["fixed"] == 0] = np.arange(int((g["fixed"] == 0).sum()))
    return h


def check_graph(name, g):
    """The path condition of a graph, from its arrays alone; returns (rows, entries)."""
    nv = g["fixed"].shape[0]
    nb = int((g["fixed"] == 0).sum())
    n = 7 * nb
    if name == "rows_36":
        assert nb == 36 and n == 252 < WG
    if name == "rows_37":
        assert nb == 37 and WG < n == 259 < 2 * WG and n % 2 == 1
    if name == "partials":
        assert 3000 <= nb <= 5000 and n > 64 * WG  # a grid of 1 strides more than 64 times; 2048 leaves workgroups empty
        assert (n + WG - 1) // WG < 255            # ... so every count of PARTIAL_COUNTS from 255 on is forced, not natural
    if name == "rows_8193":
        assert (nb + 3) // 4 > MAX_GRID            # the span_grid clamp admits more than 2048 SpMV partials
    if name in UPDATE_GRAPHS:
        h = hidx_of(g)
        free = np.flatnonzero(h >= 0)
        assert nv == int(name[3:]) and g["fixed"][0] and g["fixed"][nv - 1] and g["fixed"][1:nv - 1].sum() == 1
        assert len(set((free - h[free]).tolist())) > 1  # hidx[v] != v - const: a kernel that ignores hidx reads another row
        assert (nv + WG - 1) // WG == (1 if nv <= WG else 2)
    return nb, n


# ------------------------------------------------------------------------------------------------ vectors (h_gn)
VECTORS = ("generic", "orthogonal", "decades", "zero")


def vector(kind, b, seed=5):
    """h_gn of a kind for the system's own b (7 per block row)."""
    rng = np.random.default_rng(seed)
    n = b.shape[0]
    r = rng.standard_normal(n)
    if kind == "generic":
        return r * 0.1
    if kind == "orthogonal":  # b . g = 0 to rounding: the bound must rest on sum |b_i g_i|, not on the value
        bl = np.asarray(b, dtype=LD)
        g = np.asarray(r, dtype=LD)
        g = g - (g @ bl) / (bl @ bl) * bl
        return np.asarray(g, dtype=np.float64)
    if kind == "decades":     # entries spread over 12 decades
        return r * 10.0 ** rng.uniform(-6, 6, n)
    if kind == "zero":
        return np.zeros(n)
    raise KeyError(kind)


def check_vector(kind, b, g):
    b, g = np.asarray(b, dtype=LD), np.asarray(g, dtype=LD)
    if kind == "generic":
        assert abs(b @ g) > 1e-3 * (np.abs(b) * np.abs(g)).sum()
    if kind == "orthogonal":
        assert abs(b @ g) < 1e-13 * (np.abs(b) * np.abs(g)).sum() and (np.abs(b) * np.abs(g)).sum() > 0
    if kind == "decades":
        a = np.abs(g[g != 0])
        assert a.max() / a.min() > 1e12
    if kind == "zero":
        assert not g.any()


def ranges(n):
    """Entry ranges [j0, j1) of the dots on n entries: j0 odd and no multiple of 7 or 256 (no row, no workgroup
    boundary), ends inside a workgroup and at n, one entry, and empty ranges."""
    out = [(1, n), (3, n - 1), (n - 4, n), (n - 1, n), (5, 5), (n, n)]
    if n > 4 * WG:
        out += [(2 * WG + 1, 3 * WG + 1), (1003, n - 1000)]
    for j0, j1 in out:
        assert 0 <= j0 <= j1 <= n
        if j1 > j0 and j0 != n - 4 and j0 != n - 1:
            assert j0 % 2 == 1 and j0 % 7 and j0 % WG
    assert any(j0 == j1 for j0, j1 in out)
    return out


# span_grid requests on rows_8193 and the class of SpMV partial count each must yield (sum_partials in k_dl_sum and
# k_dl_final: the tail loop alone up to one pass, a second pass, the last count below the unrolled loop, its first
# trips, and more than MAX_GRID)
SPAN_GRIDS = ((100, "<=255"), (256, "256-257"), (257, "256-257"), (1023, "1023"), (1024, "1024-1025"),
              (1025, "1024-1025"), (2049, ">2048"))


def check_span_count(cls, count):
    lo, hi = {"<=255": (8, 255), "256-257": (256, 257), "1023": (1023, 1023), "1024-1025": (1024, 1025),
              ">2048": (MAX_GRID + 1, 65536)}[cls]
    assert lo <= count <= hi, (cls, count)


# ------------------------------------------------------------------------------------------------ update
COEFFS = (("gn", 0.0, 1.0), ("sd", 0.37, 0.0), ("mixed", 0.21, 0.64), ("none", 0.0, 0.0))
STEP_SIZES = (0.3, 1e-7)  # |h| on the generic branch of exp and on its small-angle branch


# ------------------------------------------------------------------------------------------------ the rule's scalars
def scalars_of(b, g, H):
    """The six scalars of vectors b, g and a symmetric H, rounded from long double."""
    b, g, H = (np.asarray(x, dtype=LD) for x in (b, g, H))
    return np.array([b @ b, b @ H @ b, g @ g, b @ g, (H @ b) @ g, g @ H @ g], dtype=np.float64)


H2 = np.array([[1.0, 0.2], [0.2, 2.0]])  # b = (1, 0): b^T H b = b.b = 1, alpha = 1, h_sd = b


def rule_case(name):
    """(scalars, delta) with h_sd = (1, 0) inside the trust region and h_gn = h_sd + d outside it."""
    tiny = 1.0 + 1e-12  # delta^2 - ||h_sd||^2 ~ 2e-12: ||d||^2 d2 is far below c^2, the other form of the root cancels
    d, delta = {"c_neg": ((-3.0, 0.5), 1.5), "c_pos": ((3.0, 0.5), 1.5), "c_neg_cancel": ((-3.0, 0.5), tiny),
                "c_pos_cancel": ((3.0, 0.5), tiny), "c_zero": ((0.0, 2.0), 1.5)}[name]
    b = np.array([1.0, 0.0])
    return scalars_of(b, b + np.array(d), H2), delta


RULE_CASES = ("c_neg", "c_pos", "c_neg_cancel", "c_pos_cancel", "c_zero")


def check_rule_case(name, s, delta):
    """From the inputs alone (long double): a dogleg step, the sign of c, and for *_cancel that the form NOT taken
    subtracts two numbers that agree to more than half of float64's digits."""
    bb, bHb, gg, bg = (LD(x) for x in s[:4])
    alpha = bb / bHb
    hsd2 = alpha * alpha * bb
    assert np.sqrt(gg) >= delta and np.sqrt(hsd2) <= delta  # neither GN nor SD
    c = alpha * bg - hsd2
    bma2 = gg - 2 * alpha * bg + hsd2
    d2 = LD(delta) * LD(delta) - hsd2
    assert (c < 0) if name.startswith("c_neg") else (c > 0) if name.startswith("c_pos") else (c == 0)
    if name.endswith("cancel"):
        root = np.sqrt(c * c + bma2 * d2)
        assert abs(root - abs(c)) < 2.0 ** -27 * abs(c)  # |c| - root (c < 0: c + root) loses more than 26 of 53 bits
    return float(c)
