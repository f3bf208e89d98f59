"""Graphs of the PCG operator tests (tests/test_pcg_ref.py on the host, tests/test_gpu_pcg_operator.py on the device)
and the PATH CONDITIONS they exist for: each case is there because its span table and pattern drive k_spmv_span
through one particular path, and `facts` measures that from a span table and a pattern, so that both tests assert it
instead of assuming it.

  tiny1, tiny3 ....... one free vertex; a chain of three: most spans are empty, the first rows and the last row are
                       handled by single spans far apart.
  m400 ............... Manhattan 400 / 4000: as many spans as rows, none long enough for a refill of the column
                       window or of the row-end table: the baseline.
  hub_first / _mid / _last ... m400 plus one vertex joined to 235 others, 20 of them by two edges, inserted so that
                       its block row is the first, a middle or the last free row: a row of > 192 blocks (three changes
                       of the 64-block column window inside one row), duplicate columns, and -- the span table being
                       balanced by blocks -- empty spans between non-empty ones.
  chain10k ........... chain_loop(10000, 20000); with span_grid = 8 a span holds > 256 rows (four refills of the
                       64-row table of row ends) and > 64 blocks; with span_grid = 2500 the SpMV leaves more partial
                       sums than MAX_GRID.
  m3000 .............. Manhattan 3000 / 30000 with the multigrid preconditioner: the batch buffers exist.  With the
                       automatic table no span of this graph exceeds 60 blocks, so the case sets span_grid = 64:
                       spans of about twelve rows and 250 blocks, the column window changes under K systems too.
"""
import numpy as np

from sim3opt_amd import sim3np as S3, synth

MAX_GRID = 2048  # engine_impl.hpp: partial sums a PCG step adds for itself; above it k_final_sum2 adds them first
HUB_NEIGHBOURS, HUB_DOUBLE = 235, 20

CASES = {  # name -> (graph, options of the Graph)
    "tiny1": ("tiny1", {}),
    "tiny3": ("tiny3", {}),
    "m400": ("m400", {}),
    "hub_first": ("hub_first", {}),
    "hub_mid": ("hub_mid", {}),
    "hub_last": ("hub_last", {}),
    "chain10k_g8": ("chain10k", dict(span_grid=8)),
    "chain10k_g2500": ("chain10k", dict(span_grid=2500)),
    "m3000": ("m3000", dict(preconditioner=2, span_grid=64)),
}


def _with_hub(g, pos, seed=77):
    """g plus one vertex at insertion position `pos` (>= 1: vertex 0 stays the fixed one), joined to HUB_NEIGHBOURS
    other vertices, the first HUB_DOUBLE of them by two edges.  The measurements carry loop-closure noise about the
    current estimates, the new vertex starts at a neighbour's estimate moved by a small step."""
    rng = np.random.default_rng(seed)
    S = np.asarray(g["states"])
    V = S.shape[0]
    others = rng.choice(np.arange(V), size=HUB_NEIGHBOURS, replace=False)
    others = np.concatenate([others, others[:HUB_DOUBLE]])
    hub_state = S3.mul(S3.exp(synth._noise(rng, 1, (0.05, 0.3, 0.02)), fix_b=True), S[others[:1]])[0]
    states = np.insert(S, pos, hub_state, axis=0)
    fixed = np.insert(np.asarray(g["fixed"]), pos, 0)
    shift = lambda v: np.where(np.asarray(v) >= pos, np.asarray(v) + 1, np.asarray(v))
    o = shift(others)
    e0, e1 = np.minimum(o, pos), np.maximum(o, pos)  # (v0 < v1, the generators' loop-edge convention)
    meas = S3.mul(S3.exp(synth._noise(rng, o.shape[0], synth.LOOP_SIGMA), fix_b=True),
                  S3.mul(states[e1], S3.inv(states[e0])))
    return dict(states=states, fixed=fixed.astype(np.uint8),
                v0=np.concatenate([shift(g["v0"]), e0]).astype(np.int32),
                v1=np.concatenate([shift(g["v1"]), e1]).astype(np.int32),
                meas=np.concatenate([g["meas"], meas]), hub_vertex=int(pos))


def graph_of(name):
    synth.DRIFT_TARGET = 0.05
    if name == "tiny1":
        return synth.chain_loop(2, 1)
    if name == "tiny3":
        return synth.chain_loop(4, 3)
    if name == "m400":
        return synth.manhattan(400, 4000, dims=(6, 6, 10))
    if name.startswith("hub_"):
        g = synth.manhattan(400, 4000, dims=(6, 6, 10))
        return _with_hub(g, dict(hub_first=1, hub_mid=200, hub_last=400)[name])
    if name == "chain10k":
        return synth.chain_loop(10000, 20000)
    if name == "m3000":
        return synth.manhattan(3000, 30000, dims=(17, 17, 10))
    raise KeyError(name)


def hub_row(g):
    """Block row of the hub: free vertices in insertion order (vertex 0 is the only fixed one)."""
    return g["hub_vertex"] - 1 if "hub_vertex" in g else None


def facts(rowptr, colidx, wrow, hub=None):
    """What a span table makes of a pattern: spans, empty ones, empty ones strictly between non-empty ones, the most
    rows / blocks of one span, the most blocks of one row; with a hub row its blocks, its duplicate columns and
    whether it ends the matrix."""
    rowptr, colidx, wrow = np.asarray(rowptr), np.asarray(colidx), np.asarray(wrow)
    nb = rowptr.shape[0] - 1
    assert wrow[0] == 0 and wrow[-1] == nb and (np.diff(wrow) >= 0).all()  # every row in exactly one span
    rows = np.diff(wrow)
    blocks = rowptr[wrow[1:]] - rowptr[wrow[:-1]]
    ne = np.flatnonzero(rows > 0)
    f = dict(spans=int(rows.shape[0]), span_grid=int(rows.shape[0]) // 4, empty=int((rows == 0).sum()),
             empty_interior=int((rows[ne[0]:ne[-1] + 1] == 0).sum()), max_rows=int(rows.max()),
             max_blocks=int(blocks.max()), max_row_blocks=int(np.diff(rowptr).max()), nb=int(nb),
             nnzb=int(rowptr[-1]), first_span=int(ne[0]), last_span=int(ne[-1]))
    if hub is not None:
        c = colidx[rowptr[hub]:rowptr[hub + 1]]
        f.update(hub_row=int(hub), hub_blocks=int(c.shape[0]), hub_duplicates=int(c.shape[0] - np.unique(c).shape[0]),
                 hub_ends_matrix=bool(rowptr[hub + 1] == rowptr[-1]))
    return f


def check_path(name, f):
    """The condition case `name` exists for, asserted on facts(...)."""
    if name.startswith("tiny"):
        assert 2 * f["empty"] > f["spans"] and f["max_rows"] == 1 and f["first_span"] > 0, f
        if name == "tiny1":  # the one row is the LAST wavefront's; every workgroup before the last is idle
            assert f["last_span"] == f["spans"] - 1, f
        else:  # empty spans before, between and after the three rows
            assert f["empty_interior"] >= 1 and f["last_span"] < f["spans"] - 1, f
    elif name == "m400":
        # one span per row on average (balanced by blocks: a few spans hold two or three short rows, some none), and
        # no span reaches a refill of the column window or of the row-end table
        assert f["spans"] >= f["nb"] and f["max_blocks"] <= 64 and f["max_rows"] < 64, f
    elif name.startswith("hub_"):
        assert f["hub_blocks"] > 192 and f["hub_duplicates"] >= HUB_DOUBLE and f["empty_interior"] >= 1, f
        assert f["hub_row"] == dict(hub_first=0, hub_mid=199, hub_last=f["nb"] - 1)[name], f
        if name == "hub_last":
            assert f["hub_ends_matrix"], f
    elif name == "chain10k_g8":
        assert f["span_grid"] == 8 and f["max_rows"] > 256 and f["max_blocks"] > 64, f
    elif name == "chain10k_g2500":
        assert f["span_grid"] == 2500 > MAX_GRID, f
    elif name == "m3000":
        assert f["span_grid"] == 64 and f["max_rows"] >= 2 and f["max_blocks"] > 64, f
    else:
        raise KeyError(name)


def describe(name, f):
    keys = ("span_grid", "nb", "nnzb", "max_rows", "max_blocks", "empty", "empty_interior", "hub_row", "hub_blocks",
            "hub_duplicates")
    return f"[pcg-op] {name}: " + ", ".join(f"{k} {f[k]}" for k in keys if k in f)


def rhs_set(b, hub=None, seed=0):
    """(names, vectors): the system's own b, three seeded Gaussian vectors, unit vectors on the first and the last
    column (and on the hub's first column), one vector of alternating sign with magnitudes over twelve decades."""
    rng = np.random.default_rng(seed)
    n = b.shape[0]
    names, vs = ["b"], [np.asarray(b, dtype=np.float64)]
    for k in range(3):
        names.append(f"gauss{k}")
        vs.append(rng.standard_normal(n))
    for nm, j in (("e_first", 0), ("e_last", n - 1)) + ((("e_hub", 7 * hub),) if hub is not None else ()):
        e = np.zeros(n)
        e[j] = 1.0
        names.append(nm)
        vs.append(e)
    names.append("decades")
    vs.append((-1.0) ** np.arange(n) * 10.0 ** rng.uniform(-6, 6, n))
    return names, np.stack(vs)


LAMBDA_REL = (0.0, 1e-7, 1e-3, 1.0)  # dampings relative to max diag(H), as in test_gpu_preconditioners.py
# PCG iterates: case -> damping relative to max diag(H).  m400 as everywhere: 1e-3.  The hub's own diagonal block is
# twenty times the others, so on hub_mid 1e-3 x max diag is a heavy damping, and the chain is so sparse that block-Jacobi
# PCG at 1e-3 converges in 17 iterations: both would have the larger caps compare iterates that no longer move.  1e-5
# and 1e-6 keep the residual above 1e-5 of its start up to the largest cap and let the solve to the end replay the
# captured graph several times (130 and 263 iterations); the GPU test asserts the former with the reference.
ITERATE_CASES = {"m400": 1e-3, "hub_mid": 1e-5, "chain10k_g8": 1e-6, "chain10k_g2500": 1e-6}
ITERATE_FLOOR = 1e-10  # smallest gamma_k / gamma_0 (squared residual ratio) the reference may reach at the largest cap
ITERATE_CAPS = (1, 2, 3, 8, 16, 17, 33, 40)
PCG_REL_TOL = 1e-150  # tol^2 = 1e-300 is a normal double, and no iterate comes near it: the cap stops the solve
