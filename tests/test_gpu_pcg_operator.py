"""GPU tests (-m gpu) of the PCG's own operator and recurrence: q = (H + lambda I) p with its two dot products, as the
SpMV launch of a PCG iteration computes them (k_spmv_span MODE 0, one system and K systems), and the iterates x_k of
k_pcg_init / k_pcg_step are read out of the device (sim3opt_operator_apply, sim3opt_spmv_spans, sim3opt_solve with an
iteration cap) and compared with tests/pcg_ref.py in long double.  A CG with a slightly wrong operator or recurrence
still converges, so the parity tests cannot see a block lost at a window edge, a damping term on the wrong row, a beta
from the wrong parity slot or a replay that runs one step too many; these can (tests/test_pcg_ref.py asserts that each
such defect moves the result by >= 1e4 x the tolerance used here).

Every case comes with the PATH CONDITION it exists for (tests/pcg_cases.py), asserted here on the span table the DEVICE
holds, so that a change of the span rule cannot silently empty a case.

Three kinds of check:
  derived ...... per entry of q, row i with m_i stored blocks: |q_dev - q_ld| <= gamma(7 m_i + 3) (|A||p| + |lambda||p|)_i,
                 gamma(k) = k u / (1 - k u): a sum of 7 m_i products and the damping term, any order, any contraction; the
                 device's blocks are the reference's inputs bit for bit.  Dots: |pq_dev - sum p_i q_dev,i| <=
                 gamma(7 nb + 2) sum |p_i q_dev,i| against the DEVICE's q, likewise r.p.
  exact ........ q does not depend on the SpMV variant (SIM3OPT_SPMV) nor on the span table; system s of a K-system
                 launch is the one-system launch bit for bit; read-outs change nothing; x, iters and rel_res do not depend
                 on pcg_graph / pcg_check_every.
  measured ..... iterates x_k and rel_res: amg_ref.noise_and_tol (32 x |float64 restatement - long double|, floored at
                 4u), the project's convention for kernels with another summation order.  Each case prints noise and the
                 device's ratio (-s); DESIGN.md 5a'' records the table.
"""
import ctypes

import numpy as np
import pytest

from sim3opt_amd import lib as L
import amg_ref as R
import pcg_cases as C
import pcg_ref as P

LD, U = R.LD, R.U
pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not R.longdouble_ok(), reason="np.longdouble has no 64-bit mantissa here")]


@pytest.fixture(autouse=True)
def _no_env_knobs(monkeypatch):
    monkeypatch.delenv("SIM3OPT_SPAN_GRID", raising=False)
    monkeypatch.delenv("SIM3OPT_SPMV", raising=False)


_graphs = {}


def graph(gname):
    if gname not in _graphs:
        _graphs[gname] = C.graph_of(gname)
    return _graphs[gname]


def mk(gname, linearize=True, **opts):
    g = graph(gname)
    o = dict(fix_small_angle_b=1, fd_delta=1e-6, linear_solver=0, preconditioner=0)
    o.update(opts)
    G = L.Graph(**o)
    G.add_vertices(g["states"], g["fixed"])
    G.add_edges(g["v0"], g["v1"], g["meas"])
    G.initialize()
    if linearize:
        G.linearize()
    return G


def mk_case(name, **extra):
    gname, opts = C.CASES[name]
    return mk(gname, **{**opts, **extra}), graph(gname)


def system(G):
    rp, ci, blk, b = G.get_system()
    return dict(rp=rp, ci=ci, blk=blk, b=b, maxdiag=float(np.abs(blk[rp[:-1]].diagonal(0, 1, 2)).max()))


def path_facts(name, G, g, s):
    """facts of the DEVICE's span table on the host's pattern (which must be the device's), condition asserted."""
    rp, ci = G.system_pattern()
    assert np.array_equal(rp, s["rp"]) and np.array_equal(ci, s["ci"])
    f = C.facts(rp, ci, G.spmv_spans(), C.hub_row(g))
    print(C.describe(name, f))
    C.check_path(name, f)
    return f


class Product:
    """A p and |A||p| in long double for a set of vectors, once; q and its bound for any damping from them."""

    def __init__(self, s, ps):
        self.s, self.p = s, np.asarray(ps, dtype=LD)
        self.Ap, self.mag = P.bcsr_apply(s["rp"], s["ci"], s["blk"], 0.0, ps, LD)
        self.g = P.gamma_k(7 * P.blocks_per_row(s["rp"]).astype(LD) + 3)

    def q_ratio(self, i, lam, q_dev):
        """max over the entries of |q_dev - q_ld| / bound (an entry whose bound is 0 must be exact)."""
        q_ld = self.Ap[i] + LD(lam) * self.p[i]
        tol = self.g * (self.mag[i] + LD(lam) * np.abs(self.p[i]))
        err = np.abs(np.asarray(q_dev, dtype=LD) - q_ld)
        assert (err[tol == 0] == 0).all()
        return float((err[tol > 0] / tol[tol > 0]).max()) if (tol > 0).any() else 0.0


def dot_ratio(d_dev, a, b_):
    """|d_dev - sum a_i b_i| / (gamma(n + 2) sum |a_i b_i|), the sum in long double."""
    t = np.asarray(a, dtype=LD) * np.asarray(b_, dtype=LD)
    tol = P.gamma_k(t.shape[0] + 2) * np.abs(t).sum()
    err = abs(LD(d_dev) - t.sum())
    if tol == 0:
        assert err == 0
        return 0.0
    return float(err / tol)


# ------------------------------------------------------------------------------------------------ derived bound
@pytest.mark.parametrize("name", list(C.CASES))
def test_operator_and_dots_within_the_derived_bound(name):
    G, g = mk_case(name)
    s = system(G)
    path_facts(name, G, g, s)
    names, ps = C.rhs_set(s["b"], C.hub_row(g))
    rs = np.roll(ps, 1, axis=0)  # r of p_i: another vector of the set
    ref = Product(s, ps)
    worst_q = worst_d = 0.0
    for lam_rel in C.LAMBDA_REL:
        lam = lam_rel * s["maxdiag"]
        for i, nm in enumerate(names):
            q, pq, rp = G.operator_apply(lam, ps[i], rs[i])
            rq = ref.q_ratio(i, lam, q)
            rd = max(dot_ratio(pq, ps[i], q), dot_ratio(rp, rs[i], ps[i]))
            assert rq <= 1.0 and rd <= 1.0, (name, nm, lam_rel, rq, rd)
            q2, pq2, none = G.operator_apply(lam, ps[i])  # without r: the same q and p.q
            assert none is None and np.array_equal(q2, q) and pq2 == pq
            worst_q, worst_d = max(worst_q, rq), max(worst_d, rd)
    print(f"[pcg-op] {name}: {len(names)} vectors x {len(C.LAMBDA_REL)} dampings; worst q {worst_q:.3f} of its bound, "
          f"worst dot {worst_d:.1e} of its bound")


# ------------------------------------------------------------------------------------------------ exact checks
@pytest.mark.parametrize("gname", ["hub_mid", "chain10k", "m3000"])
def test_q_bits_do_not_depend_on_the_variant_or_the_span_table(gname, monkeypatch):
    """CH = 4 / 8, non-temporal or not, 8 workgroups, the automatic table, one row per wavefront: the same q bit for
    bit (per row the same products in the same order); the dots are sums over other partitions and must meet their
    bound each time.  That the knob was honoured is read back from the engine (spmv_variant), as the span tables are."""
    nb = None
    base = None
    seen, variants = set(), set()
    for variant in ("8,1", "4,0", "4,1", "8,0"):
        monkeypatch.setenv("SIM3OPT_SPMV", variant)
        for grid in ("auto", 8, "largest"):
            sg = 0 if grid == "auto" else (8 if grid == 8 else (nb + 3) // 4)
            G = mk(gname, span_grid=sg)
            assert G.spmv_variant() == tuple(int(c) for c in variant.split(",")), (variant, G.spmv_variant())
            variants.add(G.spmv_variant())
            s = system(G)
            nb = s["rp"].shape[0] - 1
            spans = G.spmv_spans()
            seen.add(spans.shape[0] - 1)
            names, ps = C.rhs_set(s["b"], C.hub_row(graph(gname)))
            out = []
            for i in (0, 1, len(names) - 1):
                for lam_rel in (0.0, 1e-3):
                    q, pq, rp = G.operator_apply(lam_rel * s["maxdiag"], ps[i], ps[i - 1])
                    assert dot_ratio(pq, ps[i], q) <= 1.0 and dot_ratio(rp, ps[i - 1], ps[i]) <= 1.0
                    out.append(q)
            if base is None:
                base = out
            for a, b_ in zip(base, out):
                assert np.array_equal(a, b_), (gname, variant, grid)
            G.close()
    assert len(seen) >= 2 and len(variants) == 4, (seen, variants)  # (the tables and the instantiations did differ)
    print(f"[pcg-op] {gname}: q bit-identical over 4 variants x span tables of {sorted(seen)} spans")


def test_systems_of_a_batch_equal_the_one_system_launches():
    """K = 2, 3, 4 systems with distinct dampings and vectors through the batch's launch (K > 1: the shuffles, per-system
    damping from the batch's scalars) against K one-system launches (the LDS copy, damping from the solver's scalars):
    q, p.q and r.p bit for bit."""
    name = "m3000"
    G, g = mk_case(name)
    assert G.preconditioner_in_use() == 2
    s = system(G)
    path_facts(name, G, g, s)
    names, ps = C.rhs_set(s["b"])
    rs = np.roll(ps, 2, axis=0)
    lams = np.array([1e-3, 1e-7, 1.0, 0.0]) * s["maxdiag"]
    for K, first in ((2, 0), (3, 2), (4, 3), (4, 0)):
        idx = [(first + k) % len(names) for k in range(K)]
        q, pq, rp = G.operator_apply(lams[:K], ps[idx], rs[idx])
        qn, pqn, none = G.operator_apply(lams[:K], ps[idx])
        assert none is None and np.array_equal(qn, q) and np.array_equal(pqn, pq)
        for k, i in enumerate(idx):
            q1, pq1, rp1 = G.operator_apply(lams[k], ps[i], rs[i])
            assert np.array_equal(q1, q[k]) and pq1 == pq[k] and rp1 == rp[k], (K, k, names[i])
    print(f"[pcg-op] {name}: systems of K = 2, 3, 4 launches equal the one-system launches bit for bit")


def test_span_grid_option_is_used_and_reported(monkeypatch):
    """options.span_grid without any environment variable: 8 workgroups = 32 spans; 0 = the automatic table; the
    clamps; the environment variable overrides the field; get_options reports what was used."""
    def spans_of(gname, **o):
        G = mk(gname, linearize=False, **o)
        assert G.spmv_variant() == (8, 1)  # (no SIM3OPT_SPMV: the default instantiation)
        w, used = G.spmv_spans(), G.options().span_grid
        rp, _ = G.system_pattern()
        assert np.array_equal(w, L.partition_rows(rp, w.shape[0] - 1))  # balanced by blocks, whatever the count
        G.close()
        return w.shape[0] - 1, used

    assert spans_of("m400", span_grid=8) == (32, 8)
    assert spans_of("m400") == (400, 0) and spans_of("m400", span_grid=0) == (400, 0)   # 399 rows: 100 workgroups
    assert spans_of("chain10k") == (8192, 0)                                             # 9999 rows: 2048 workgroups
    assert spans_of("m400", span_grid=5) == (32, 8) and spans_of("m400", span_grid=10 ** 6) == (400, 100)
    assert spans_of("chain10k", span_grid=2500) == (10000, 2500)
    # the request is kept apart from the value in use: clamped anew when the graph has grown and is initialised again,
    # also after a get / set round trip of the options (set_options reads them, changes one field and writes them back)
    g = graph("m400")
    G = mk("m400", linearize=False, span_grid=10 ** 6)
    assert (G.spmv_spans().shape[0] - 1, G.options().span_grid) == (400, 100)
    G.set_options(pcg_max_iters=7)
    more = 400 + np.arange(12)
    G.add_vertices(np.asarray(g["states"])[-12:], np.zeros(12, dtype=np.uint8), ids=more)
    G.add_edges(np.r_[399, more[:-1]].astype(np.int32), more.astype(np.int32), np.asarray(g["meas"])[:12])
    G.initialize()
    assert (G.spmv_spans().shape[0] - 1, G.options().span_grid) == (412, 103)  # 411 rows: (411 + 3) / 4 workgroups
    assert G.options().pcg_max_iters == 7
    G.set_options(span_grid=8)
    G.initialize()
    assert (G.spmv_spans().shape[0] - 1, G.options().span_grid) == (32, 8)
    G.close()
    monkeypatch.setenv("SIM3OPT_SPAN_GRID", "16")
    assert spans_of("m400", span_grid=8) == (64, 16) and spans_of("m400") == (64, 16)


def test_operator_readouts_refuse_what_they_cannot_do():
    G = mk("m400", linearize=False)
    b = np.ones(7 * 399)
    with pytest.raises(L.Sim3OptError) as e:
        G.operator_apply(1.0, b)  # no linearisation yet
    assert e.value.code == L.ERR_STATE
    assert G.spmv_spans().shape[0] == 401  # (the table exists from initialize on)
    G.linearize()
    with pytest.raises(L.Sim3OptError) as e:
        G.operator_apply([1.0, 2.0], np.stack([b, b]))  # no batch buffers without the multigrid preconditioner
    assert e.value.code == L.ERR_STATE
    with pytest.raises(L.Sim3OptError) as e:
        G.operator_apply(-1.0, b)
    assert e.value.code == L.ERR_ARG
    with pytest.raises(L.Sim3OptError) as e:
        G.operator_apply(np.ones(5), np.stack([b] * 5))
    assert e.value.code == L.ERR_ARG
    dp = ctypes.POINTER(ctypes.c_double)
    lam, q, pq = np.ones(1), np.zeros_like(b), np.zeros(1)
    a = lambda v: v.ctypes.data_as(dp)
    assert G._L.sim3opt_operator_apply(G._g, 1, a(lam), a(b), a(b), a(q), a(pq), None) == L.ERR_ARG  # r without rp
    assert G._L.sim3opt_operator_apply(G._g, 1, a(lam), a(b), None, a(q), a(pq), a(pq)) == L.ERR_ARG  # rp without r
    assert G._L.sim3opt_operator_apply(G._g, 1, a(lam), a(b), None, a(q), a(pq), None) == L.OK


def _stats_tuple(G):  # (without the phase times: measured on graphs of more than 4096 rows)
    return [tuple(getattr(s, f) for f, _ in s._fields_ if not f.startswith("ms_")) for s in G.stats()]


@pytest.mark.parametrize("gname,prec", [("m400", 0), ("m3000", 2), ("chain10k", 0)])
def test_operator_readouts_change_nothing(gname, prec):
    """solve and optimize(3) with operator_apply (one and, on the multigrid graph, three systems) and spmv_spans
    interleaved are bit-identical to a fresh graph without them: estimates, stats(), x, iters, rel_res, and the
    counters of kernel_times().  On the multigrid graph the run is the one of
    test_batched_rejected_trials_equal_sequential_solves (delta = 1e-9, 30 iterations: LM rejects trials in bursts),
    and it is asserted that trial solves were batched after the read-outs had used the batch's scalars and buffers."""
    iters = 30 if prec == 2 else 3
    o = dict(fd_delta=1e-9, pcg_rel_tol=1e-8) if prec == 2 else {}

    def run(diag):
        G = mk(gname, preconditioner=prec, **o)
        assert G.preconditioner_in_use() == prec and G.options().pcg_graph == 1
        s = system(G)
        lam = 1e-3 * s["maxdiag"]
        _, ps = C.rhs_set(s["b"])

        def poke(k):
            if not diag:
                return
            G.operator_apply(lam * 10.0 ** k, ps[1], ps[2])
            G.spmv_spans()
            if prec == 2:
                G.operator_apply(lam * np.array([1.0, 3.0, 9.0]), ps[1:4], ps[2:5])
            G.operator_apply(0.0, ps[-1])
        poke(1)
        x1, it1, rr1 = G.solve(lam)
        poke(-2)
        x2, it2, rr2 = G.solve(10 * lam)
        poke(0)
        n_it = G.optimize(iters)
        assert n_it == iters if iters == 3 else n_it >= 3
        assert prec != 2 or G.kernel_times().n_batches >= 1
        poke(2)
        v = G.get_vertices()
        G.linearize()
        poke(-1)
        x3, it3, rr3 = G.solve(lam)
        kt = G.kernel_times()
        counts = tuple(getattr(kt, f) for f, _ in kt._fields_ if f.startswith("n_"))
        return (x1, x2, x3, v), (it1, it2, it3, rr1, rr2, rr3, n_it), _stats_tuple(G), counts

    a, b_ = run(False), run(True)
    for u, v in zip(a[0], b_[0]):
        assert np.array_equal(u, v)
    assert a[1] == b_[1] and a[2] == b_[2] and a[3] == b_[3]
    print(f"[pcg-op] read-outs change nothing, {gname} prec {prec}: PCG iterations {a[1][:3]}, counters {a[3]}")


# ------------------------------------------------------------------------------------------------ PCG iterates
_ref_runs = {}


def reference_iterates(gname, s, lam):
    """Long-double and float64 restatements up to the largest cap, once per system (the two chain cases share theirs)."""
    key = (gname, float(lam))
    if key not in _ref_runs:
        a = (s["rp"], s["ci"], s["blk"], s["b"], lam, max(C.ITERATE_CAPS), C.PCG_REL_TOL)
        _ref_runs[key] = (P.pcg(*a, LD), P.pcg(*a, np.float64), s["blk"].copy())
    ld, f64, blk = _ref_runs[key]
    assert np.array_equal(blk, s["blk"])  # (the span table does not touch the assembly)
    return ld, f64


@pytest.mark.parametrize("name", list(C.ITERATE_CASES))
def test_pcg_iterates_match_the_recurrence(name):
    G, g = mk_case(name, pcg_rel_tol=C.PCG_REL_TOL)
    s = system(G)
    path_facts(name, G, g, s)
    lam = C.ITERATE_CASES[name] * s["maxdiag"]
    ld, f64 = reference_iterates(C.CASES[name][0], s, lam)
    gam = np.array(ld["gamma"], dtype=LD)
    # the cap stops every solve, not the tolerance (reference alone); tol^2 is a normal double
    assert ld["iters"] == max(C.ITERATE_CAPS) and (gam / gam[0] > LD(C.PCG_REL_TOL) ** 2).all()
    assert gam[-1] / gam[0] > C.ITERATE_FLOOR  # ... and every compared iterate still moves (pcg_cases.ITERATE_CASES)
    assert C.PCG_REL_TOL ** 2 > np.finfo(np.float64).tiny
    for k in C.ITERATE_CAPS:
        G.set_options(pcg_max_iters=k)
        x, it, rr = G.solve(lam)
        assert it == k, (name, k, it)
        nx, tx = R.noise_and_tol(f64["x"][k - 1], ld["x"][k - 1])
        ex = R.relerr(x, ld["x"][k - 1])
        rel_ld = np.sqrt(gam[k - 1] / gam[0])
        rel_64 = np.sqrt(f64["gamma"][k - 1] / f64["gamma"][0])
        nr, tr = R.noise_and_tol(np.array([rel_64]), np.array([rel_ld]))
        er = R.relerr(np.array([rr]), np.array([rel_ld]))
        print(f"[pcg-op] {name} k {k:2d}: x_k noise {nx:.2e} device {ex:.2e} = {ex / nx:5.2f} x noise; rel_res "
              f"{float(rel_ld):.3e} noise {nr:.2e} device {er:.2e} = {er / nr:5.2f} x noise (limit 32)")
        assert ex <= tx and er <= tr, (name, k, nx, ex, nr, er)


@pytest.mark.parametrize("name", list(C.ITERATE_CASES))
def test_launch_mechanics_do_not_change_a_bit(name):
    """Captured-graph replay or eager launches, the host polling every 1, 5 or 16 iterations: the same kernels in the
    same order, so x, iters and rel_res are identical -- for caps just past one and two replays (17, 33), a cap that
    ends in eager steps after two replays (40) and a solve run to its end; two solves in a row with different dampings
    on ONE graph object (the instantiated graph is reused and reads the damping from the device's scalars)."""
    G, g = mk_case(name)
    s = system(G)
    lam = C.ITERATE_CASES[name] * s["maxdiag"]
    base = {}
    for pcg_graph in (0, 1):
        for every in (1, 5, 16):
            for cap in (17, 33, 40, 0):
                G.set_options(pcg_graph=pcg_graph, pcg_check_every=every, pcg_max_iters=cap,
                              pcg_rel_tol=C.PCG_REL_TOL if cap else 1e-10)
                got = [G.solve(lam), G.solve(3.0 * lam)]
                if cap:
                    assert got[0][1] == cap and got[1][1] == cap
                if cap not in base:
                    base[cap] = got
                for (x, it, rr), (x0, it0, rr0) in zip(got, base[cap]):
                    assert it == it0 and rr == rr0 and np.array_equal(x, x0), (name, pcg_graph, every, cap, it, it0)
    print(f"[pcg-op] {name}: pcg_graph x pcg_check_every bit-identical; solves to the end took "
          f"{base[0][0][1]} and {base[0][1][1]} iterations (rel_res {base[0][0][2]:.2e}, {base[0][1][2]:.2e})")
