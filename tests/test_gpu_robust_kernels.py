"""Robust kernels beyond Huber on the GPU (-m gpu).  The CPU oracle knows Huber only, but a first-order kernel is
a per-edge rescaling of the information: edge k with weight w_k = rho'(e_k^T Omega_k e_k) linearises exactly as a
kernel-free edge with information w_k Omega_k, and contributes rho(e_k^T Omega_k e_k) to chi2.  So chi2, H, b and
the first LM step are checked against the unchanged oracle with the rescaled information; changing kernels after
initialize against a graph built with them; and the point of the feature -- rejecting false loop closures --
on a chain with corrupted loops."""
import os
import subprocess

import numpy as np
import pytest
import torch.multiprocessing as mp

from oracle import oracle as O
from sim3opt_amd import lib as L, sim3np as S3, synth
import dist_helpers as H

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = np.arange(10)


def rho_w(kinds, deltas, e2):
    """numpy restatement of the kernel table (include/sim3opt.h), vectorised over edges."""
    rho, w = np.empty_like(e2), np.empty_like(e2)
    for k, (kind, d, x) in enumerate(zip(kinds, deltas, e2)):
        d2 = d * d
        if kind == L.KERNEL_NONE:
            r = (x, 1.0)
        elif kind == L.KERNEL_HUBER:
            r = (x, 1.0) if x <= d2 else (2 * np.sqrt(x) * d - d2, d / np.sqrt(x))
        elif kind == L.KERNEL_PSEUDO_HUBER:
            a = np.sqrt(1 + x / d2)
            r = (2 * d2 * (a - 1), 1 / a)
        elif kind == L.KERNEL_CAUCHY:
            r = (d2 * np.log1p(x / d2), 1 / (1 + x / d2))
        elif kind == L.KERNEL_GEMAN_MCCLURE:
            r = (d * x / (d + x), d2 / (d + x) ** 2)
        elif kind == L.KERNEL_WELSCH:
            r = (d2 * (1 - np.exp(-x / d2)), np.exp(-x / d2))
        elif kind == L.KERNEL_FAIR:
            a = np.sqrt(x) / d
            r = (2 * d2 * (a - np.log1p(a)), 1 / (1 + a))
        elif kind == L.KERNEL_TUKEY:
            r = (d2 / 3 * (1 - (1 - x / d2) ** 3), (1 - x / d2) ** 2) if x <= d2 else (d2 / 3, 0.0)
        elif kind == L.KERNEL_SATURATED:
            r = (x, 1.0) if x <= d2 else (d2, 0.0)
        else:  # DCS
            s = 2 * d / (d + x)
            r = (x, 1.0) if s >= 1 else (s * s * x, s * s)
        rho[k], w[k] = r
    return rho, w


def spd_info(m, seed):
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((m, 7, 7)) * 0.3
    return np.einsum("kij,klj->kil", M, M) + np.eye(7)


def mixed_graph(V=600, E=1000, seed=5):
    """A chain-loop graph off its dead-reckoning start (every residual non-zero), dense information, all ten kinds
    mixed over the edges, each edge's delta placed so that its e2 sits a factor 4 below or above the kink."""
    synth.DRIFT_TARGET = 0.05
    g = synth.chain_loop(V, E, seed_graph=700 + seed, seed_noise=800 + seed, min_gap=20)
    rng = np.random.default_rng(seed)
    xi = np.concatenate([rng.standard_normal((V, 3)) * 0.01, rng.standard_normal((V, 3)) * 0.05,
                         rng.standard_normal((V, 1)) * 0.01], axis=1)
    g["states"] = S3.mul(S3.exp(xi, fix_b=True), g["states"])
    g["states"][0] = g["gt"][0]
    m = g["v0"].shape[0]
    g["info"] = spd_info(m, seed)
    e = oracle_of(g).errors(O.default_options())
    e2 = np.einsum("ki,kij,kj->k", e, g["info"], e)
    assert e2.min() > 0
    kinds = np.resize(KINDS, m)
    rng.shuffle(kinds)
    f = np.where(rng.random(m) < 0.5, 0.25, 4.0)  # e2 / d^2 (or e2 / d for DCS, whose kink is e2 = d)
    deltas = np.where(kinds == L.KERNEL_DCS, e2 / f, np.sqrt(e2 / f))
    deltas[kinds == L.KERNEL_NONE] = 0.0
    g["kinds"], g["deltas"], g["e2"] = kinds.astype(np.int32), deltas, e2
    return g


def oracle_of(g, info=None):
    inf = g.get("info") if info is None else info
    inf = None if inf is None else np.asarray(inf).transpose(0, 2, 1).reshape(-1, 49)
    return O.Graph(g["states"], g["fixed"], g["v0"], g["v1"], g["meas"], info=inf)


def mk(g, kinds=None, deltas=None, init=True, **opts):
    G = L.Graph(**opts)
    G.add_vertices(g["states"], g["fixed"])
    if kinds is None:
        G.add_edges(g["v0"], g["v1"], g["meas"], info=g.get("info"))
    else:
        G.add_edges(g["v0"], g["v1"], g["meas"], info=g.get("info"), kernel=kinds, kernel_delta=deltas)
    if init:
        G.initialize()
    return G


def expected(g, opt):
    """rho, w at the graph's states, and the oracle with information w_k Omega_k."""
    e = oracle_of(g).errors(opt)
    e2 = np.einsum("ki,kij,kj->k", e, g["info"], e)
    rho, w = rho_w(g["kinds"], g["deltas"], e2)
    return e2, rho, w, oracle_of(g, info=g["info"] * w[:, None, None])


@pytest.mark.parametrize("mode", ["fd1e-9", "fd1e-6", "analytic"])
def test_mixed_kernels_chi2_and_system_match_rescaled_oracle(mode):
    g = mixed_graph()
    # (the oracle's Jacobians are central differences: of the same step for the numeric modes, of 1e-6 for the
    # closed form -- whose b then differs from the oracle's by the differences' noise, 4e-7 of max |b| on this
    # graph's long loops; the rescaled kernel-free graph on the device below is the tight check)
    opts, tol = {"fd1e-9": (dict(fd_delta=1e-9), 2e-4), "fd1e-6": (dict(fd_delta=1e-6), 1e-7),
                 "analytic": (dict(jacobians=1, fix_small_angle_b=1), 2e-6)}[mode]
    ofd = dict(fd_delta=opts.get("fd_delta", 1e-6), fix_small_angle_b=opts.get("fix_small_angle_b", 0))
    o = O.default_options(**ofd)
    e2, rho, w, OW = expected(g, o)
    kink = np.where(g["kinds"] == L.KERNEL_DCS, g["deltas"], g["deltas"] ** 2)
    assert np.all(np.abs(e2 - kink) > 1e-6 * kink)
    assert (w < 1).sum() > 0.3 * len(w) and (w == 0).sum() > 0  # (Tukey / Saturated above the kink)
    G = mk(g, g["kinds"], g["deltas"], **opts)
    chi = G.chi2()
    assert abs(chi - rho.sum()) < 1e-10 * rho.sum()
    G.linearize()
    Hg, bg = G.dense_system()
    Ho, bo = OW.build_dense(o)
    assert np.abs(Hg - Hg.T).max() == 0.0
    assert np.abs(Hg - Ho).max() < tol * np.abs(Ho).max()
    assert np.abs(bg - bo).max() < tol * max(1.0, np.abs(bo).max())
    # the same device arithmetic with information w_k Omega_k and no kernel: equal up to where w rounds
    gw = dict(g, info=g["info"] * w[:, None, None])
    GW = mk(gw, **opts)
    GW.linearize()
    Hw, bw = GW.dense_system()
    assert np.abs(Hg - Hw).max() < 1e-12 * np.abs(Hw).max()
    assert np.abs(bg - bw).max() < 1e-12 * max(1.0, np.abs(bw).max())
    # per-edge readback
    c, r, ww = G.edge_chi2()
    assert np.allclose(c, e2, rtol=1e-10, atol=0)
    assert np.allclose(r, rho, rtol=1e-10, atol=1e-300)
    assert np.allclose(ww, w, rtol=1e-9, atol=1e-300)
    assert abs(r.sum() - chi) < 1e-12 * chi


def test_kernels_set_after_initialize_match_a_graph_built_with_them():
    g = mixed_graph(seed=6)
    opts = dict(fd_delta=1e-6)

    def snapshot(G):
        chi = G.chi2()
        G.linearize()
        _, _, blocks, b = G.get_system()
        return chi, blocks, b

    def same(a, b):
        return a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])

    built = mk(g, g["kinds"], g["deltas"], **opts)
    ref = snapshot(built)
    # a graph initialised without any kernel
    late = mk(g, **opts)
    plain = snapshot(late)
    late.set_edge_kernels(None, g["kinds"], g["deltas"])
    assert same(snapshot(late), ref)
    assert np.array_equal(late.edge_kernels()[0], g["kinds"])
    # kinds changed mid-run: equal to a graph built with the new kinds
    kinds2 = np.roll(g["kinds"], 3)
    deltas2 = np.where(kinds2 == L.KERNEL_NONE, 0.0, np.roll(g["deltas"], 3) + 0.01)
    sel = np.nonzero(kinds2 != g["kinds"])[0]
    late.set_edge_kernels(sel, kinds2[sel], deltas2[sel])
    late.set_edge_kernels(np.arange(len(kinds2)), kinds2, deltas2)
    built2 = mk(g, kinds2, deltas2, **opts)
    assert same(snapshot(late), snapshot(built2))
    # and the LM from equal states
    n1, n2 = late.optimize(10), built2.optimize(10)
    assert n1 == n2
    assert abs(late.chi2() - built2.chi2()) <= 1e-12 * built2.chi2()
    assert np.abs(late.get_vertices() - built2.get_vertices()).max() < 1e-9
    # everything back to NONE: the kernel-free graph's bits
    late.set_vertices(g["states"])
    late.set_edge_kernels(None, np.zeros(len(kinds2), np.int32), np.zeros(len(kinds2)))
    assert same(snapshot(late), plain)
    kf = mk(g, **opts)
    assert same(snapshot(kf), plain)
    n1, n2 = late.optimize(10), kf.optimize(10)
    assert n1 == n2 and abs(late.chi2() - kf.chi2()) <= 1e-12 * kf.chi2()


@pytest.mark.parametrize("linear_solver", [1, 0])
def test_first_lm_step_matches_rescaled_oracle(linear_solver):
    g = mixed_graph(seed=7)
    o = O.default_options(fd_delta=1e-6)
    _, _, _, OW = expected(g, o)
    G = mk(g, g["kinds"], g["deltas"], fd_delta=1e-6, pcg_rel_tol=1e-12, linear_solver=linear_solver)
    G.linearize()
    Hg, _ = G.dense_system()
    lam = 1e-5 * np.abs(np.diag(Hg)).max()
    x, _, _ = G.solve(lam)
    ok, xo, _ = OW.solve_once(lam, o)
    assert ok and np.abs(x - xo).max() < 1e-5 * np.abs(xo).max()


def corrupted_chain(V=2000, E=3000, frac=0.03, seed=11):
    """A chain with loops whose start is a front end's estimate (ground truth off by small per-vertex noise);
    a seeded `frac` of its loop measurements replaced by random Sim(3)s.  (CPU oracle, no kernel, 30 LM iterations:
    RMSE vs gt 0.164 on the clean graph, 1.1e3 with the corrupted loops; clean inlier loops' e2: 99th percentile
    0.077, maximum 0.22.)"""
    synth.DRIFT_TARGET = 0.05
    g = synth.chain_loop(V, E, seed_graph=900 + seed, seed_noise=1000 + seed)
    rng = np.random.default_rng(seed)
    xi = np.concatenate([rng.standard_normal((V, 3)) * 0.01, rng.standard_normal((V, 3)) * 0.1,
                         rng.standard_normal((V, 1)) * 0.01], axis=1)
    g["states"] = S3.mul(S3.exp(xi, fix_b=True), g["gt"])
    g["states"][0] = g["gt"][0]
    nl = g["n_loop"]
    bad = np.sort(rng.choice(nl, int(round(frac * nl)), replace=False))
    q = rng.standard_normal((bad.size, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    t = rng.uniform(-20, 20, (bad.size, 3))
    s = np.exp(rng.uniform(-0.5, 0.5, bad.size))
    g["clean_meas"] = g["meas"].copy()
    g["meas"] = g["meas"].copy()
    g["meas"][bad] = np.concatenate([q, t, s[:, None]], axis=1)
    g["bad"] = bad
    return g


def run_lm(g, meas, kind=L.KERNEL_NONE, delta=0.0, iters=30):
    G = L.Graph()
    G.add_vertices(g["states"], g["fixed"])
    G.add_edges(g["v0"], g["v1"], meas)
    nl = g["n_loop"]
    if kind != L.KERNEL_NONE:
        G.set_edge_kernels(np.arange(nl), kind, delta)  # the loop edges (synth puts them first)
    G.initialize()
    G.optimize(iters)
    return G, synth.rmse(G.get_vertices(), g["gt"])


def test_redescending_kernels_reject_false_loops():
    g = corrupted_chain()
    nl = g["n_loop"]
    inl = np.setdiff1d(np.arange(nl), g["bad"])
    _, clean = run_lm(g, g["clean_meas"])
    _, plain = run_lm(g, g["meas"])
    res = {}
    # Observed on an MI355X (30 iterations): clean 0.164, no kernel 1.1e3; Cauchy 1.0: 0.169, max outlier w
    # 1.5e-4, every inlier above 0.5; DCS 10: 0.169, max outlier w 8.4e-6, every inlier above 0.5.  (DCS with
    # Phi = 1 rejects the inliers too from this start -- its long loops begin with e2 in the tens -- and LM stops
    # after 13 iterations with a third of them above 0.5; Cauchy 0.5 keeps 99.2 %.)
    for name, kind, delta in (("cauchy", L.KERNEL_CAUCHY, 1.0), ("dcs", L.KERNEL_DCS, 10.0)):
        G, rm = run_lm(g, g["meas"], kind, delta)
        _, _, w = G.edge_chi2()
        res[name] = (rm, w[g["bad"]].max(), (w[inl] > 0.5).mean())
    print(f"\nRMSE vs gt: clean {clean:.4g}, corrupted without kernel {plain:.4g}, "
          + ", ".join(f"{k} {v[0]:.4g} (max outlier w {v[1]:.3g}, inliers w > 0.5: {v[2]:.4f})" for k, v in res.items()))
    assert plain >= 10 * clean
    for rm, wbad, winl in res.values():
        assert rm <= 2 * clean
        assert wbad < 0.05
        assert winl >= 0.99


def _rank_worker(rank, world, port, out):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import dist_helpers as D
    D.init(rank, world, port)
    g = mixed_graph(V=400, E=700, seed=8)
    G = L.Graph(fix_small_angle_b=1, fd_delta=1e-6, pcg_rel_tol=1e-12)
    G.add_vertices(g["states"], g["fixed"])
    G.add_edges(g["v0"], g["v1"], g["meas"], info=g["info"])
    D.attach(G, rank, world)
    G.initialize()
    G.set_edge_kernels(None, g["kinds"], g["deltas"])  # every rank makes the same call
    chi = G.chi2()
    G.linearize()
    rowptr, colidx, blocks, b = G.get_system()
    lo, hi = G.local_rows()
    c, r, w = G.edge_chi2()
    np.savez(out + f".{rank}.npz", chi=chi, rowptr=rowptr, colidx=colidx, blocks=blocks, b=b, rows=[lo, hi],
             c=c, r=r, w=w)
    D.finish()


def test_partitioned_kernels_set_after_initialize_match_single(tmp_path):
    import socket
    out, world = str(tmp_path / "r"), 2

    def port():
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            return s.getsockname()[1]

    H.spawn_with_port_retry(lambda: mp.spawn(_rank_worker, args=(world, port(), out), nprocs=world, join=True))
    res = [np.load(out + f".{r}.npz") for r in range(world)]
    g = mixed_graph(V=400, E=700, seed=8)
    G = mk(g, g["kinds"], g["deltas"], fix_small_angle_b=1, fd_delta=1e-6, pcg_rel_tol=1e-12, row_order=1)
    chi = G.chi2()
    G.linearize()
    rowptr, colidx, blocks, b = G.get_system()
    c, r, w = G.edge_chi2()
    for x in res:
        assert abs(float(x["chi"]) - chi) <= 1e-12 * chi
        assert np.array_equal(x["rowptr"], rowptr) and np.array_equal(x["colidx"], colidx)
        lo, hi = x["rows"]
        k0, k1 = rowptr[lo], rowptr[hi]
        assert np.allclose(x["blocks"][k0:k1], blocks[k0:k1], rtol=0, atol=1e-12 * np.abs(blocks).max())
        assert np.allclose(x["b"][7 * lo:7 * hi], b[7 * lo:7 * hi], rtol=0, atol=1e-12 * np.abs(b).max())
        assert np.array_equal(x["c"], c) and np.array_equal(x["r"], r) and np.array_equal(x["w"], w)
    assert res[0]["rows"][1] == res[1]["rows"][0] and res[1]["rows"][1] == rowptr.shape[0] - 1


def test_robust_shim_matches_the_c_abi(tmp_path):
    exe = str(tmp_path / "robust_conformance")
    libdir = os.path.join(ROOT, "sim3opt_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-DSIM3OPT_G2O_NAMES",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "mock_eigen"),
                           os.path.join(ROOT, "tests", "cxx", "robust_conformance.cpp"), "-L" + libdir,
                           "-lsim3opt", "-Wl,-rpath," + libdir, "-o", exe])
    r = subprocess.run([exe, "gpu"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout and "robust chi2" in r.stdout
