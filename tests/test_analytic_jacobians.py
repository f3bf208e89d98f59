"""CPU tests of the closed-form Sim(3) edge Jacobians (options.jacobians = 1, csrc/sim3_jac.hpp) through the host
entry sim3opt_sim3_edge_jacobian: against finite differences of scipy's expm / logm on 4x4 similarity matrices (no
code shared with the library), the Lie-group identities of J_l against a high-precision series, the library's own
residual (with the band where its log switches to theta = 0 coefficients), dof_mask, and the option's checks."""
import mpmath as mp
import numpy as np
import pytest
import scipy.linalg as sl

from sim3opt_amd import lib as L, sim3np as S3

I8 = np.array([0, 0, 0, 1, 0, 0, 0, 1.0])


def hat(x):
    M = np.zeros((4, 4))
    w = x[:3]
    M[:3, :3] = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) + x[6] * np.eye(3)
    M[:3, 3] = x[3:6]
    return M


def vee(M):
    return np.array([M[2, 1], M[0, 2], M[1, 0], M[0, 3], M[1, 3], M[2, 3], np.trace(M[:3, :3]) / 3])


def mat(S):
    M = np.eye(4)
    M[:3, :3] = S[7] * S3.quat_to_R(S[:4])
    M[:3, 3] = S[4:7]
    return M


def err_expm(C, A, B):
    return vee(np.real(sl.logm(C @ A @ np.linalg.inv(B))))


def fd_expm(Cm, S0, S1, h=1e-4):
    """five-point central differences of logm(C exp(d0) S0 (exp(d1) S1)^-1)"""
    Cq, A, B = mat(Cm), mat(S0), mat(S1)
    J = np.zeros((7, 14))
    for d in range(7):
        P = {}
        for k in (-2, -1, 1, 2):
            x = np.zeros(7)
            x[d] = k * h
            P[k] = sl.expm(hat(x))
        for off, f in ((0, lambda Q: err_expm(Cq, Q @ A, B)), (7, lambda Q: err_expm(Cq, A, Q @ B))):
            J[:, off + d] = (8 * (f(P[1]) - f(P[-1])) - (f(P[2]) - f(P[-2]))) / (12 * h)
    return J


def rand_sim3(rng, theta, upsilon, sigma):
    w = rng.standard_normal(3)
    u = rng.standard_normal(3)
    w *= theta / np.linalg.norm(w)
    u *= upsilon / np.linalg.norm(u)
    return S3.exp(np.concatenate([w, u, [sigma]]), fix_b=1)


def ad(x):
    """ad_xi of sim(3), tangent order [omega, upsilon, sigma]"""
    def skew(v):
        return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    A = np.zeros((7, 7))
    A[:3, :3] = skew(x[:3])
    A[3:6, :3] = skew(x[3:6])
    A[3:6, 3:6] = skew(x[:3]) + x[6] * np.eye(3)
    A[3:6, 6] = -x[3:6]
    return A


def left_jacobian_mp(x, dps=40):
    """J_l(xi) = sum ad^n / (n+1)! = top-right block of expm([[ad, I], [0, 0]]), in 40-digit arithmetic"""
    with mp.workdps(dps):
        Z = mp.zeros(14, 14)
        a = ad(np.asarray(x, dtype=np.float64))
        for i in range(7):
            Z[i, 7 + i] = 1
            for j in range(7):
                Z[i, j] = mp.mpf(float(a[i, j]))
        E = mp.expm(Z)
        return np.array([[float(E[i, 7 + j]) for j in range(7)] for i in range(7)])


def adjoint_np(S):
    R, t, s = S3.quat_to_R(S[:4]), S[4:7], S[7]
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    A = np.zeros((7, 7))
    A[:3, :3] = R
    A[3:6, :3] = tx @ R
    A[3:6, 3:6] = s * R
    A[3:6, 6] = -t
    A[6, 6] = 1
    return A


def left_jacobian_via_host(xi):
    """J_l(e) and J_l(-e) from the host entry with C = I, S1 = I, S0 = exp(xi): J0 = J_l(e)^-1, J1 = -J_l(-e)^-1"""
    S0 = S3.exp(np.asarray(xi, dtype=np.float64), fix_b=1)
    e, J = L.edge_jacobian_host(I8, S0, I8)
    return e, np.linalg.inv(J[:, :7]), -np.linalg.inv(J[:, 7:])


def test_against_expm_logm_finite_differences():
    rng = np.random.default_rng(7)
    cases = []
    for _ in range(14):
        cases.append((rand_sim3(rng, rng.uniform(0, 3.0), rng.uniform(0, 100), rng.uniform(-1.5, 1.5)),
                      rand_sim3(rng, rng.uniform(0, 3.0), rng.uniform(0, 50), rng.uniform(-1.5, 1.5)),
                      rand_sim3(rng, rng.uniform(0, 3.0), rng.uniform(0, 50), rng.uniform(-1.5, 1.5))))
    # a large-translation measurement, and residuals with theta near pi and |sigma| near 3
    cases.append((rand_sim3(rng, 0.7, 100.0, 0.3), rand_sim3(rng, 0.2, 3.0, 0.1), rand_sim3(rng, 0.4, 2.0, -0.2)))
    cases.append((rand_sim3(rng, 3.0, 20.0, 3.0), I8, I8))
    cases.append((rand_sim3(rng, 2.9, 60.0, -3.0), I8, I8))
    worst = 0.0
    for Cm, S0, S1 in cases:
        e, J = L.edge_jacobian_host(Cm, S0, S1)
        assert np.abs(e - err_expm(mat(Cm), mat(S0), mat(S1))).max() < 1e-10 * max(1.0, np.abs(e).max())
        r = np.abs(J - fd_expm(Cm, S0, S1)).max() / np.abs(J).max()
        worst = max(worst, r)
    assert worst <= 1e-8, worst


@pytest.mark.parametrize("theta,upsilon,sigma", [(0.3, 2.0, 0.1), (2.5, 40.0, -1.2), (3.1, 100.0, 2.5)])
def test_left_jacobian_identity(theta, upsilon, sigma):
    """J_l(xi) = Ad_exp(xi) J_l(-xi), and both equal the high-precision series"""
    rng = np.random.default_rng(3)
    xi = S3.log(rand_sim3(rng, theta, upsilon, sigma), fix_b=1)
    e, Jl, Jl_neg = left_jacobian_via_host(xi)
    Ad = adjoint_np(S3.exp(e, fix_b=1))
    scale = np.abs(Jl).max()
    assert np.abs(Jl - Ad @ Jl_neg).max() < 1e-11 * scale
    assert np.abs(Jl - left_jacobian_mp(e)).max() < 1e-12 * scale
    assert np.abs(Jl_neg - left_jacobian_mp(-e)).max() < 1e-12 * np.abs(Jl_neg).max()


@pytest.mark.parametrize("which", ["theta", "sigma"])
def test_left_jacobian_continuous_at_zero(which):
    """No branch of the closed form: J_l at theta (or sigma) = 1e-9, 1e-6, 1e-3 matches the 40-digit series, and the
    three are within first order of each other"""
    base = np.array([0.2, -0.1, 0.3, 3.0, -5.0, 8.0, 0.2])
    prev = None
    for v in (1e-9, 1e-6, 1e-3):
        xi = base.copy()
        if which == "theta":
            xi[:3] *= v / np.linalg.norm(xi[:3])
        else:
            xi[6] = v
        # e is what the library's log returns for exp(xi): the comparison is made at that e
        e, Jl, _ = left_jacobian_via_host(xi)
        ref = left_jacobian_mp(e)
        assert np.abs(Jl - ref).max() < 1e-13 * np.abs(ref).max(), (v, np.abs(Jl - ref).max())
        if prev is not None:
            assert np.abs(Jl - prev).max() < 10 * v * np.abs(ref).max()
        prev = Jl


@pytest.mark.parametrize("theta", [1e-5, 1e-4, 1e-3, 4.4e-3, 5e-3, 1e-2, 0.5, 2.0])
def test_against_library_residual(theta):
    """Central differences (delta = 1e-6) of the library's own residual (sim3np, fix_b = 1): agreement to 1e-8, except
    where the residual's log uses theta = 0 coefficients (1e-4 < theta < 5e-3), where the gap is ~0.12 theta^2"""
    rng = np.random.default_rng(5)
    Cm = rand_sim3(rng, 0.4, 3.0, 0.1)
    S1 = rand_sim3(rng, 0.8, 4.0, -0.3)
    w = rng.standard_normal(3)
    xi = np.concatenate([w * theta / np.linalg.norm(w), [3.0, -5.0, 8.0], [0.2]])
    # S0 such that e = log(C S0 S1^-1) = xi
    S0 = S3.mul(S3.inv(Cm), S3.mul(S3.exp(xi, fix_b=1), S1))
    e, J = L.edge_jacobian_host(Cm, S0, S1)
    h = 1e-6
    Jn = np.zeros((7, 14))
    for d in range(7):
        x = np.zeros(7)
        x[d] = h
        P, M = S3.exp(x, fix_b=1), S3.exp(-x, fix_b=1)
        Jn[:, d] = (S3.edge_error(Cm, S3.mul(P, S0), S1, fix_b=1) - S3.edge_error(Cm, S3.mul(M, S0), S1, fix_b=1)) / (2 * h)
        Jn[:, 7 + d] = (S3.edge_error(Cm, S0, S3.mul(P, S1), fix_b=1) - S3.edge_error(Cm, S0, S3.mul(M, S1), fix_b=1)) / (2 * h)
    th = np.linalg.norm(e[:3])
    gap = np.abs(J - Jn).max() / np.abs(J).max()
    bound = 1e-8 if (th >= 5e-3 or th <= 1e-4) else 0.2 * th * th
    assert gap <= bound, (th, gap, bound)


def test_dof_mask_zeroes_columns():
    rng = np.random.default_rng(9)
    Cm, S0, S1 = (rand_sim3(rng, 1.0, 10.0, 0.4) for _ in range(3))
    e, J = L.edge_jacobian_host(Cm, S0, S1)
    for mask in (0x78, 0x40):
        em, Jm = L.edge_jacobian_host(Cm, S0, S1, dof_mask=mask)
        assert np.array_equal(em, e)
        for d in range(7):
            for c in (d, 7 + d):
                if (mask >> d) & 1:
                    assert np.array_equal(Jm[:, c], J[:, c])
                else:
                    assert not Jm[:, c].any()


def test_jacobians_option():
    G = L.Graph()
    assert G.options().jacobians == 0 and L.default_options().jacobians == 0
    with pytest.raises(L.Sim3OptError) as ei:
        G.set_options(jacobians=1)  # the as-written B (the default) is refused
    assert ei.value.code == L.ERR_ARG and "fix_small_angle_b" in str(ei.value)
    assert G.options().jacobians == 0
    with pytest.raises(L.Sim3OptError) as ei:
        G.set_options(jacobians=2, fix_small_angle_b=1)
    assert ei.value.code == L.ERR_ARG
    G.set_options(jacobians=1, fix_small_angle_b=1)
    assert G.options().jacobians == 1
    with pytest.raises(L.Sim3OptError):  # switching the B back alone is refused as well
        G.set_options(fix_small_angle_b=0)
    with pytest.raises(L.Sim3OptError):
        L.edge_jacobian_host(I8, I8, I8, fix_small_angle_b=0)
    with pytest.raises(L.Sim3OptError):
        L.edge_jacobian_host(I8, I8, [0, 0, 0, 1, 0, 0, 0, -1.0])
    G2 = L.Graph(fix_small_angle_b=1)
    G2.add_vertex(0, I8, fixed=True)
    G2.add_vertex(1, I8)
    G2.add_edge(0, 1, I8)
    with pytest.raises(L.Sim3OptError) as ei:  # a device entry: initialize first
        G2.edge_jacobians()
    assert ei.value.code == L.ERR_STATE
