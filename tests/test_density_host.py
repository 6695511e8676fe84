"""Reduced density of the HK wavepacket, host side (no GPU): the C-ABI symbols, and a numpy restatement
of the closed form -- the reference of tests/test_density_gpu.py -- against direct quadrature of |psi|^2."""
import os
import re

import numpy as np

ZERO = 1.0e-8          # eigenvalue threshold of the reference's pseudo-inverses (propagators.py:16)
HBAR = 1.0


def overlap_constants(G):
    """A, B, C, fac of <q_i,p_i,G|q_j,p_j,G> (reference propagators.py:145-179, 230) for one width matrix G"""
    e = np.linalg.eigvalsh(G)
    rank = int(np.count_nonzero(abs(e) > ZERO))
    det_g = np.prod(e[abs(e) > ZERO])
    e2, V2 = np.linalg.eigh(2.0 * G)
    keep = abs(e2) > ZERO
    B = (V2[:, keep] / e2[keep]) @ V2[:, keep].T
    fac = np.sqrt(2.0 ** rank * np.sqrt(det_g) * np.sqrt(det_g) / np.prod(e2[keep]))
    return G @ B @ G, B, G @ B, fac


def pair_exponents(q, p, G):
    """E_ij (n, n) and fac with O_ij = fac exp(E_ij) (reference propagators.py:232-237); q, p (D, n)"""
    A, B, C, fac = overlap_constants(G)
    dq = q[:, None, :] - q[:, :, None]                  # (D, i, j): q_j - q_i
    dp = p[:, None, :] - p[:, :, None]
    E = (-0.5 * np.einsum('aij,ab,bij->ij', dq, A, dq) - 0.5 / HBAR ** 2 * np.einsum('aij,ab,bij->ij', dp, B, dp)
         - 1j / HBAR * np.einsum('aj,aij->ij', p, dq) + 1j / HBAR * np.einsum('aij,ab,bij->ij', dq, C, dp))
    return E, fac


def density_terms(q, p, G, u):
    """sigma^2, m_ij, beta_ij of direction u and the combined exponent at s = m: E_ij + beta^2 / (2 sigma^2)"""
    _, B, _, _ = overlap_constants(G)
    E, fac = pair_exponents(q, p, G)
    sigma2 = float(u @ B @ u)
    a, b = 0.5 * (u @ q), (u @ B @ p) / HBAR
    m = a[:, None] + a[None, :]
    beta = b[None, :] - b[:, None]
    return sigma2, m, beta, E + beta ** 2 / (2.0 * sigma2), fac


def restated_density(q, p, v, G, directions, s, complex_sum=False, bra=None):
    """rho_u(s) = Re sum_ij v_i^* v_j O_ij (2 pi sigma^2)^-1/2 exp(-(s - mu_ij)^2 / (2 sigma^2)), each term as the exponential of
    ONE exponent.  q, p (D, n), v (n,), G = Gamma_t (D, D), directions (M, D), s (ns,) -> (M, ns); ``complex_sum``: the complex
    sums, not their real parts; ``bra`` = (q, p, v) of another set of bras (default: the kets)."""
    U = np.atleast_2d(np.asarray(directions, dtype=float))
    s = np.asarray(s, dtype=float)
    qi, pi, vi = (q, p, v) if bra is None else bra
    ni = qi.shape[1]
    qq, pp = np.concatenate((qi, q), 1), np.concatenate((pi, p), 1)
    out = np.empty((U.shape[0], s.shape[0]), dtype=complex)
    for d, u in enumerate(U):
        sigma2, m, beta, Z, fac = density_terms(qq, pp, G, u)
        m, beta, Z = m[:ni, ni:], beta[:ni, ni:], Z[:ni, ni:]
        w = fac * np.conj(vi)[:, None] * v[None, :] / np.sqrt(2.0 * np.pi * sigma2)
        for k, sk in enumerate(s):
            ds = sk - m
            out[d, k] = np.sum(w * np.exp(Z - ds ** 2 / (2.0 * sigma2) + 1j * ds * beta / sigma2))
    return out if complex_sum else out.real


def first_moment(q, p, v, G, u):
    """int s rho_u(s) ds = Re sum_ij v_i^* v_j O_ij mu_ij"""
    _, m, beta, _, fac = density_terms(q, p, G, u)
    E, _ = pair_exponents(q, p, G)
    return float(np.sum(fac * np.conj(v)[:, None] * v[None, :] * np.exp(E) * (m + 1j * beta)).real)


def gaussian_wavefunction(q, p, v, G, x):
    """psi(x) = sum_i v_i (det'G / pi^rank)^(1/4) exp(-1/2 (x-q_i)^T G (x-q_i) + i/hbar p_i.(x-q_i)) (reference
    propagators.py:284-290); x (D, nx)"""
    e = np.linalg.eigvalsh(G)
    keep = abs(e) > ZERO
    fac = (np.prod(e[keep]) / np.pi ** int(np.count_nonzero(keep))) ** 0.25
    dx = x[:, None, :] - q[:, :, None]                  # (D, n, nx)
    g = fac * np.exp(-0.5 * np.einsum('anx,ab,bnx->nx', dx, G, dx) + 1j / HBAR * np.einsum('an,anx->nx', p, dx))
    return v @ g


def _ensemble(rng, D, n):
    q = rng.normal(0.0, 0.8, (D, n))
    p = rng.normal(0.0, 1.2, (D, n))
    v = rng.normal(size=n) + 1j * rng.normal(size=n)
    return q, p, v


def test_symbols_are_exported_and_declared():
    from semiclassical_amd import _lib
    for name in ("sc_density_pair_sum", "sc_density_pair_sum_rows"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    assert _lib.lib.sc_density_pair_sum_rows(1, 1) == 1
    assert _lib.lib.sc_density_pair_sum_rows(130, 65) == 3 * 2        # bra bands x shares of the ket tiles
    assert _lib.lib.sc_density_pair_sum_rows(0, 5) == 0


def test_abi_number_is_unchanged():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "semiclassical_hip.h")).read()
    assert int(re.search(r"#define SC_ABI_VERSION\s+(\d+)", header).group(1)) == 18


def test_propagators_offer_reduced_density():
    from semiclassical_amd import propagators as PR
    assert callable(PR.HermanKlukPropagator.reduced_density)
    assert PR.WaltonManolopoulosPropagator.reduced_density is not PR.HermanKlukPropagator.reduced_density


def test_restated_formula_matches_quadrature_in_two_dimensions():
    """(a) D = 2, non-diagonal Gamma, a rotated direction that is not normalised, 7 trajectories with random complex v"""
    rng = np.random.default_rng(7)
    G = np.array([[1.3, 0.4], [0.4, 0.7]])
    q, p, v = _ensemble(rng, 2, 7)
    u = 1.7 * np.array([np.cos(0.6), np.sin(0.6)])
    s = np.linspace(-6.0, 6.0, 41)
    rho = restated_density(q, p, v, G, u, s)[0]
    # x = (s / |u|) e + t e_perp, delta(s - u.x) = delta(x_par - s / |u|) / |u|
    un = np.linalg.norm(u)
    e, eperp = u / un, np.array([-u[1], u[0]]) / un
    t = np.linspace(-14.0, 14.0, 2801)
    want = np.empty_like(rho)
    for k, sk in enumerate(s):
        x = (sk / un) * e[:, None] + t[None, :] * eperp[:, None]
        f = abs(gaussian_wavefunction(q, p, v, G, x)) ** 2
        want[k] = (t[1] - t[0]) * (f.sum() - 0.5 * (f[0] + f[-1])) / un
    assert rho.max() > 0.1
    assert np.max(abs(rho - want)) <= 1e-10 * rho.max()
    # ... and the integral over s is sum_ij v_i^* O_ij v_j
    E, fac = pair_exponents(q, p, G)
    norm2 = float((np.conj(v) @ (fac * np.exp(E)) @ v).real)
    fine = np.linspace(-16.0, 16.0, 641)
    r = restated_density(q, p, v, G, u, fine)[0]
    assert abs((fine[1] - fine[0]) * r.sum() - norm2) <= 1e-10 * norm2


def test_restated_formula_is_psi_squared_in_one_dimension():
    """(b) D = 1, u = 1"""
    rng = np.random.default_rng(8)
    G = np.array([[0.9]])
    q, p, v = _ensemble(rng, 1, 9)
    s = np.linspace(-4.0, 4.0, 57)
    rho = restated_density(q, p, v, G, [1.0], s)[0]
    want = abs(gaussian_wavefunction(q, p, v, G, s[None, :])) ** 2
    assert np.max(abs(rho - want)) <= 1e-12 * rho.max()


def test_combined_exponent_never_grows():
    """(c) Re (E_ij + beta^2 / (2 sigma^2)) <= 0 (Cauchy-Schwarz), also for a singular Gamma with u in its range"""
    rng = np.random.default_rng(9)
    for D, rank in ((2, 2), (5, 5), (6, 3)):
        Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
        w = rng.uniform(0.3, 2.0, D)
        w[rank:] = 0.0
        G = (Q * w) @ Q.T
        q, p, _ = _ensemble(rng, D, 12)
        u = Q[:, :rank] @ rng.standard_normal(rank)
        _, _, _, Z, _ = density_terms(q, p, G, u)
        assert Z.real.max() <= 1e-12
