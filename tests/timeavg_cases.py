"""Time-averaged Herman-Kluk spectra: a numpy restatement of the definitions -- the yardstick of
tests/test_timeavg_host.py and tests/test_timeavg_gpu.py -- and the one-dimensional harmonic oscillator with its closed form."""
import math

import numpy as np

from tests.test_cross_host import HBAR, direct_exponents, overlap_constants


# ------------------------------------------------------------------------------------------- the restatement

def unit_prefactor(c, act):
    """u_i = c_i / |c_i| e^{i S_i/hbar}, 0 where c_i = 0; c (n,) complex: the signed root of the prefactor's square"""
    mod = np.abs(c)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(mod > 0, c / mod, 0.0) * np.exp(1j * act / HBAR)


def restated_terms(q, p, c, act, Gt, G0, Q, P, kept=None):
    """g_ik = conj(O_ik) u_i of one step, (n, K): q, p (D, n) the trajectories (bras, width Gt), Q, P (K, D) the reference states
    (kets, width G0); ``kept`` (n,) bool: every other row is exactly zero and its state is not looked at"""
    n = q.shape[1]
    rows = np.arange(n) if kept is None else np.flatnonzero(np.asarray(kept, dtype=bool))
    g = np.zeros((n, Q.shape[0]), dtype=complex)
    if len(rows):
        O = overlap_constants(Gt, G0)[3] * np.exp(direct_exponents(q[:, rows], p[:, rows], Gt, G0, Q, P))
        g[rows] = np.conj(O) * unit_prefactor(c[rows], act[rows])[:, None]
    return g


def time_grid(t_a, dt, ns, first=0):
    """t_s = t_a + s dt for s = first ... first + ns - 1: a product, not a repeated addition"""
    return t_a + np.arange(first, first + ns) * dt


def restated_accumulator(g, energies, t_a, dt):
    """A_ik(E_e) = dt sum_s g_ik(t_s) exp(i E_e t_s / hbar), (n, K, NE), from g (ns, n, K)"""
    ns, n, K = g.shape
    W = dt * np.exp(1j * np.outer(time_grid(t_a, dt, ns), energies) / HBAR)            # (ns, NE)
    return (g.reshape(ns, n * K).T @ W).reshape(n, K, len(energies))


def restated_sums(A, T, mc_norm, probi, kept=None):
    """(I, S2), (K, NE) each: y_ik(e) = |A_ik(E_e)|^2 / (2 pi hbar T mc_norm P_i), I = sum_i y, S2 = sum_i y^2; a trajectory
    outside ``kept`` counts as y = 0"""
    y = np.abs(A) ** 2 / (2.0 * np.pi * HBAR * T * mc_norm * probi[:, None, None])
    if kept is not None:
        y = y[np.asarray(kept, dtype=bool)]
    return y.sum(0), (y ** 2).sum(0)


def standard_error(I, S2, N):
    """sigma = sqrt(max(N S2 - I^2, 0) / (N - 1))"""
    return np.sqrt(np.maximum(N * S2 - I ** 2, 0.0) / (N - 1.0))


def restated_spectrum(g, energies, t_a, dt, mc_norm, probi, N, kept=None):
    """(I, sigma) of the window of all ns steps of g (ns, n, K)"""
    I, S2 = restated_sums(restated_accumulator(g, energies, t_a, dt), g.shape[0] * dt, mc_norm, probi, kept)
    return I, standard_error(I, S2, N)


# ------------------------------------------------------------------------------------------- the harmonic oscillator

OSC = dict(omega=1.0, q0=1.6, dt=0.05, ns=2000, N=2048)
OSC_ENERGIES = np.array([0.5, 1.0, 1.5, 2.2, 2.5, 3.5])
OSC_PEAKS = (0, 2, 4)          # E = 0.5, 1.5, 2.5: the eigenvalues among them


def oscillator_closed_form(energies, omega=1.0, q0=1.6, dt=0.05, ns=2000, nmax=60):
    """I(E) = sum_n e^{-s} s^n / n! |dt sum_s e^{i (E - (n + 1/2) omega) t_s}|^2 / (2 pi T), s = omega q0^2 / 2: the coherent state
    chi = |q0, 0, omega> on the oscillator's own surface, on the discrete time grid t_s = s dt"""
    s = 0.5 * omega * q0 ** 2
    t = time_grid(0.0, dt, ns)
    out = np.zeros(len(energies))
    for n in range(nmax):
        weight = math.exp(-s) * s ** n / math.factorial(n)
        kernel = np.abs(dt * np.exp(1j * np.outer(energies - (n + 0.5) * omega, t)).sum(1)) ** 2
        out += weight * kernel / (2.0 * np.pi * ns * dt)
    return out


def oscillator_sample(N, q0=1.6, seed=2048):
    """(q, p, prob), N points from the Husimi density |<q, p, 1|q0, 0, 1>|^2 / (2 pi hbar) of chi (Gamma_i = Gamma_0 = 1)"""
    rng = np.random.default_rng(seed)
    q, p = q0 + rng.normal(size=N), rng.normal(size=N)
    return q, p, np.exp(-0.5 * ((q - q0) ** 2 + p ** 2)) / (2.0 * np.pi)


def oscillator_terms(q, p, q0=1.6, dt=0.05, ns=2000):
    """g_i(t_s) (ns, n, 1) on analytic trajectories of H = (p^2 + q^2) / 2 with Gamma_t = Gamma_0 = 1: q_t, p_t a rotation, the
    action in closed form and the prefactor c_t = sqrt(e^{-i t}) on its continuous branch, e^{-i t / 2}"""
    t = time_grid(0.0, dt, ns)[:, None]
    qt, pt = q * np.cos(t) + p * np.sin(t), p * np.cos(t) - q * np.sin(t)
    act = 0.25 * (p ** 2 - q ** 2) * np.sin(2.0 * t) - 0.5 * q * p * (1.0 - np.cos(2.0 * t))
    c = np.exp(-0.5j * t) * np.ones_like(qt)
    one = np.eye(1)
    Q, P = np.array([[q0]]), np.array([[0.0]])
    return np.stack([restated_terms(qt[s][None, :], pt[s][None, :], c[s], act[s], one, one, Q, P) for s in range(ns)])
