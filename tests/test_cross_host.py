"""Cross-correlation of the HK wavepacket with target coherent states, host side (no GPU): a numpy
restatement of the definition -- the reference of tests/test_cross_gpu.py -- against quadrature of int phi_k^*(x) psi(x) dx, the
transformed-coordinate form of the exponent the kernel evaluates, the result file's pooling, and the C-ABI symbols."""
import os
import re

import numpy as np
import pytest

from tests import cases

ZERO = 1.0e-8          # eigenvalue threshold of the reference's pseudo-inverses (propagators.py:16)
HBAR = 1.0


def overlap_constants(Gi, Gj):
    """A, B, C, fac of <q,p,Gi|q',p',Gj> (the formulas of the reference's CoherentStatesOverlap, propagators.py:125-179, 230):
    B = (Gi + Gj)^+, A = Gi B Gj, C = Gj B, fac^2 = 2^rank sqrt(det' Gi det' Gj) / det'(Gi + Gj)"""
    ei, ej = np.linalg.eigvalsh(Gi), np.linalg.eigvalsh(Gj)
    rank = int(np.count_nonzero(abs(ei) > ZERO))
    e, V = np.linalg.eigh(Gi + Gj)
    keep = abs(e) > ZERO
    B = (V[:, keep] / e[keep]) @ V[:, keep].T
    fac = np.sqrt(2.0 ** rank * np.sqrt(np.prod(ei[abs(ei) > ZERO])) * np.sqrt(np.prod(ej[abs(ej) > ZERO])) / np.prod(e[keep]))
    return Gi @ B @ Gj, B, Gj @ B, fac


def direct_exponents(q, p, Gt, G0, Q, P):
    """E_ik (n, K) of the definition, as written: q, p (D, n) the trajectories (bras, width Gt), Q, P (K, D) the targets (kets,
    width G0)"""
    A, B, C, _ = overlap_constants(Gt, G0)
    dq = Q.T[:, None, :] - q[:, :, None]                # (D, n, K): q_k - q_i
    dp = P.T[:, None, :] - p[:, :, None]
    return (-0.5 * np.einsum('aik,ab,bik->ik', dq, A, dq) - 0.5 / HBAR ** 2 * np.einsum('aik,ab,bik->ik', dp, B, dp)
            - 1j / HBAR * np.einsum('ka,aik->ik', P, dq) + 1j / HBAR * np.einsum('aik,ab,bik->ik', dq, C, dp))


def cross_terms(q, p, v, Gt, G0, Q, P):
    """x_ik = conj(O_ik) v_i, (n, K)"""
    fac = overlap_constants(Gt, G0)[3]
    return np.conj(fac * np.exp(direct_exponents(q, p, Gt, G0, Q, P))) * v[:, None]


def restated_cross(q, p, v, Gt, G0, Q, P, kept=None):
    """the five columns (K, 5) of the definition: Re X, Im X, S_rr, S_ii, S_ri with X_k = sum_i x_ik (no dynamical phase);
    ``kept`` (n,) bool: the trajectories that contribute"""
    x = cross_terms(q, p, v, Gt, G0, Q, P)
    if kept is not None:
        x = x[np.asarray(kept, dtype=bool)]
    return np.stack((x.real.sum(0), x.imag.sum(0), (x.real ** 2).sum(0), (x.imag ** 2).sum(0), (x.real * x.imag).sum(0)), axis=1)


def psd_sqrt(M):
    M = 0.5 * (M + M.T)
    e, V = np.linalg.eigh(M)
    return (V * np.sqrt(np.clip(e, 0.0, None))) @ V.T


def transformed_exponents(q, p, Gt, G0, Q, P):
    """E_ik from differences in transformed coordinates, the form sc_hk_cross evaluates: La = A^(1/2), Lb = B^(1/2) / hbar,
    Re E = -1/2 (|La q_k - La q_i|^2 + |Lb p_k - Lb p_i|^2), Im E = 1/hbar sum_d dq_d ((C p_k)_d - (C p_i)_d - p_k,d)"""
    A, B, C, _ = overlap_constants(Gt, G0)
    La, Lb = psd_sqrt(A), psd_sqrt(B) / HBAR
    ti = (La @ q, Lb @ p, q, C @ p)                     # (D, n) each: the trajectory rows
    tk = (La @ Q.T, Lb @ P.T, Q.T, C @ P.T, P.T)        # (D, K) each: the target rows
    da, db, dq = (tk[j][:, None, :] - ti[j][:, :, None] for j in range(3))
    g = (tk[3] - tk[4])[:, None, :] - ti[3][:, :, None]
    return -0.5 * ((da ** 2).sum(0) + (db ** 2).sum(0)) + 1j / HBAR * (dq * g).sum(0)


def gaussian(q, p, G, x):
    """<x|q,p,G> = (det'G / pi^rank)^(1/4) exp(-1/2 (x-q)^T G (x-q) + i/hbar p.(x-q)) (reference propagators.py:284-290);
    q, p (D,), x (D, nx)"""
    e = np.linalg.eigvalsh(G)
    keep = abs(e) > ZERO
    fac = (np.prod(e[keep]) / np.pi ** int(np.count_nonzero(keep))) ** 0.25
    dx = x - q[:, None]
    return fac * np.exp(-0.5 * np.einsum('ax,ab,bx->x', dx, G, dx) + 1j / HBAR * (p @ dx))


def coherent_overlap(qb, pb, Gb, qk, pk, Gk):
    """<qb,pb,Gb|qk,pk,Gk> in closed form"""
    E = direct_exponents(qb[:, None], pb[:, None], Gb, Gk, qk[None, :], pk[None, :])[0, 0]
    return overlap_constants(Gb, Gk)[3] * np.exp(E)


def _random_spd(rng, D):
    M = rng.normal(size=(D, D))
    e = rng.uniform(0.6, 1.8, D)
    V = np.linalg.qr(M)[0]
    return (V * e) @ V.T


# ------------------------------------------------------------------------------------------- 1. restatement vs quadrature

@pytest.mark.parametrize("D", [1, 2])
def test_restatement_matches_quadrature(D):
    """X_k = int phi_k^*(x) psi(x) dx with psi(x) = sum_i v_i <x|q_i,p_i,Gamma_t>, by the trapezoid rule (spectrally accurate for
    Gaussians: the grid reaches 9 widths beyond every centre at 25 points per width)"""
    rng = np.random.default_rng(10 + D)
    n, K = 7, 5
    Gt, G0 = _random_spd(rng, D), _random_spd(rng, D)        # D = 2: non-diagonal, Gamma_t != Gamma_0
    q, p = rng.normal(0.0, 0.8, (D, n)), rng.normal(0.0, 1.2, (D, n))
    v = rng.normal(size=n) + 1j * rng.normal(size=n)
    Q, P = rng.normal(0.0, 0.8, (K, D)), rng.normal(0.0, 1.2, (K, D))
    axis = np.arange(-14.0, 14.0 + 1e-9, 0.04)
    x = np.stack([a.ravel() for a in np.meshgrid(*([axis] * D), indexing="ij")])
    psi = sum(v[i] * gaussian(q[:, i], p[:, i], Gt, x) for i in range(n))
    quad = np.array([np.sum(np.conj(gaussian(Q[k], P[k], G0, x)) * psi) for k in range(K)]) * 0.04 ** D
    rows = restated_cross(q, p, v, Gt, G0, Q, P)
    X = rows[:, 0] + 1j * rows[:, 1]
    dev = abs(X - quad).max() / abs(X).max()
    print(f"D = {D}: max |X| {abs(X).max():.3e}, deviation from quadrature {dev:.2e} of it")
    assert dev <= 1e-10
    x_ik = cross_terms(q, p, v, Gt, G0, Q, P)
    assert np.allclose(rows[:, 2], (x_ik.real ** 2).sum(0), rtol=1e-15) and np.allclose(rows[:, 4], (x_ik.real * x_ik.imag).sum(0), rtol=1e-15)


# ------------------------------------------------------------------------------------------- 2. transformed coordinates

def _identity_deviation(q, p, Gt, G0, Q, P):
    E, T = direct_exponents(q, p, Gt, G0, Q, P), transformed_exponents(q, p, Gt, G0, Q, P)
    return abs(E - T).max() / max(1.0, abs(E).max())


def test_transformed_exponent_dense():
    rng = np.random.default_rng(5)
    D, n, K = 6, 9, 4
    Gt, G0 = _random_spd(rng, D), _random_spd(rng, D)
    dev = _identity_deviation(rng.normal(0.0, 0.8, (D, n)), rng.normal(0.0, 1.2, (D, n)), Gt, G0, rng.normal(0.0, 0.8, (K, D)),
                              rng.normal(0.0, 1.2, (K, D)))
    print(f"dense D = {D}: transformed against direct exponent {dev:.2e}")
    assert dev <= 1e-13


def test_transformed_exponent_singular_widths():
    """methylium's Cartesian widths are singular (rank 6 of 12): A, B and their roots carry the pseudo-inverse conventions"""
    g = cases.load("hk_methylium")
    Gt, G0 = g["Gamma_t"], g["Gamma_0"]
    D = Gt.shape[0]
    assert np.count_nonzero(abs(np.linalg.eigvalsh(Gt)) > ZERO) < D
    q, p = g["zi"][:D, :16], g["zi"][D:, :16]
    Q = np.vstack((g["q0"], q[:, 16 - 3:].T))
    P = np.vstack((g["p0"], p[:, 16 - 3:].T))
    dev = _identity_deviation(q, p, Gt, G0, Q, P)
    print(f"methylium: transformed against direct exponent {dev:.2e}")
    assert dev <= 1e-13


# ------------------------------------------------------------------------------------------- 3. result file and finalize_cross

def _batch(rng, nt, K, n):
    """raw rows (nt, K, 5) of a batch of n terms per step and target, with the weight 1/n inside the terms"""
    x = (rng.normal(size=(nt, K, n)) + 1j * rng.normal(size=(nt, K, n))) / n
    return np.stack((x.real.sum(2), x.imag.sum(2), (x.real ** 2).sum(2), (x.imag ** 2).sum(2), (x.real * x.imag).sum(2)), axis=2), x


def test_finalize_cross():
    from semiclassical_amd import hostmath
    from semiclassical_amd.propagators import HermanKlukPropagator as HK
    rng = np.random.default_rng(2)
    nt, K, n, t0, dt, E0 = 4, 3, 50, 0.7, 0.3, 0.9
    raw, x = _batch(rng, nt, K, n)
    C, sigma = HK.finalize_cross(raw, t0, dt, E0, n)
    times = t0 + hostmath.time_grid(nt, dt)
    phased = x * np.exp(1j * times * E0 / HBAR)[:, None, None]
    assert C.shape == sigma.shape == (nt, K)
    assert np.allclose(C, phased.sum(2), rtol=1e-13, atol=0)
    # sigma^2 of the mean of n samples y = n x: var(y) / n, with the unbiased variance
    want = np.sqrt(np.var(n * phased.real, axis=2, ddof=1) / n) + 1j * np.sqrt(np.var(n * phased.imag, axis=2, ddof=1) / n)
    assert np.allclose(sigma, want, rtol=1e-10, atol=0)


def _store(tmp_path, name, nt):
    from collections import namedtuple
    import torch
    from semiclassical_amd import driver
    store = driver.CorrelationStore(str(tmp_path / name))
    setup = namedtuple("S", "adiabatic_gap zero_point_energy")(0.1, 0.2)
    store.start({"results": {"overwrite": True}}, "HK", torch.linspace(0.0, 1.0, nt), setup)
    return store


def _record(rng, nt, K, n, Q, P, errors=True):
    raw, x = _batch(rng, nt, K, n)
    rec = {"q": Q, "p": P, "correlation": raw[:, :, 0] + 1j * raw[:, :, 1]}
    if errors:
        rec["second_moment"] = n * raw[:, :, 2:5]
    auto = np.ones(nt, dtype=complex)
    return auto, rec, x


def test_store_pools_batches(tmp_path):
    """two batches pooled equal one batch of both: means with the weights of the autocorrelation, errors from the pooled moments"""
    from semiclassical_amd import hostmath
    rng = np.random.default_rng(4)
    nt, K, D, n1, n2 = 3, 4, 2, 30, 50
    Q, P = rng.normal(size=(K, D)), rng.normal(size=(K, D))
    a1, r1, x1 = _record(rng, nt, K, n1, Q, P)
    a2, r2, x2 = _record(rng, nt, K, n2, Q, P)
    store = _store(tmp_path, "two.npz", nt)
    store.add_batch(a1, a1, n1, second_moments=(np.zeros((nt, 3)), np.zeros((nt, 3))), cross=r1)
    store.add_batch(a2, a2, n2, second_moments=(np.zeros((nt, 3)), np.zeros((nt, 3))), cross=r2)
    got = dict(np.load(store.path))
    # the same samples y = n_b x as ONE batch of n1 + n2 terms with the weight 1 / (n1 + n2)
    n = n1 + n2
    x = np.concatenate((n1 * x1, n2 * x2), axis=2) / n
    assert np.array_equal(got["cross_targets_q"], Q) and np.array_equal(got["cross_targets_p"], P)
    assert got["cross_correlation"].shape == (nt, K)
    assert np.allclose(got["cross_correlation"], x.sum(2), rtol=1e-13, atol=0)
    m3 = np.stack(((x.real ** 2).sum(2), (x.imag ** 2).sum(2), (x.real * x.imag).sum(2)), axis=2)
    assert np.allclose(got["cross_correlation_second_moment"], n * m3, rtol=1e-12, atol=0)
    assert np.allclose(got["cross_correlation_error"], hostmath.standard_errors(x.sum(2), m3, n), rtol=1e-10, atol=0)
    assert int(got["trajectories"]) == n


def test_store_drops_errors_it_cannot_pool(tmp_path):
    rng = np.random.default_rng(6)
    nt, K, D = 3, 2, 2
    Q, P = rng.normal(size=(K, D)), rng.normal(size=(K, D))
    store = _store(tmp_path, "drop.npz", nt)
    a, r, _ = _record(rng, nt, K, 20, Q, P, errors=True)
    store.add_batch(a, a, 20, cross=r)
    assert "cross_correlation_error" in np.load(store.path)
    a, r, _ = _record(rng, nt, K, 20, Q, P, errors=False)
    store.add_batch(a, a, 20, cross=r)
    got = np.load(store.path)
    assert "cross_correlation" in got and "cross_correlation_error" not in got and "cross_correlation_second_moment" not in got


def test_store_refuses_other_targets(tmp_path):
    from semiclassical_amd import driver
    rng = np.random.default_rng(8)
    nt, K, D = 3, 2, 2
    Q, P = rng.normal(size=(K, D)), rng.normal(size=(K, D))
    store = _store(tmp_path, "other.npz", nt)
    a, r, _ = _record(rng, nt, K, 20, Q, P)
    store.add_batch(a, a, 20, cross=r)
    before = dict(np.load(store.path))
    for other in (dict(r, q=Q + 1e-9), dict(r, p=P[::-1].copy()), dict(r, q=Q[:1], p=P[:1], correlation=r["correlation"][:, :1]), None):
        with pytest.raises(driver.ConfigurationError):
            store.add_batch(a, a, 20, cross=other)
    # ... and a file without cross-correlation functions takes none
    plain = _store(tmp_path, "plain.npz", nt)
    plain.add_batch(a, a, 20)
    with pytest.raises(driver.ConfigurationError):
        plain.add_batch(a, a, 20, cross=r)
    after = dict(np.load(store.path))
    assert set(before) == set(after) and all(np.array_equal(before[k], after[k]) for k in before)
    # start() refuses before any trajectory runs
    import torch
    task = {"results": {"overwrite": False}}
    with pytest.raises(driver.ConfigurationError):
        store.start(task, "HK", torch.linspace(0.0, 1.0, nt), None, cross_targets=(Q + 1.0, P))
    store.start(task, "HK", torch.linspace(0.0, 1.0, nt), None, cross_targets=(Q, P))


def test_store_without_the_key_has_todays_keys(tmp_path):
    store = _store(tmp_path, "none.npz", 3)
    a = np.ones(3, dtype=complex)
    store.add_batch(a, a, 10)
    assert set(np.load(store.path).keys()) == {"propagator", "times", "autocorrelation", "ic_correlation", "adiabatic_gap",
                                               "zero_point_energy", "trajectories"}


def test_driver_refuses_wm_and_bad_files(tmp_path):
    from semiclassical_amd import driver
    task = {"task": "dynamics", "propagator": "WM", "cross_correlation_targets": str(tmp_path / "t.npz"), "potential": {"type": "none"}}
    with pytest.raises(driver.ConfigurationError, match="WM"):
        driver.run_semiclassical_dynamics(task)
    np.savez(tmp_path / "t.npz", q=np.zeros((2, 3)), p=np.zeros((2, 4)))
    with pytest.raises(driver.ConfigurationError, match="shape"):
        driver._load_targets(str(tmp_path / "t.npz"), 3)
    np.savez(tmp_path / "u.npz", q=np.zeros((2, 3)))
    with pytest.raises(driver.ConfigurationError):
        driver._load_targets(str(tmp_path / "u.npz"), 3)
    np.savez(tmp_path / "v.npz", q=np.zeros((2, 3)), p=np.full((2, 3), np.nan))
    with pytest.raises(driver.ConfigurationError, match="non-finite"):
        driver._load_targets(str(tmp_path / "v.npz"), 3)


# ------------------------------------------------------------------------------------------- 4. ABI

def test_symbols_are_declared_bound_and_exported():
    from semiclassical_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "semiclassical_hip.h")).read()
    for name in ("sc_hk_cross", "sc_hk_cross_rows"):
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    assert "propagators.py:181-240" in header
    assert int(re.search(r"#define SC_ABI_VERSION\s+(\d+)", header).group(1)) == 18
    assert _lib.lib.sc_abi_version() == _lib.ABI_VERSION == 18
    assert _lib.lib.sc_hk_cross_rows(1, 1) == 1 and _lib.lib.sc_hk_cross_rows(64, 500) == 1
    assert _lib.lib.sc_hk_cross_rows(65, 1) == 2 and _lib.lib.sc_hk_cross_rows(130, 65) == 3
    assert _lib.lib.sc_hk_cross_rows(0, 5) == 0 and _lib.lib.sc_hk_cross_rows(5, 0) == 0


def test_propagators_offer_cross_correlation():
    import inspect
    from semiclassical_amd import propagators as PR
    assert callable(PR.HermanKlukPropagator.cross_correlation) and callable(PR.HermanKlukPropagator.finalize_cross)
    run = inspect.signature(PR.HermanKlukPropagator.run).parameters
    assert "targets" in run and "cross" in run and run["targets"].default is None and run["cross"].default is None
    assert PR.WaltonManolopoulosPropagator._cross_ok is False and PR.HermanKlukPropagator._cross_ok is True


# ------------------------------------------------------------------------------------------- 5. the 5 sigma check, on the CPU

def initial_coefficients(g):
    """v_i of t = 0 from the fixture's own initial conditions: <q_i,p_i,Gamma_i|q0,p0,Gamma_0> / (N (2 pi hbar)^D P_i)"""
    D, n = g["q0"].shape[0], g["zi"].shape[1]
    q, p = g["zi"][:D], g["zi"][D:]
    E = direct_exponents(q, p, g["Gamma_i"], g["Gamma_0"], g["q0"][None, :], g["p0"][None, :])[:, 0]
    vi = overlap_constants(g["Gamma_i"], g["Gamma_0"])[3] * np.exp(E)
    return vi / (n * (2.0 * np.pi * HBAR) ** D * g["probi"])


def width_targets(g, modes=(0, 4), widths=1.0):
    """(q0, p0) and q0 -+ `widths` / sqrt(Gamma_0[m, m]) along the modes m: (Q, P), (1 + 2 len(modes), D)"""
    q0, p0, G0 = g["q0"], g["p0"], g["Gamma_0"]
    Q = [q0.copy()]
    for m in modes:
        for sign in (-1.0, 1.0):
            t = q0.copy()
            t[m] += sign * widths / np.sqrt(G0[m, m])
            Q.append(t)
    return np.array(Q), np.tile(p0, (len(Q), 1))


def exact_overlaps(g, Q, P):
    """<phi_k|phi_0>, the closed-form Gaussian overlaps the estimates of t = 0 converge to"""
    return np.array([coherent_overlap(Q[k], P[k], g["Gamma_0"], g["q0"], g["p0"], g["Gamma_0"]) for k in range(len(Q))])


ROUNDING = 1.0e-12     # what fp64 sums of N <= 1e4 terms of magnitude 1/N resolve (N 2^-53 = 1e-12), ten orders below any sigma here


def within_five_sigma(C, sigma, exact):
    """|C - exact| <= 5 sigma, real and imaginary parts apart.  The (q0, p0) target of an ensemble sampled with Gamma_i = Gamma_0 is
    degenerate at t = 0: every term is 1/N up to rounding, so sigma is 0 or rounding noise and the deviation is rounding noise too
    -- the comparison cannot resolve below the arithmetic, hence the ROUNDING floor (it plays no part for sigma ~ 1e-2)."""
    d = C - exact
    return (abs(d.real) <= 5.0 * sigma.real + ROUNDING) & (abs(d.imag) <= 5.0 * sigma.imag + ROUNDING)


def test_five_sigma_at_t0_on_the_cpu():
    """the restatement on the fixture's (zi, probi) at t = 0 lies within 5 sigma of <phi_k|phi_0> for every target of the GPU
    test (test_cross_gpu.py::test_standard_errors_cover_the_exact_overlap): the displacement of one width stands"""
    from semiclassical_amd import hostmath
    g = cases.load("hk_as5_chi002")
    D, n = g["q0"].shape[0], g["zi"].shape[1]
    Q, P = width_targets(g)
    rows = restated_cross(g["zi"][:D], g["zi"][D:], initial_coefficients(g), g["Gamma_t"], g["Gamma_0"], Q, P)
    C = rows[:, 0] + 1j * rows[:, 1]
    sigma = hostmath.standard_errors(C, rows[:, 2:5], n)
    exact = exact_overlaps(g, Q, P)
    for k in range(len(Q)):
        print(f"target {k}: C {C[k]:.6f}  exact {exact[k]:.6f}  sigma {sigma[k]:.2e}  |dev| / sigma "
              f"{abs((C - exact)[k].real) / max(sigma[k].real, 1e-300):.2f}, {abs((C - exact)[k].imag) / max(sigma[k].imag, 1e-300):.2f}")
    assert abs(exact[0] - 1.0) < 1e-12
    assert within_five_sigma(C, sigma, exact).all()
