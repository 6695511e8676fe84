"""Thermal ensembles on the host: hostmath.ThermalConstants, and the estimator -- the restatement of
tests/thermal_cases.py on host-drawn samples -- against the exact traces in a truncated Fock basis."""
import numpy as np
import pytest
import torch

from oracle import sc_oracle as orc
from semiclassical_amd import hostmath, units
from tests import cases, thermal_cases as tcs

torch.set_default_dtype(torch.float64)


# ------------------------------------------------------------------------------------------------ ThermalConstants

def test_constants_diagonal():
    omega = torch.tensor([0.004, 0.009, 0.013])
    masses = torch.tensor([1.0, 2.5, 0.7])
    kT = 0.006
    tc = hostmath.ThermalConstants(torch.diag(omega * masses), masses, kT)
    assert tc.diag and tc.dmodes == 3
    assert torch.allclose(tc.omega, omega, rtol=1e-14, atol=0)          # mode k is coordinate k: no reordering
    assert torch.allclose(tc.nbar, 1.0 / (torch.exp(omega / kT) - 1.0), rtol=1e-13, atol=0)
    assert torch.equal(tc.map_q, torch.diag(masses ** -0.5)) and torch.equal(tc.map_p, torch.diag(masses ** 0.5))
    # a permuted diagonal stays in place, too (eigh would sort it)
    tc2 = hostmath.ThermalConstants(torch.diag(torch.tensor([0.013, 0.004])), torch.ones(2), kT)
    assert torch.equal(tc2.omega, torch.tensor([0.013, 0.004]))


def test_constants_dense_and_singular():
    g = cases.load("hk_methylium")
    G0, masses = cases.T(g["Gamma_0"]), cases.T(g["masses"])
    tc = hostmath.ThermalConstants(G0, masses, 300.0 * units.kelvin_to_hartree)
    assert tc.dim == 12 and tc.dmodes == 6 and not tc.diag
    _, _, _, _, dprime = hostmath.sampling_matrices(G0, G0)
    assert tc.dmodes == dprime                                             # the same rule for the range of a singular width
    W = G0 / torch.sqrt(torch.outer(masses, masses))
    assert torch.allclose(tc.L @ torch.diag(tc.omega) @ tc.L.T, W, rtol=0, atol=1e-12 * float(abs(W).max()))
    assert torch.allclose(tc.L.T @ tc.L, torch.eye(6), atol=1e-12)
    # the images of the centres stay in the range of Gamma_0: no thermal population in a zero mode
    e, V = torch.linalg.eigh(W)
    null = V[:, e <= hostmath.ZERO]
    assert float(abs(null.T @ (torch.sqrt(masses).unsqueeze(1) * tc.map_q)).max()) < 1e-10


def test_constants_refusals_and_zero_temperature():
    G0, m = torch.diag(torch.tensor([1.0, 2.0])), torch.ones(2)
    for bad in (dict(p0=torch.tensor([0.0, 0.1])), dict(temperature=-1.0), dict(temperature=float("nan")), dict(masses=torch.ones(3)),
                dict(masses=torch.ones((2, 1))), dict(masses=torch.tensor([1.0, -1.0]))):
        kw = dict(Gamma_0=G0, masses=m, temperature=0.5)
        kw.update(bad)
        with pytest.raises(ValueError):
            hostmath.ThermalConstants(**kw)
    tc = hostmath.ThermalConstants(G0, m, 0.0, p0=torch.zeros(2))
    assert torch.equal(tc.nbar, torch.zeros(2))
    assert torch.equal(tc.draw_centres(7, torch.Generator().manual_seed(1)), torch.zeros((7, 4)))


def test_centre_variances():
    """Q_k ~ N(0, hbar nbar_k / omega_k), P_k ~ N(0, hbar nbar_k omega_k): sample variances of n = 2^16 draws within 4 sqrt(2/n)
    relative (four standard errors of a variance estimate)"""
    omega, kT, n = torch.tensor([0.5, 1.0, 2.2]), 0.9, 2 ** 16
    tc = hostmath.ThermalConstants(torch.diag(omega), torch.ones(3), kT)
    c = tc.draw_centres(n, torch.Generator().manual_seed(5))
    nbar = 1.0 / np.expm1(omega.numpy() / kT)
    want = np.concatenate((nbar / omega.numpy(), nbar * omega.numpy()))
    got = (c ** 2).mean(0).numpy()
    assert abs(got / want - 1.0).max() < 4.0 * np.sqrt(2.0 / n)
    assert abs(c.mean(0).numpy() / np.sqrt(want)).max() < 4.0 / np.sqrt(n)


def test_kelvin():
    assert abs(300.0 * units.kelvin_to_hartree * units.hartree_to_ev - 0.025852) < 1e-6


# ------------------------------------------------------------------------------------------------ the estimator is exact

N_EXACT, DT, NT = 20000, 0.1, 30
BASIS = (38, 32)


def _within(est, sigma, exact, k=5.0):
    dev = est - exact          # (1e-12: sums that are real by symmetry, sigma_Im = 0 at t = 0, against rounding)
    return bool((abs(dev.real) <= k * sigma.real + 1e-12).all() and (abs(dev.imag) <= k * sigma.imag + 1e-12).all())


def _worst(est, sigma, exact):
    dev = est - exact          # (from the second point on: at t = 0 the terms have no spread at all for Gamma_i = Gamma_0)
    return max(float((abs(dev.real)[1:] / sigma.real[1:]).max()), float((abs(dev.imag)[1:] / sigma.imag[1:]).max()))


@pytest.fixture(scope="module")
def exact_model():
    m = tcs.model_2d()
    prop, pot, tc, centres = tcs.model_objects(m, m["kT"], N_EXACT, seed=11)
    times = hostmath.time_grid(NT, DT)
    runs = {flag: tcs.run_restatement(prop if flag else tcs.model_objects(m, m["kT"], N_EXACT, seed=11)[0], pot, tc, centres, DT, NT,
                                      m["E0"], with_phase=flag) for flag in (True, False)}
    args = (tc.omega.numpy(), tc.L.numpy(), m["masses"], m["q0"], m["pos_gs"], m["hess_gs"], m["nac"])
    return m, tc, times, runs, args


def test_convention_at_zero_temperature():
    """the restatement at k_B T = 0 IS the oracle's zero-temperature C and k (1e-9), and the exact traces at k_B T = 0 -- same
    operator convention, T^+ = -n1.grad -- lie within five of its standard errors"""
    m = tcs.model_2d()
    n = 4000
    prop, pot, tc, centres = tcs.model_objects(m, 0.0, n, seed=3)
    assert not bool(centres.any())
    twin = orc.HKOracle(prop.Gamma_i, prop.Gamma_t)
    twin.set_initial_conditions(prop.q0, prop.p0, prop.Gamma_0, prop.zi.clone(), prop.probi.clone())
    want_c, want_k = orc.run_loop(twin, pot, DT, 12, m["E0"])
    C, K, _, _, sC, sK = tcs.run_restatement(prop, pot, tc, centres, DT, 12, m["E0"])
    assert abs(C - want_c).max() <= 1e-9 * abs(want_c).max() and abs(K - want_k).max() <= 1e-9 * abs(want_k).max()
    eC, eK = tcs.exact_traces(tc.omega.numpy(), tc.L.numpy(), m["masses"], m["q0"], m["pos_gs"], m["hess_gs"], m["nac"], 0.0,
                              hostmath.time_grid(12, DT), (20, 18))
    assert abs(eC[0] - 1.0) < 1e-12
    assert _within(C, sC, eC) and _within(K, sK, eK)


def test_basis_is_converged(exact_model):
    m, tc, times, runs, args = exact_model
    some = times[::7]
    small = tcs.exact_traces(*args, m["kT"], some, BASIS)
    big = tcs.exact_traces(*args, m["kT"], some, tuple(2 * b for b in BASIS))
    change = max(abs(small[0] - big[0]).max(), abs(small[1] - big[1]).max())
    print(f"doubling the basis {BASIS} changes the traces by {change:.2e}")
    assert change < 1e-10


def test_estimator_matches_exact_traces(exact_model):
    """N = 20000 host-drawn samples (generator seed 11), 30 steps of 0.1 (RK4 error of the harmonic flow ~1e-6, far below sigma).
    Measured on the CPU: max sigma_C 4.7e-3 (the bound against a vacuous pass is 0.01), max sigma_k 4.0e-3; largest deviation
    from the exact traces 5.8e-3 for C and 5.1e-3 for k (complex magnitude), 1.5 standard errors at the worst point and component.
    Without Phi: 0.13 for C, 26 standard errors."""
    m, tc, times, runs, args = exact_model
    C, K, _, _, sC, sK = runs[True]
    eC, eK = tcs.exact_traces(*args, m["kT"], times, BASIS)
    print(f"max sigma_C {abs(sC.real).max():.2e} {abs(sC.imag).max():.2e}, max sigma_k {abs(sK.real).max():.2e}; deviation "
          f"C {abs(C - eC).max():.2e} k {abs(K - eK).max():.2e}; worst {_worst(C, sC, eC):.2f} / {_worst(K, sK, eK):.2f} sigma")
    assert max(sC.real.max(), sC.imag.max()) <= 0.01                     # not a vacuous pass
    assert abs(eC[0] - 1.0) < 1e-10 and abs(C[0] - 1.0) <= 5 * sC.real[0]
    assert _within(C, sC, eC) and _within(K, sK, eK)


def test_without_the_phase_it_fails(exact_model):
    m, tc, times, runs, args = exact_model
    C, K, _, _, sC, sK = runs[False]
    eC, eK = tcs.exact_traces(*args, m["kT"], times, BASIS)
    print(f"without Phi: deviation C {abs(C - eC).max():.2e}, {_worst(C, sC, eC):.1f} sigma")
    assert not _within(C, sC, eC)
