"""Operator correlation functions <phi_0| A e^(-iHt) B |phi_0> with linear operators, host side (no GPU): a
numpy restatement of the two Gaussian matrix-element factors and of the term -- the reference of tests/test_opcorr_gpu.py --
against quadrature, the folded vectors the kernel takes, the closed form at t = 0 within the Monte-Carlo error, the result file's
pooling, the rates helpers and the C-ABI symbols."""
import os
import re
import types

import numpy as np
import pytest

from tests import cases
from tests.test_cross_host import ROUNDING, _random_spd, coherent_overlap, cross_terms, gaussian, initial_coefficients

ZERO = 1.0e-8          # eigenvalue threshold of the reference's pseudo-inverses (propagators.py:16)
HBAR = 1.0


# ------------------------------------------------------------------------------------------- the restatement

def pinv_sum(Ga, Gb):
    """((Ga + Gb)^+, the projector onto the range of Ga + Gb)"""
    e, V = np.linalg.eigh(Ga + Gb)
    keep = abs(e) > ZERO
    return (V[:, keep] / e[keep]) @ V[:, keep].T, V[:, keep] @ V[:, keep].T


def position_element(qa, pa, Ga, qb, pb, Gb):
    """<a|x|b> / <a|b> = (Ga + Gb)^+ (Ga qa + Gb qb + i (pb - pa) / hbar) for the bra |qa, pa, Ga> and the ket |qb, pb, Gb>;
    centres (D,) or (D, n), broadcast against each other"""
    S = pinv_sum(Ga, Gb)[0]
    col = lambda v: v if v.ndim == 2 else v[:, None]
    return S @ (Ga @ col(qa) + Gb @ col(qb) + 1j / HBAR * (col(pb) - col(pa)))


def ket_factors(c, m, q, p, Gi, G0, q0, p0):
    """g_ia = cB_a + mB_a.<q_i,p_i,Gi|x|phi_0> / <q_i,p_i,Gi|phi_0>, (n, M), from the initial points q, p (D, n)"""
    return c[None, :] + (m @ position_element(q, p, Gi, q0, p0, G0)).T


def bra_factors(c, m, Q, P, Gt, G0, q0, p0):
    """f_ia = cA_a + mA_a.<phi_0|x|Q_i,P_i,Gt> / <phi_0|Q_i,P_i,Gt>, (n, M), from the current points Q, P (D, n)"""
    return c[None, :] + (m @ position_element(q0, p0, G0, Q, P, Gt)).T


def restated_rows(x, kept=None):
    """the five columns (M, 5) of terms x (n, M): Re X, Im X, S_rr, S_ii, S_ri; ``kept`` (n,) bool: the trajectories that contribute"""
    if kept is not None:
        x = x[np.asarray(kept, dtype=bool)]
    return np.stack((x.real.sum(0), x.imag.sum(0), (x.real ** 2).sum(0), (x.imag ** 2).sum(0), (x.real * x.imag).sum(0)), axis=1)


def restated_opcorr(bra, ket, Q, P, q, p, cq, Gi, Gt, G0, q0, p0, kept=None):
    """rows (M, 5) of x_ia = f_ia g_ia cq_i (no dynamical phase)"""
    f = bra_factors(bra[0], bra[1], Q, P, Gt, G0, q0, p0)
    g = ket_factors(ket[0], ket[1], q, p, Gi, G0, q0, p0)
    return restated_rows(f * g * cq[:, None], kept)


def closed_form_t0(bra, ket, G0, q0):
    """X_a(0) = <phi_0|A_a B_a|phi_0> = (cA + mA.q0)(cB + mB.q0) + 1/2 mA^T G0^+ mB"""
    e, V = np.linalg.eigh(G0)
    keep = abs(e) > ZERO
    iG0 = (V[:, keep] / e[keep]) @ V[:, keep].T
    return (bra[0] + bra[1] @ q0) * (ket[0] + ket[1] @ q0) + 0.5 * np.einsum('ad,de,ae->a', bra[1], iG0, ket[1])


def project(m, Ga, Gb):
    """rows of m projected onto the range of Ga + Gb"""
    return m @ pinv_sum(Ga, Gb)[1]


def t0_operator_pairs(D):
    """the three pairs of the 5 sigma checks (this file and test_opcorr_gpu.py): x_0 with x_0, x_0 with x_4, and a mixed pair with
    constants on both sides"""
    e = np.eye(D)
    mixed_a, mixed_b = 0.5 * e[1] - 0.25 * e[3] + 0.1 * e[0], 0.3 * e[2] + 0.2 * e[1] - 0.15 * e[4]
    bra = (np.array([0.0, 0.0, 0.7]), np.array([e[0], e[0], mixed_a]))
    ket = (np.array([0.0, 0.0, -1.3]), np.array([e[0], e[4], mixed_b]))
    return bra, ket


# ------------------------------------------------------------------------------------------- 1. matrix element vs quadrature

@pytest.mark.parametrize("D", [1, 2])
def test_matrix_element_matches_quadrature(D):
    """int phi_a^*(x) (m.x) phi_b(x) dx by the trapezoid rule (spectrally accurate for Gaussians: the grid reaches 9 widths beyond
    every centre at 25 points per width) against m.(Ga + Gb)^+ (...) <a|b>"""
    rng = np.random.default_rng(20 + D)
    Ga, Gb = _random_spd(rng, D), _random_spd(rng, D)          # D = 2: non-diagonal, Gamma_a != Gamma_b
    qa, qb = rng.normal(0.0, 0.8, D), rng.normal(0.0, 0.8, D)
    pa, pb = rng.normal(0.0, 1.2, D), rng.normal(0.0, 1.2, D)
    m = rng.normal(size=(3, D))
    axis = np.arange(-14.0, 14.0 + 1e-9, 0.04)
    x = np.stack([a.ravel() for a in np.meshgrid(*([axis] * D), indexing="ij")])
    weight = np.conj(gaussian(qa, pa, Ga, x)) * gaussian(qb, pb, Gb, x) * 0.04 ** D
    quad = (m @ x) @ weight
    overlap = coherent_overlap(qa, pa, Ga, qb, pb, Gb)
    assert abs(weight.sum() - overlap) <= 1e-12 * abs(overlap)
    closed = (m @ position_element(qa, pa, Ga, qb, pb, Gb))[:, 0] * overlap
    dev = abs(closed - quad) / abs(closed)
    print(f"D = {D}: |<a|m.x|b>| {np.array2string(abs(closed), precision=3)}, deviation from quadrature {dev.max():.2e} of the value")
    assert (dev <= 1e-10).all()


# ------------------------------------------------------------------------------------------- 2. folded vectors

def _folded_deviation(Gi, Gt, G0, q0, p0, q, p, c, m):
    """largest deviation of kappa + u.Q + i w.P (hostmath.fold_linear_operators) from the direct formula, bra and ket side"""
    import torch
    from semiclassical_amd import hostmath
    t = lambda a: torch.from_numpy(np.array(a, dtype=np.float64))
    worst = 0.0
    for ket, G in ((False, Gt), (True, Gi)):
        u, w, kap = (a.numpy() for a in hostmath.fold_linear_operators(t(c), t(m), t(G), t(G0), t(q0), t(p0), ket=ket))
        assert u.shape == w.shape == m.shape and kap.shape == c.shape and kap.dtype == np.complex128
        folded = kap[None, :] + (u @ q).T + 1j * (w @ p).T
        direct = ket_factors(c, m, q, p, G, G0, q0, p0) if ket else bra_factors(c, m, q, p, G, G0, q0, p0)
        worst = max(worst, (abs(folded - direct) / np.maximum(1.0, abs(direct))).max())
    return worst


def test_folded_vectors_dense():
    rng = np.random.default_rng(6)
    D, n, M = 6, 9, 4
    Gi, Gt, G0 = _random_spd(rng, D), _random_spd(rng, D), _random_spd(rng, D)
    dev = _folded_deviation(Gi, Gt, G0, rng.normal(0.0, 0.8, D), rng.normal(0.0, 1.2, D), rng.normal(0.0, 0.8, (D, n)),
                            rng.normal(0.0, 1.2, (D, n)), rng.normal(size=M), rng.normal(size=(M, D)))
    print(f"dense D = {D}: folded against direct factor {dev:.2e}")
    assert dev <= 1e-12


def test_folded_vectors_singular_widths():
    """methylium's Cartesian widths are singular (rank 6 of 12): the pseudo-inverse, m projected onto the range"""
    g = cases.load("hk_methylium")
    Gi, Gt, G0 = g["Gamma_i"], g["Gamma_t"], g["Gamma_0"]
    D = Gt.shape[0]
    assert np.count_nonzero(abs(np.linalg.eigvalsh(Gt + G0)) > ZERO) < D
    rng = np.random.default_rng(7)
    m = project(rng.normal(size=(4, D)), Gt, G0)
    dev = _folded_deviation(Gi, Gt, G0, g["q0"], g["p0"], g["zi"][:D, :16], g["zi"][D:, :16], rng.normal(size=4), m)
    print(f"methylium: folded against direct factor {dev:.2e}")
    assert dev <= 1e-12


def test_vector_outside_the_range_is_refused():
    import torch
    from semiclassical_amd import hostmath
    g = cases.load("hk_methylium")
    t = lambda a: torch.from_numpy(np.array(a, dtype=np.float64))
    Gt, G0 = g["Gamma_t"], g["Gamma_0"]
    D = Gt.shape[0]
    e, V = np.linalg.eigh(Gt + G0)
    null = V[:, abs(e) <= ZERO][:, 0]
    inside = project(np.random.default_rng(1).normal(size=(2, D)), Gt, G0)
    args = (t(Gt), t(G0), t(g["q0"]), t(g["p0"]))
    hostmath.fold_linear_operators(t(np.zeros(2)), t(inside), *args, ket=False)
    hostmath.fold_linear_operators(t(np.ones(1)), t(np.zeros((1, D))), *args, ket=True)         # m = 0 (a constant) is inside
    for ket in (False, True):
        with pytest.raises(ValueError, match=r"\[1\]"):
            hostmath.fold_linear_operators(t(np.zeros(2)), t(np.vstack((inside[0], inside[1] + 1e-6 * np.linalg.norm(inside[1]) * null))),
                                           *args, ket=ket)


# ------------------------------------------------------------------------------------------- 3. the 5 sigma check, on the CPU

def initial_terms(g):
    """cq_i of t = 0 from the fixture's own initial conditions (Gamma_i = Gamma_t: the prefactor of t = 0 is 1):
    <phi_0|q_i,p_i,Gamma_t> <q_i,p_i,Gamma_i|phi_0> / (N (2 pi hbar)^D P_i)"""
    assert np.array_equal(g["Gamma_i"], g["Gamma_t"])
    D = g["q0"].shape[0]
    return cross_terms(g["zi"][:D], g["zi"][D:], initial_coefficients(g), g["Gamma_t"], g["Gamma_0"], g["q0"][None, :], g["p0"][None, :])[:, 0]


def within_five_sigma(X, sigma, exact):
    """|X - exact| <= 5 sigma, real and imaginary parts apart.  A pair with the same operator on both sides is degenerate in its
    imaginary part at t = 0 for Gamma_i = Gamma_t: g_i = conj(f_i) and cq_i > 0, so every Im x_i is zero up to rounding, and so are
    Im X and sigma_Im -- the comparison cannot resolve below the arithmetic, hence the floor of test_cross_host.py (ROUNDING, for
    sums of N terms of magnitude 1/N), scaled to the terms' magnitude |exact| / N here (it plays no part for sigma ~ 1)."""
    d = X - exact
    floor = ROUNDING * np.maximum(1.0, abs(exact))
    return (abs(d.real) <= 5.0 * sigma.real + floor) & (abs(d.imag) <= 5.0 * sigma.imag + floor)


def test_five_sigma_at_t0_on_the_cpu():
    """the restatement on the fixture's (zi, probi) at t = 0 lies within 5 sigma of <phi_0|A B|phi_0> for the three pairs of the GPU
    test (test_opcorr_gpu.py::test_standard_errors_cover_the_closed_form)"""
    from semiclassical_amd import hostmath
    g = cases.load("hk_as5_chi002")
    D, n = g["q0"].shape[0], g["zi"].shape[1]
    q, p = g["zi"][:D], g["zi"][D:]
    bra, ket = t0_operator_pairs(D)
    rows = restated_opcorr(bra, ket, q, p, q, p, initial_terms(g), g["Gamma_i"], g["Gamma_t"], g["Gamma_0"], g["q0"], g["p0"])
    X = rows[:, 0] + 1j * rows[:, 1]
    sigma = hostmath.standard_errors(X, rows[:, 2:5], n)
    exact = closed_form_t0(bra, ket, g["Gamma_0"], g["q0"])
    for a in range(3):
        print(f"pair {a}: X {X[a]:.6f}  exact {exact[a]:.6f}  sigma {sigma[a]:.2e}  |dev| / sigma "
              f"{abs((X - exact)[a].real) / sigma[a].real:.2f}, {abs((X - exact)[a].imag) / max(sigma[a].imag, 1e-300):.2f}")
    assert (sigma.real > 0.01 * abs(exact)).all() and (sigma.real < 0.5 * abs(exact)).all()      # error bars that mean something
    assert within_five_sigma(X, sigma, exact).all()


# ------------------------------------------------------------------------------------------- 4. plumbing

def _batch(rng, nt, M, n):
    """raw rows (nt, M, 5) of a batch of n terms per step and operator pair, with the weight 1/n inside the terms"""
    x = (rng.normal(size=(nt, M, n)) + 1j * rng.normal(size=(nt, M, n))) / n
    return np.stack((x.real.sum(2), x.imag.sum(2), (x.real ** 2).sum(2), (x.imag ** 2).sum(2), (x.real * x.imag).sum(2)), axis=2), x


def test_finalize_cross_on_opcorr_rows():
    """the rows are the rows of section 4.13: finalize_cross applies unchanged"""
    from semiclassical_amd import hostmath
    from semiclassical_amd.propagators import HermanKlukPropagator as HK
    rng = np.random.default_rng(3)
    nt, M, n, t0, dt, E0 = 4, 3, 50, 0.7, 0.3, 0.9
    raw, x = _batch(rng, nt, M, n)
    X, sigma = HK.finalize_cross(raw, t0, dt, E0, n)
    phased = x * np.exp(1j * (t0 + hostmath.time_grid(nt, dt)) * E0 / HBAR)[:, None, None]
    assert X.shape == sigma.shape == (nt, M) and np.allclose(X, phased.sum(2), rtol=1e-13, atol=0)
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


def _operators(rng, M, D):
    return {"bra_c": rng.normal(size=M), "bra_m": rng.normal(size=(M, D)), "ket_c": rng.normal(size=M), "ket_m": rng.normal(size=(M, D))}


def _record(rng, nt, ops, n, errors=True):
    raw, x = _batch(rng, nt, ops["bra_c"].shape[0], n)
    rec = dict(ops, correlation=raw[:, :, 0] + 1j * raw[:, :, 1])
    if errors:
        rec["second_moment"] = n * raw[:, :, 2:5]
    return np.ones(nt, dtype=complex), rec, x


def test_store_pools_batches(tmp_path):
    """two batches pooled equal one batch of both: means with the weights of the autocorrelation, errors from the pooled moments"""
    from semiclassical_amd import hostmath
    rng = np.random.default_rng(4)
    nt, M, D, n1, n2 = 3, 4, 2, 30, 50
    ops = _operators(rng, M, D)
    a1, r1, x1 = _record(rng, nt, ops, n1)
    a2, r2, x2 = _record(rng, nt, ops, n2)
    store = _store(tmp_path, "two.npz", nt)
    store.add_batch(a1, a1, n1, operators=r1)
    store.add_batch(a2, a2, n2, operators=r2)
    got = dict(np.load(store.path))
    n = n1 + n2
    x = np.concatenate((n1 * x1, n2 * x2), axis=2) / n
    assert all(np.array_equal(got["operator_" + key], ops[key]) for key in ops)
    assert got["operator_correlation"].shape == (nt, M)
    assert np.allclose(got["operator_correlation"], x.sum(2), rtol=1e-13, atol=0)
    m3 = np.stack(((x.real ** 2).sum(2), (x.imag ** 2).sum(2), (x.real * x.imag).sum(2)), axis=2)
    assert np.allclose(got["operator_correlation_second_moment"], n * m3, rtol=1e-12, atol=0)
    assert np.allclose(got["operator_correlation_error"], hostmath.standard_errors(x.sum(2), m3, n), rtol=1e-10, atol=0)
    assert int(got["trajectories"]) == n
    # a batch without moments: the error keys go, the means stay (the keep-or-drop rule of the moments)
    a3, r3, _ = _record(rng, nt, ops, 20, errors=False)
    store.add_batch(a3, a3, 20, operators=r3)
    got = np.load(store.path)
    assert "operator_correlation" in got and "operator_correlation_error" not in got and "operator_correlation_second_moment" not in got


def test_store_refuses_other_operators(tmp_path):
    import torch
    from semiclassical_amd import driver
    rng = np.random.default_rng(8)
    nt, M, D = 3, 2, 2
    ops = _operators(rng, M, D)
    store = _store(tmp_path, "other.npz", nt)
    a, r, _ = _record(rng, nt, ops, 20)
    store.add_batch(a, a, 20, operators=r)
    before = dict(np.load(store.path))
    others = [dict(r, bra_c=ops["bra_c"] + 1e-9), dict(r, ket_m=ops["ket_m"][::-1].copy()),
              dict(r, **{key: ops[key][:1] for key in ops}, correlation=r["correlation"][:, :1]), None]
    for other in others:
        with pytest.raises(driver.ConfigurationError):
            store.add_batch(a, a, 20, operators=other)
    plain = _store(tmp_path, "plain.npz", nt)
    plain.add_batch(a, a, 20)
    with pytest.raises(driver.ConfigurationError):
        plain.add_batch(a, a, 20, operators=r)
    after = dict(np.load(store.path))
    assert set(before) == set(after) and all(np.array_equal(before[k], after[k]) for k in before)
    # start() refuses before any trajectory runs
    task = {"results": {"overwrite": False}}
    same = tuple(ops[key] for key in ("bra_c", "bra_m", "ket_c", "ket_m"))
    with pytest.raises(driver.ConfigurationError):
        store.start(task, "HK", torch.linspace(0.0, 1.0, nt), None, operators=(same[0] + 1.0,) + same[1:])
    with pytest.raises(driver.ConfigurationError):
        store.start(task, "HK", torch.linspace(0.0, 1.0, nt), None)
    store.start(task, "HK", torch.linspace(0.0, 1.0, nt), None, operators=same)


def test_store_without_the_key_has_todays_keys(tmp_path):
    store = _store(tmp_path, "none.npz", 3)
    a = np.ones(3, dtype=complex)
    store.add_batch(a, a, 10)
    assert set(np.load(store.path).keys()) == {"propagator", "times", "autocorrelation", "ic_correlation", "adiabatic_gap",
                                               "zero_point_energy", "trajectories"}


def test_driver_refuses_wm_and_bad_files(tmp_path):
    from semiclassical_amd import driver
    task = {"task": "dynamics", "propagator": "WM", "operator_correlation": str(tmp_path / "t.npz"), "potential": {"type": "none"}}
    with pytest.raises(driver.ConfigurationError, match="WM"):
        driver.run_semiclassical_dynamics(task)
    np.savez(tmp_path / "ok.npz", bra_c=np.zeros(2), bra_m=np.ones((2, 3)))
    bra_c, bra_m, ket_c, ket_m = driver._load_operators(str(tmp_path / "ok.npz"), 3)
    assert np.array_equal(ket_c, bra_c) and np.array_equal(ket_m, bra_m) and bra_m.shape == (2, 3)
    bad = {"t": dict(bra_c=np.zeros(2), bra_m=np.zeros((2, 4))), "u": dict(bra_c=np.zeros(2)),
           "v": dict(bra_c=np.zeros(2), bra_m=np.full((2, 3), np.nan)), "w": dict(bra_c=np.zeros(0), bra_m=np.zeros((0, 3))),
           "x": dict(bra_c=np.zeros(2), bra_m=np.zeros((2, 3)), ket_c=np.zeros(2)),
           "y": dict(bra_c=np.zeros(2), bra_m=np.zeros((2, 3)), ket_c=np.zeros(3), ket_m=np.zeros((3, 3)))}
    for name, arrays in bad.items():
        np.savez(tmp_path / f"{name}.npz", **arrays)
        with pytest.raises(driver.ConfigurationError):
            driver._load_operators(str(tmp_path / f"{name}.npz"), 3)


def test_shape_refusals():
    """the validation of one side's (c, m), without a device"""
    from semiclassical_amd.propagators import HermanKlukPropagator as HK
    D = 3
    stub = types.SimpleNamespace(dim=D, _is_operator_set=HK._is_operator_set)
    c, m = HK._operator_set(stub, "bra", ([1.0, 2.0], np.ones((2, D))))
    assert tuple(c.shape) == (2,) and tuple(m.shape) == (2, D)
    bad_m = np.ones((2, D))
    bad_m[1, 1] = np.inf
    for ops in ((np.zeros(2), np.zeros((2, D + 1))), (np.zeros(3), np.zeros((2, D))), (np.zeros((2, 1)), np.zeros((2, D))),
                (np.zeros(2), np.zeros(D)), (np.zeros(0), np.zeros((0, D))), (np.zeros(2), bad_m), (np.full(2, np.nan), np.ones((2, D))),
                np.zeros(2), (np.zeros(2),), None):
        with pytest.raises(ValueError):
            HK._operator_set(stub, "bra", ops)


def test_propagators_offer_operator_correlation():
    import inspect
    from semiclassical_amd import propagators as PR
    assert callable(PR.HermanKlukPropagator.operator_correlation)
    sig = inspect.signature(PR.HermanKlukPropagator.operator_correlation).parameters
    assert list(sig)[1:] == ["bra", "ket", "energy0_es", "standard_errors"] and sig["ket"].default is None
    run = inspect.signature(PR.HermanKlukPropagator.run).parameters
    assert "operators" in run and "opcorr" in run and run["operators"].default is None and run["opcorr"].default is None
    assert PR.WaltonManolopoulosPropagator._opcorr_ok is False and PR.HermanKlukPropagator._opcorr_ok is True


def test_step_rows_carry_the_opcorr_buffer():
    """the buffer is a trailing keyword of _StepRows and a trailing field of _Row; the positional signature keeps its places"""
    import torch
    from semiclassical_amd.propagators import _Row, _StepRows
    assert _Row._fields == ("slot", "moments", "blocks", "cross", "slots", "k", "opcorr")
    nt, M = 3, 4
    slots, buf = torch.zeros((nt, 5), dtype=torch.float64), torch.zeros((nt + 2, M, 5), dtype=torch.float64)
    rows = _StepRows(torch.device("cpu"), nt, slots, opcorr=buf, M=M)
    for k in range(nt):
        assert rows.row(k).opcorr == buf.data_ptr() + 40 * M * k and rows.row(k).cross is None
    assert _StepRows(torch.device("cpu"), nt, slots).row(1).opcorr is None
    assert _StepRows.single(opcorr=buf).opcorr == buf.data_ptr()
    for bad in (buf[:nt - 1], torch.zeros((nt, M + 1, 5), dtype=torch.float64), torch.zeros((nt, M, 5), dtype=torch.float32)):
        with pytest.raises(ValueError, match="opcorr"):
            _StepRows(torch.device("cpu"), nt, slots, opcorr=bad, M=M)


# ------------------------------------------------------------------------------------------- 5. rates helpers

def test_lineshape_sums_to_the_value_at_t0():
    """sum_E G(E) dE = f(0) C(0): the discrete transform is exact for the zero-time element (the cos^2 switch is 1 there)"""
    from semiclassical_amd import broadening, rates
    rng = np.random.default_rng(9)
    nt = 64
    times = np.linspace(0.0, 300.0, nt)
    C = (rng.normal(size=nt) + 1j * rng.normal(size=nt)) * np.exp(-times / 80.0)
    C[0] = 0.8 + 0.0j
    shape = broadening.gaussian(0.02)
    energies, G = rates.lineshape_from_correlation(times, C, shape)
    e2, k = rates.rate_from_correlation(times, C, shape)
    assert np.array_equal(energies, e2) and G.shape == k.shape == (2 * nt - 1,)
    total = G.sum() * (energies[1] - energies[0])
    want = C[0] * shape(np.zeros(1))[0]
    print(f"sum G dE = {total:.15f}, f(0) C(0) = {want:.15f}")
    assert abs(total - want) <= 1e-12
    # the same transform as the rate's, without the conversion to s^-1 and with the 1 / (2 pi hbar) of the definition
    from semiclassical_amd import units
    assert np.allclose(k, 2.0 * np.pi * G * 1.0e15 / units.autime_to_fs, rtol=1e-14, atol=0)


def test_radiative_rate_of_a_gaussian_lineshape():
    """G(gap - eps) = mu^2 N(eps; E_c, s): int eps^3 N = E_c^3 + 3 E_c s^2, so k_r = 4 / (3 c^3) mu^2 (E_c^3 + 3 E_c s^2).

    The grid: E from gap - E_c - 10 s to gap - E_c + 10 s at spacing h = s / 4 (81 points); eps = gap - E stays above
    E_c - 10 s = 0.06 > 0, so nothing is cut at eps = 0.  The error of the trapezoid rule for an integrand polynomial x Gaussian
    on the whole line is of the order exp(-2 pi^2 s^2 / h^2) = exp(-316): nothing.  What remains is the truncation: the tails
    beyond 10 s hold erfc(10 / sqrt 2) = 1.5e-23 of the weight, times (1 + 10 s / E_c)^3 < 5 for eps^3: < 1e-22 relative.  The
    bound is therefore rounding alone: 81 terms of relative error 2^-52 each in the products and the sum, < 81 x 4 x 2.2e-16 =
    7e-14; asserted 1e-13."""
    from semiclassical_amd import rates, units
    mu2, Ec, s, gap = 0.37, 0.1, 0.004, 0.15
    E = (gap - Ec) + s / 4.0 * np.arange(-40, 41)
    eps = gap - E
    G = mu2 * np.exp(-0.5 * ((eps - Ec) / s) ** 2) / (s * np.sqrt(2.0 * np.pi))
    want = 4.0 / (3.0 * units.speed_of_light ** 3) * mu2 * (Ec ** 3 + 3.0 * Ec * s ** 2) * 1.0e15 / units.autime_to_fs
    got = rates.radiative_rate(E, G, gap)
    shuffled = np.random.default_rng(0).permutation(E.shape[0])
    print(f"k_r = {got:.6e} s^-1, closed form {want:.6e} s^-1, deviation {abs(got - want) / want:.2e}")
    assert abs(got - want) <= 1e-13 * want
    assert rates.radiative_rate(E[shuffled], G[shuffled], gap) == got                 # any order of the grid
    # photon energies at or below zero do not count
    assert rates.radiative_rate(E, G, gap - Ec - 20 * s) == 0.0
    assert abs(units.speed_of_light - 137.036) < 1e-3


def test_rates_task_writes_the_lineshapes(tmp_path):
    """the rates task: operator_lineshape (nE, M) on the energies it writes, radiative_rate with "adiabatic_gap_ev"; ic_rate and the
    other keys as without the operators"""
    from semiclassical_amd import driver, rates, units
    rng = np.random.default_rng(12)
    nt, M = 32, 2
    times = np.linspace(0.0, 400.0, nt)
    k = (rng.normal(size=nt) + 1j * rng.normal(size=nt)) * np.exp(-times / 90.0)
    X = (rng.normal(size=(nt, M)) + 1j * rng.normal(size=(nt, M))) * np.exp(-times / 90.0)[:, None]
    base = dict(propagator="HK", times=times, autocorrelation=k, ic_correlation=k, trajectories=10)
    np.savez(tmp_path / "plain.npz", **base)
    np.savez(tmp_path / "ops.npz", **base, operator_correlation=X)
    for name in ("plain", "ops"):
        driver.calculate_rates({"correlations": str(tmp_path / f"{name}.npz"), "rates": str(tmp_path / f"{name}_rates.npz"),
                                "adiabatic_gap_ev": 3.0})
    plain, ops = dict(np.load(tmp_path / "plain_rates.npz")), dict(np.load(tmp_path / "ops_rates.npz"))
    assert set(ops) == set(plain) | {"operator_correlation", "operator_lineshape", "radiative_rate"}
    assert all(np.array_equal(plain[key], ops[key]) for key in plain)
    assert "operator_lineshape" not in plain and "radiative_rate" not in plain
    nE = ops["energies"].shape[0]
    assert ops["operator_lineshape"].shape == (nE, M) and ops["operator_lineshape"].dtype == np.float64
    lineshape, _ = driver.lineshape_from_task({})
    energies, G = rates.lineshape_from_correlation(times, X[:, 1], lineshape)
    assert np.array_equal(ops["operator_lineshape"][:, 1], G[energies >= 0.0].real)
    want = rates.radiative_rate(ops["energies"], ops["operator_lineshape"].sum(1), 3.0 / units.hartree_to_ev)
    assert float(ops["radiative_rate"]) == want
    # without the gap: the lineshapes only
    driver.calculate_rates({"correlations": str(tmp_path / "ops.npz"), "rates": str(tmp_path / "nogap.npz")})
    nogap = np.load(tmp_path / "nogap.npz")
    assert "operator_lineshape" in nogap and "radiative_rate" not in nogap


# ------------------------------------------------------------------------------------------- 6. ABI

def test_symbols_are_declared_bound_and_exported():
    from semiclassical_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "semiclassical_hip.h")).read()
    for name in ("sc_hk_opcorr", "sc_hk_opcorr_initial", "sc_hk_opcorr_rows"):
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    assert int(re.search(r"#define SC_ABI_VERSION\s+(\d+)", header).group(1)) == 18
    assert _lib.lib.sc_abi_version() == _lib.ABI_VERSION == 18
    rows = _lib.lib.sc_hk_opcorr_rows
    assert rows(1, 1) == 1 and rows(64, 500) == 1 and rows(65, 1) == 2 and rows(130, 65) == 3
    assert rows(0, 5) == 0 and rows(5, 0) == 0
