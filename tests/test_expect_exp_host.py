"""Expectation values of operators with exp(-a.x) terms in the HK wavepacket, host side (no GPU): the
restatement of tests/expect_exp_cases.py against direct quadrature of psi^* A psi, the product columns of
hostmath.fold_exponential_operators against the direct formula, one Gaussian alone on a Morse surface, the refusals of the fold
and the interface."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import cases, expect_cases as EC, expect_exp_cases as XC
from tests.test_density_host import gaussian_wavefunction, overlap_constants
from tests.test_expect_host import _quadrature

torch.set_default_dtype(torch.float64)


def _fold(G, w, a):
    from semiclassical_amd import hostmath
    return tuple(t.numpy() for t in hostmath.fold_exponential_operators(torch.from_numpy(np.ascontiguousarray(w)),
                                                                        torch.from_numpy(np.ascontiguousarray(a, dtype=float)),
                                                                        torch.from_numpy(np.ascontiguousarray(G, dtype=float))))


def _quadrature_with_exponentials(q, p, v, G, ops, x, weight):
    """int psi^* A psi over the grid: the five parts by test_expect_host._quadrature, sum_e w_e exp(-a_e.x) as a potential"""
    M, D = len(ops["w"]), q.shape[0]
    c, m, K, n, W = EC.zeros_for(M, D, *(ops.get(k) for k in "cmKnW"))
    want, n2 = _quadrature(q, p, v, G, c, m, K, n, W, x, weight)
    rho = abs(gaussian_wavefunction(q, p, v, G, x)) ** 2
    pot = np.einsum('me,mex->mx', ops["w"], np.exp(-np.einsum('med,dx->mex', ops["a"], x)))
    return want + weight * (pot * rho[None]).sum(axis=1), n2


def _assert_meets_quadrature(q, p, v, G, ops, x, weight, label):
    want, n2 = _quadrature_with_exponentials(q, p, v, G, ops, x, weight)
    E, At, N2 = XC.restated_expectation(q, p, v, G, **ops)
    print(f"{label}: relative deviations", abs(E - want) / abs(want), abs(N2 - n2) / n2, "|E| / At", abs(E) / At)
    assert (abs(want) > 1e-2 * At).all()
    assert (abs(E - want) <= 1e-10 * abs(want)).all() and abs(N2 - n2) <= 1e-10 * n2
    # ... and the engine's product columns, summed over the pairs with the columns of the other parts, meet the same quadrature
    from tests.test_expect_host import _fold as fold_five
    M, D = len(ops["w"]), q.shape[0]
    five = fold_five(G, *EC.zeros_for(M, D, *(ops.get(k) for k in "cmKnW")))
    T, _, _ = EC.pair_terms(q, p, v, G)
    F = EC.folded_factors(q, p, five) + XC.folded_exponential_factors(q, p, _fold(G, ops["w"], ops["a"]))
    assert (abs((T[None] * F).sum(axis=(1, 2)) - want) <= 1e-10 * abs(want)).all()


# ------------------------------------------------------------------------------------------- 1. restatement against quadrature

def test_restatement_matches_quadrature_in_one_dimension():
    """exp(-a x) alone, and a Morse V = D (1 - exp(-a x))^2 as a constant and two exponentials"""
    rng = np.random.default_rng(31)
    G = np.array([[1.6]])
    q, p, v = rng.normal(0.0, 0.6, (1, 6)), rng.normal(0.0, 1.2, (1, 6)), rng.normal(size=6) + 1j * rng.normal(size=6)
    depth, rate = 2.5, 0.45
    ops = dict(c=np.array([0.0, depth]), w=np.array([[1.0, 0.0], [-2.0 * depth, depth]]),
               a=np.array([[[0.8], [0.0]], [[rate], [2.0 * rate]]]))
    x = np.linspace(-9.0, 9.0, 1441)[None, :]
    _assert_meets_quadrature(q, p, v, G, ops, x, x[0, 1] - x[0, 0], "D = 1")


def test_restatement_matches_quadrature_in_two_dimensions():
    """non-diagonal Gamma, non-zero momenta, a along non-axis vectors, mixed with x, xx, pp parts; 721^2 points on [-9, 9]^2"""
    rng = np.random.default_rng(32)
    G = np.array([[2.0, 0.5], [0.5, 1.4]])
    q, p, v = rng.normal(0.0, 0.6, (2, 5)), rng.normal(0.0, 1.2, (2, 5)), rng.normal(size=5) + 1j * rng.normal(size=5)
    ops = dict(c=np.array([0.7, 0.0]), m=np.array([[-0.4, 0.9], [0.0, 0.0]]),
               K=np.array([[[1.3, 0.8], [0.8, -0.9]], [[0.0, 0.0], [0.0, 0.0]]]),
               W=np.array([[[-0.7, 0.5], [0.5, 1.1]], [[0.0, 0.0], [0.0, 0.0]]]),
               w=np.array([[0.9, 1.4], [1.0, 0.0]]), a=np.array([[[0.5, -0.7], [-0.3, 0.4]], [[0.6, 0.35], [0.0, 0.0]]]))
    s = np.linspace(-9.0, 9.0, 721)
    x = np.stack([t.ravel() for t in np.meshgrid(s, s, indexing="ij")])
    _assert_meets_quadrature(q, p, v, G, ops, x, (s[1] - s[0]) ** 2, "D = 2")


# ------------------------------------------------------------------------------------------- 2. product columns against the direct formula

def _assert_fold_matches(q, p, G, w, a):
    fold = _fold(G, w, a)
    got, (want, _) = XC.folded_exponential_factors(q, p, fold), XC.exponential_sums(q, p, G, w, a)
    dev = abs(got - want) / np.maximum(1.0, abs(want))
    print(f"largest deviation {dev.max():.2e} of max(1, |F|), max |F| {abs(want).max():.3e}")
    assert dev.max() <= 1e-12
    return fold


def test_product_columns_match_the_direct_formula_dense():
    """D = 6, dense Gamma; real and complex weights, operators with 3, 1 and 0 terms in one set (w = 0: padding, whatever its a)"""
    rng = np.random.default_rng(33)
    D, nt = 6, 9
    Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    G = (Q * rng.uniform(0.5, 2.0, D)) @ Q.T
    G = 0.5 * (G + G.T)
    q, p = rng.normal(0.3, 0.8, (D, nt)), rng.normal(0.0, 1.0, (D, nt))
    a = rng.normal(0.0, 0.4, (3, 3, D))
    w = rng.standard_normal((3, 3))
    w[1, 1:], w[2] = 0.0, 0.0
    uq, up, mu = _assert_fold_matches(q, p, G, w, a)
    assert uq.shape == up.shape == (3, 3, D) and mu.shape == (3, 3) and uq.dtype == up.dtype == mu.dtype == np.complex128
    assert np.array_equal(uq[0], 0.5 * a[0]) and not up.real.any()
    assert not uq[2].any() and not up[2].any() and not mu[2].any() and not uq[1, 1:].any()
    _assert_fold_matches(q, p, G, w * (0.6 - 0.8j), a)
    empty = _fold(G, np.zeros((2, 0)), np.zeros((2, 0, D)))
    assert empty[0].shape == (2, 0, D) and empty[2].shape == (2, 0)


def test_product_columns_match_the_direct_formula_singular():
    """methylium's Gamma_t (rank 6 of 12 coordinates): every a projected onto its range"""
    rng = np.random.default_rng(34)
    G = cases.load("hk_methylium")["Gamma_t"]
    D, nt = G.shape[0], 7
    P = EC.projector(G)
    assert round(np.trace(P)) < D
    _, B, _, _ = overlap_constants(G)
    q, p = rng.normal(0.0, 0.5, (D, nt)), rng.normal(0.0, 1.0, (D, nt))
    a = (rng.standard_normal((2, 4, D)) @ P) / np.sqrt(np.trace(B))
    _assert_fold_matches(q, p, G, rng.standard_normal((2, 4)), a)


# ------------------------------------------------------------------------------------------- 3. one Gaussian on a Morse surface

def test_one_gaussian_on_a_morse_surface():
    """n = 1: <V_Morse> = sum_k D_k (1 - 2 exp(-a_k q_k + a_k^2 B_kk / 2) + exp(-2 a_k q_k + 2 a_k^2 B_kk)), from the product columns"""
    rng = np.random.default_rng(35)
    D = 4
    Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    G = (Q * rng.uniform(0.5, 2.0, D)) @ Q.T
    G = 0.5 * (G + G.T)
    B = np.linalg.inv(2.0 * G)
    q, p, v = rng.normal(0.3, 0.8, (D, 1)), rng.normal(0.0, 1.0, (D, 1)), np.array([0.7 - 0.4j])
    depth, rate = rng.uniform(1.0, 3.0, D), rng.uniform(0.2, 0.6, D)
    w, a = np.concatenate((-2.0 * depth, depth))[None], np.concatenate((np.diag(rate), np.diag(2.0 * rate)))[None]
    bkk = np.diag(B)
    want = np.sum(depth * (1.0 - 2.0 * np.exp(-rate * q[:, 0] + 0.5 * rate ** 2 * bkk) + np.exp(-2.0 * rate * q[:, 0] + 2.0 * rate ** 2 * bkk)))
    F = depth.sum() + XC.folded_exponential_factors(q, p, _fold(G, w, a))[0, 0, 0]
    assert abs(F - want) <= 1e-13 * np.sum(depth) and abs(F.imag) <= 1e-13 * np.sum(depth)
    E, _, N2 = XC.restated_expectation(q, p, v, G, c=np.array([depth.sum()]), w=w, a=a)
    assert abs(E[0] / N2 - want) <= 1e-13 * np.sum(depth)


# ------------------------------------------------------------------------------------------- 4. refusals of the fold

def test_fold_refusals():
    rng = np.random.default_rng(36)
    G = cases.load("hk_methylium")["Gamma_t"]
    D = G.shape[0]
    P = EC.projector(G)
    e, V = np.linalg.eigh(G)
    null = V[:, np.argmin(abs(e))]
    inside = P @ rng.standard_normal(D)
    inside /= 10.0 * np.linalg.norm(inside)
    for w, a in ((np.ones(2), np.ones((2, D))), (np.ones((1, 2)), np.ones((1, 2, D + 1))), (np.ones((1, 2)), np.ones((1, 3, D))),
                 (np.ones((2, 1)), np.ones((1, 1, D))), (np.ones((0, 1)), np.ones((0, 1, D))), (np.ones((1, 1)), np.ones((1, D)))):
        with pytest.raises(ValueError, match="operators: ex"):
            _fold(G, w, a)
    for w, a in ((np.array([[np.nan]]), inside[None, None]), (np.ones((1, 1)), np.full((1, 1, D), np.inf))):
        with pytest.raises(ValueError, match="non-finite"):
            _fold(G, w, a)
    tilted = inside + 1e-6 * np.linalg.norm(inside) * null
    a = np.stack([np.stack([inside, inside, inside]), np.stack([inside, inside, tilted])])
    with pytest.raises(ValueError, match="term 2 of operator 1 .* range of Gamma_t"):
        _fold(G, np.ones((2, 3)), a)
    with pytest.raises(ValueError, match="term 0 of operator 0 .* range of Gamma_t"):
        _fold(G, np.ones((1, 1)), null[None, None])
    w = np.ones((2, 3))
    w[1, 2] = 0.0
    uq, _, mu = _fold(G, w, a)                                 # a term of weight zero is padding, whatever its a
    assert not uq[1, 2].any() and mu[1, 2] == 0.0 and uq[1, 1].any()


# ------------------------------------------------------------------------------------------- 5. the interface

def test_symbol_is_declared_bound_and_exported():
    from semiclassical_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "semiclassical_hip.h")).read()
    assert re.search(r"^int sc_pair_expect_exp\(", header, re.M)
    assert "sc_pair_expect_exp" in _lib.SIGNATURES and hasattr(_lib.lib, "sc_pair_expect_exp")
    res, args = _lib.SIGNATURES["sc_pair_expect_exp"]
    plain = _lib.SIGNATURES["sc_pair_expect"][1]
    assert args == plain[:20] + [_lib.c_double_p, _lib.c_double_p, _lib.C.c_int32] + plain[20:]     # ... plus ea, eb, P
    assert int(re.search(r"#define SC_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.ABI_VERSION == _lib.lib.sc_abi_version() == 18


def test_signatures_of_the_methods():
    from semiclassical_amd import hostmath, propagators as PR
    for cls in (PR.HermanKlukPropagator, PR.WaltonManolopoulosPropagator):
        names = list(inspect.signature(cls.expectation).parameters)
        assert names == ["self", "c", "x", "xx", "p", "pp", "normalise", "ex"]
        assert inspect.signature(cls.expectation).parameters["ex"].default is None
    assert list(inspect.signature(PR.HermanKlukPropagator.anharmonic_energy_expectation).parameters) == ["self", "potential"]
    assert list(inspect.signature(hostmath.fold_exponential_operators).parameters) == ["w", "a", "Gamma_t"]
    assert PR.WaltonManolopoulosPropagator.expectation is not PR.HermanKlukPropagator.expectation
