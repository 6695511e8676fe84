"""Expectation values of quadratic operators in the HK wavepacket, host side (no GPU): the restatement of
tests/expect_cases.py against direct quadrature of psi^* A psi, the folded columns of hostmath.fold_expectation_operators against the
direct formula, the refusals of the fold, and one Gaussian alone."""
import numpy as np
import pytest
import torch

from tests import cases, expect_cases as EC
from tests.test_density_host import HBAR, ZERO, gaussian_wavefunction

torch.set_default_dtype(torch.float64)


def _fold(G, c=None, m=None, K=None, n=None, W=None):
    from semiclassical_amd import hostmath
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=float))
    return tuple(r.numpy() if torch.is_tensor(r) else r for r in hostmath.fold_expectation_operators(t(c), t(m), t(K), t(n), t(W), t(G)))


def _gradient_of_wavefunction(q, p, v, G, x):
    """(-i hbar d/dx_a psi)(x) (D, nx): sum_i v_i (p_i + i hbar G (x - q_i)) g_i(x), the analytic gradient of the Gaussians"""
    e = np.linalg.eigvalsh(G)
    keep = abs(e) > ZERO
    fac = (np.prod(e[keep]) / np.pi ** int(np.count_nonzero(keep))) ** 0.25
    dx = x[:, None, :] - q[:, :, None]                  # (D, n, nx)
    g = fac * np.exp(-0.5 * np.einsum('anx,ab,bnx->nx', dx, G, dx) + 1j / HBAR * np.einsum('an,anx->nx', p, dx))
    return np.einsum('n,anx,nx->ax', v, p[:, :, None] + 1j * HBAR * np.einsum('ab,bnx->anx', G, dx), g)


def _quadrature(q, p, v, G, c, m, K, n, W, x, weight):
    """int psi^* A psi over the grid x (D, nx) of cell volume `weight`; <psi| p^T W p |psi> = <p psi| W |p psi> (parts)"""
    psi, ppsi = gaussian_wavefunction(q, p, v, G, x), _gradient_of_wavefunction(q, p, v, G, x)
    rho = abs(psi) ** 2
    out = np.empty(len(c), dtype=complex)
    for a in range(len(c)):
        pot = c[a] + m[a] @ x + 0.5 * np.einsum('ax,ab,bx->x', x, K[a], x)
        out[a] = weight * (np.sum(pot * rho) + np.sum(np.conj(psi) * (n[a] @ ppsi))
                           + 0.5 * np.sum(np.einsum('ax,ab,bx->x', np.conj(ppsi), W[a], ppsi)))
    return out, weight * rho.sum()


# ------------------------------------------------------------------------------------------- 1. restatement against quadrature

def _assert_folded_sum(q, p, v, G, parts, want):
    """... and the columns of the engine's fold, summed over the pairs, meet the same quadrature"""
    T, _, _ = EC.pair_terms(q, p, v, G)
    E = (T[None] * EC.folded_factors(q, p, _fold(G, *parts))).sum(axis=(1, 2))
    assert (abs(E - want) <= 1e-10 * abs(want)).all()


def test_restatement_matches_quadrature_in_one_dimension():
    rng = np.random.default_rng(11)
    G = np.array([[1.6]])
    q, p, v = rng.normal(0.0, 0.6, (1, 6)), rng.normal(0.0, 1.2, (1, 6)), rng.normal(size=6) + 1j * rng.normal(size=6)
    c, m, K, n, W = (np.array([0.7, 0.0]), np.array([[-0.4], [1.0]]), np.array([[[1.3]], [[0.0]]]), np.array([[0.9], [0.0]]),
                     np.array([[[-0.8]], [[2.0]]]))
    x = np.linspace(-9.0, 9.0, 1441)[None, :]
    want, n2 = _quadrature(q, p, v, G, c, m, K, n, W, x, x[0, 1] - x[0, 0])
    E, A, N2 = EC.restated_expectation(q, p, v, G, c, m, K, n, W)
    print("D = 1: relative deviations", abs(E - want) / abs(want), abs(N2 - n2) / n2)
    assert (abs(want) > 1e-2 * A).all()
    assert (abs(E - want) <= 1e-10 * abs(want)).all() and abs(N2 - n2) <= 1e-10 * n2
    _assert_folded_sum(q, p, v, G, (c, m, K, n, W), want)


def test_restatement_matches_quadrature_in_two_dimensions():
    """non-diagonal Gamma, non-zero momenta, an indefinite K and W, all five parts non-zero; 721^2 points on [-9, 9]^2"""
    rng = np.random.default_rng(12)
    G = np.array([[2.0, 0.5], [0.5, 1.4]])
    q, p, v = rng.normal(0.0, 0.6, (2, 5)), rng.normal(0.0, 1.2, (2, 5)), rng.normal(size=5) + 1j * rng.normal(size=5)
    c, m, n = np.array([0.7, 0.0]), np.array([[-0.4, 0.9], [0.0, 0.0]]), np.array([[0.6, -1.1], [0.3, 0.2]])
    K = np.array([[[1.3, 0.8], [0.8, -0.9]], [[0.0, 0.0], [0.0, 0.0]]])
    W = np.array([[[-0.7, 0.5], [0.5, 1.1]], [[1.0, 0.0], [0.0, 1.0]]])
    assert np.linalg.eigvalsh(K[0]).prod() < 0 and np.linalg.eigvalsh(W[0]).prod() < 0
    s = np.linspace(-9.0, 9.0, 721)
    x = np.stack([a.ravel() for a in np.meshgrid(s, s, indexing="ij")])
    want, n2 = _quadrature(q, p, v, G, c, m, K, n, W, x, (s[1] - s[0]) ** 2)
    E, A, N2 = EC.restated_expectation(q, p, v, G, c, m, K, n, W)
    print("D = 2: relative deviations", abs(E - want) / abs(want), abs(N2 - n2) / n2)
    assert (abs(want) > 1e-2 * A).all()
    assert (abs(E - want) <= 1e-10 * abs(want)).all() and abs(N2 - n2) <= 1e-10 * n2
    _assert_folded_sum(q, p, v, G, (c, m, K, n, W), want)


# ------------------------------------------------------------------------------------------- 2. folded columns against the direct formula

def _assert_fold_matches(q, p, G, parts):
    c, m, K, n, W = parts
    fold = _fold(G, c, m, K, n, W)
    got, want = EC.folded_factors(q, p, fold), EC.pair_factors(q, p, G, *EC.zeros_for(len(fold[3]), G.shape[0], c, m, K, n, W))
    dev = abs(got - want) / np.maximum(1.0, abs(want))
    print(f"R = {fold[4]}, largest deviation {dev.max():.2e} of max(1, |F|), max |F| {abs(want).max():.3e}")
    assert dev.max() <= 1e-12
    return fold


def test_folded_columns_match_the_direct_formula_dense():
    """D = 6, dense Gamma; K of ranks 0, 1, 3, 6 and W of ranks 6, 3, 1, 0 in one set: R = 6, the shorter operators padded"""
    rng = np.random.default_rng(13)
    D, nt = 6, 9
    Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    G = (Q * rng.uniform(0.5, 2.0, D)) @ Q.T
    G = 0.5 * (G + G.T)
    q, p = rng.normal(0.3, 0.8, (D, nt)), rng.normal(0.0, 1.0, (D, nt))
    ranks = [0, 1, 3, 6]
    K = np.stack([EC.symmetric(rng, D, r) for r in ranks])
    W = np.stack([EC.symmetric(rng, D, r) for r in ranks[::-1]])
    c, m, n = rng.standard_normal(4), rng.standard_normal((4, D)), rng.standard_normal((4, D))
    uq, up, lam, kappa, R = _assert_fold_matches(q, p, G, (c, m, K, n, W))
    assert R == 6 and uq.shape == up.shape == (4, 7, D) and lam.shape == (4, 7) and kappa.shape == (4,)
    assert (lam[:, 0] == 1.0).all() and np.count_nonzero(lam[:, 1:], axis=1).tolist() == [6, 4, 4, 6]
    # any of the five parts may be missing
    for drop in range(5):
        parts = [c, m, K, n, W]
        parts[drop] = None
        _assert_fold_matches(q, p, G, parts)
    fold = _assert_fold_matches(q, p, G, (None, None, K[1:2], None, None))
    assert fold[4] == 1
    fold = _assert_fold_matches(q, p, G, (c, None, None, None, None))
    assert fold[4] == 0 and not fold[0].any() and not fold[1].any() and np.array_equal(fold[3], c.astype(complex))


def test_folded_columns_match_the_direct_formula_singular():
    """methylium's Gamma_t (rank 6 of 12 coordinates): every vector and matrix projected onto its range"""
    rng = np.random.default_rng(14)
    G = cases.load("hk_methylium")["Gamma_t"]
    D, nt = G.shape[0], 7
    P = EC.projector(G)
    assert round(np.trace(P)) < D
    q, p = rng.normal(0.0, 0.5, (D, nt)), rng.normal(0.0, 1.0, (D, nt))
    K = np.stack([EC.symmetric(rng, D, P=P), EC.symmetric(rng, D, 2, P=P)])
    W = np.stack([EC.symmetric(rng, D, 3, P=P), EC.symmetric(rng, D, P=P)])
    c, m, n = rng.standard_normal(2), rng.standard_normal((2, D)) @ P, rng.standard_normal((2, D)) @ P
    fold = _assert_fold_matches(q, p, G, (c, m, K, n, W))
    assert fold[4] == round(np.trace(P)) + 3                    # operator 0: K of full rank in the range, W of rank 3


# ------------------------------------------------------------------------------------------- 3. refusals of the fold

def test_fold_refusals():
    rng = np.random.default_rng(15)
    G = cases.load("hk_methylium")["Gamma_t"]
    D = G.shape[0]
    P = EC.projector(G)
    e, V = np.linalg.eigh(G)
    null = V[:, np.argmin(abs(e))]
    inside = P @ rng.standard_normal(D)
    sym = EC.symmetric(rng, D, P=P)
    with pytest.raises(ValueError, match="at least one"):
        _fold(G)
    for kwargs in (dict(m=inside), dict(m=np.ones((1, D + 1))), dict(K=np.ones((1, D))), dict(c=np.ones((1, 1))),
                   dict(c=np.ones(2), m=inside[None, :]), dict(W=sym), dict(n=np.ones((2, D, D))), dict(c=np.zeros(0))):
        with pytest.raises(ValueError, match="operators"):
            _fold(G, **kwargs)
    for name in "cmKnW":
        bad = {"c": np.ones(1), "m": inside[None, :].copy(), "K": sym[None].copy(), "n": inside[None, :].copy(), "W": sym[None].copy()}[name]
        bad.flat[0] = np.nan
        with pytest.raises(ValueError, match="non-finite"):
            _fold(G, **{name: bad})
    skew = sym.copy()
    skew[0, 1] += 1e-9 * abs(sym).max()
    for name, label in (("K", "xx"), ("W", "pp")):
        with pytest.raises(ValueError, match=f"{label} of operator 1 is not symmetric"):
            _fold(G, **{name: np.stack([sym, skew])})
    tilted = inside + 1e-6 * np.linalg.norm(inside) * null
    for name, label in (("m", "x"), ("n", "p")):
        with pytest.raises(ValueError, match=f"{label} of operator 1 .* range of Gamma_t"):
            _fold(G, **{name: np.stack([inside, tilted])})
    outside = sym + np.outer(null, null)
    for name, label in (("K", "xx"), ("W", "pp")):
        with pytest.raises(ValueError, match=f"{label} of operator 0 .* range of Gamma_t"):
            _fold(G, **{name: outside[None]})
    _fold(G, c=np.ones(1), m=inside[None, :], K=sym[None], n=inside[None, :], W=sym[None])           # and this one is accepted


# ------------------------------------------------------------------------------------------- 4. one Gaussian

def test_one_gaussian_has_its_own_centre_and_widths():
    """n = 1: <x_k> = q_k, <p_k> = p_k, <x_k^2> = q_k^2 + B_kk, <p_k^2> = p_k^2 + hbar^2 Gamma_kk / 2, from the folded columns"""
    rng = np.random.default_rng(16)
    D = 4
    Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    G = (Q * rng.uniform(0.5, 2.0, D)) @ Q.T
    G = 0.5 * (G + G.T)
    B = np.linalg.inv(2.0 * G)
    q, p, v = rng.normal(0.3, 0.8, (D, 1)), rng.normal(0.0, 1.0, (D, 1)), np.array([0.7 - 0.4j])
    eye = np.eye(D)
    sq = np.stack([2.0 * np.outer(e, e) for e in eye])
    zv, zm = np.zeros((D, D)), np.zeros((D, D, D))
    parts = (None, np.concatenate((eye, zv, zv, zv)), np.concatenate((zm, sq, zm, zm)), np.concatenate((zv, zv, eye, zv)),
             np.concatenate((zm, zm, zm, sq)))
    F = EC.folded_factors(q, p, _fold(G, *parts))[:, 0, 0]
    want = np.concatenate((q[:, 0], q[:, 0] ** 2 + np.diag(B), p[:, 0], p[:, 0] ** 2 + 0.5 * HBAR ** 2 * np.diag(G)))
    assert abs(F - want).max() <= 1e-13 * max(1.0, abs(want).max())
    E, _, N2 = EC.restated_expectation(q, p, v, G, *parts)
    assert abs(E / N2 - want).max() <= 1e-13 * max(1.0, abs(want).max())


# ------------------------------------------------------------------------------------------- 5. the interface

def test_tiles_query_and_methods():
    from semiclassical_amd import _lib, propagators as PR
    assert _lib.lib.sc_pair_expect_tiles(1, 1) == 1 and _lib.lib.sc_pair_expect_tiles(130, 65) == 3 * 2
    assert _lib.lib.sc_pair_expect_tiles(0, 5) == 0 and _lib.lib.sc_pair_expect_tiles(5, -1) == 0
    for name in ("expectation", "wavepacket_moments", "energy_expectation"):
        assert callable(getattr(PR.HermanKlukPropagator, name))
    assert PR.WaltonManolopoulosPropagator.expectation is not PR.HermanKlukPropagator.expectation
