"""WaltonManolopoulosPropagator.wm_operator_expectation on the host: the restatement of
tests/wm_energy_cases.py against grid quadrature of the oracle's wavefunction (momentum parts as int conj(p_a psi) (p_b psi) with the
analytic gradient), the folded columns against the restatement pair by pair, the split into calls, the refusals that need no GPU, and
the declaration of the entry."""
import os
import re

import numpy as np
import pytest
import torch

from tests import cases, wm_energy_cases as EC, wm_expect_cases as WC
from tests.test_wm_expect_host import _grid, _oracle_after, _synthetic

torch.set_default_dtype(torch.float64)      # the oracle follows the reference's global default

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUADRATURE = 1e-10      # x int |psi^* A psi|: the bound of section 4.24
FOLD = 1e-12            # x max(1, |F|) per pair


def _quadrature_state(label, ref, points):
    from oracle import norm_oracle
    state = WC.oracle_state(ref)
    # the symmetric part of C alone, as tests/test_wm_expect_host.py:_check_quadrature explains
    state["cqq"] = 0.5 * (state["cqq"] + state["cqq"].transpose(0, 2, 1))
    x, cell = _grid(state, points)
    psi, grad = WC.wavefunction(state, x)
    assert cases.rel_err(psi, norm_oracle.wm_wavefunction(ref, torch.from_numpy(x.T.copy()))) < 1e-12
    return state, x, cell, psi, grad


def _assert_quadrature(label, name, E, integrand, cell):
    quad, scale = cell * integrand.sum(), cell * abs(integrand).sum()
    print(f"{label} <{name}>: restatement {E:.15g}, quadrature {quad:.15g}, difference / int |psi^* A psi| = {abs(E - quad) / scale:.2e}")
    assert abs(E - quad) <= QUADRATURE * scale


def test_restatement_against_quadrature_1d():
    """wm_1d after 3 steps, the first 48 trajectories, 4001 points: <p^2>, <exp(-b x)> with the potential's own b, and <H> of its
    NonHarmonicPotential  V = eps (1 - exp(-b x))^2 / (2 b^2) + (1 - eps) x^2 / 2"""
    g = cases.load("wm_1d")
    state, x, cell, psi, grad = _quadrature_state("wm_1d", _oracle_after(g, 3, 48), 4001)
    eps, b = float(np.ravel(g["eps"])[0]), float(np.ravel(g["b"])[0])
    dens, kin = abs(psi) ** 2, WC.HBAR ** 2 * abs(grad[:, 0]) ** 2
    V = 0.5 * eps / b ** 2 * (1.0 - np.exp(-b * x[:, 0])) ** 2 + 0.5 * (1.0 - eps) * x[:, 0] ** 2
    c, K, W, ex = EC.morse_operator([0.5 * eps / b ** 2], [b], harmonic=[1.0 - eps])
    z = np.zeros((2, 1, 1))
    E, A, N2 = EC.restated_expectation(state, state, c=np.concatenate((np.zeros(2), c)), K=np.concatenate((z, K)),
                                       W=np.concatenate((np.full((1, 1, 1), 2.0), z[:1], W)),
                                       ex=(np.concatenate((np.zeros((1, 2)), np.array([[1.0, 0.0]]), ex[0])),
                                           np.concatenate((np.zeros((1, 2, 1)), np.full((1, 2, 1), b), ex[1]))))
    assert (A >= abs(E)).all()
    for a, (name, f) in enumerate((("p^2", kin), ("exp(-b x)", dens * np.exp(-b * x[:, 0])), ("H", 0.5 * kin + V * dens))):
        _assert_quadrature("wm_1d", name, E[a], f, cell)


def test_restatement_against_quadrature_2d():
    """the D = 2 case of tests/test_wm_expect_host.py (12 trajectories on a Morse surface, 3 steps, 401 x 401 points): a dense 2 x 2
    W and exp(-a.x) with a dense a"""
    from oracle import sc_oracle as orc
    G = torch.tensor([[1.3, 0.4], [0.4, 0.8]])
    ref = orc.WMOracle(G, G, 50.0, 50.0)
    torch.manual_seed(17)
    ref.initial_conditions(torch.tensor([0.6, -0.4]), torch.tensor([0.7, -0.5]), G, ntraj=12)
    pot = orc.MorseOracle(torch.tensor([1.0, 1.4]), torch.tensor([0.02, 0.02]), torch.tensor([0.0, 0.0]))
    for _ in range(3):
        ref.step(pot, 0.05)
    state, x, cell, psi, grad = _quadrature_state("D = 2", ref, 401)
    W = np.array([[1.3, -0.6], [-0.6, 0.7]])
    a = np.array([0.4, -0.3])
    ppsi = -1j * WC.HBAR * grad
    E, _, _ = EC.restated_expectation(state, state, W=np.stack((W, 0.0 * W)), ex=(np.array([[0.0], [1.0]]), np.stack((a, a))[:, None, :]))
    _assert_quadrature("D = 2", "1/2 p^T W p", E[0], 0.5 * np.einsum('xa,ab,xb->x', ppsi.conj(), W, ppsi), cell)
    _assert_quadrature("D = 2", "exp(-a.x)", E[1], abs(psi) ** 2 * np.exp(-x @ a), cell)


# ------------------------------------------------------------------------------------------- the fold against the direct formula

def _folded_elements(bra, ket, c, m, K, n, W, ex):
    from semiclassical_amd import hostmath
    T = torch.from_numpy
    U = ket["U"]
    vx, vp, kind, lam, kap, cols = hostmath.fold_wm_operator_columns(c, m, K, n, W, ex, U)
    assert tuple(kind.shape) == tuple(lam.shape) == (kap.shape[0], cols) and not bool(((kind == 2) & (lam == 0)).any())
    za, zb, g, sfix, sket, ketcol, kd = hostmath.wm_operator_columns(vx, vp, kind, lam, T(bra["Q"]), T(bra["dvec"] @ U), T(ket["Q"]),
                                                                     T(ket["cqq"]), T(ket["dvec"]), T(ket["dvec"] @ U), T(U))
    _, Dp, b = WC.pair_system(bra, ket)
    num = lambda t: None if t is None else t.numpy()
    F, _ = EC.column_elements(Dp, b, num(za), num(zb), num(g), num(sfix), num(sket), num(ketcol), num(kd), lam.numpy(), kap.numpy())
    return F, cols


def _assert_fold(bra, ket, c, m, K, n, W, ex, cols_expected=None):
    _, terms = EC.pair_terms(bra, ket, c, m, K, n, W, ex)
    F = sum(terms)
    got, cols = _folded_elements(bra, ket, c, m, K, n, W, ex)
    assert got.shape == F.shape and (abs(got - F) <= FOLD * np.maximum(1.0, abs(F))).all(), (abs(got - F) / np.maximum(1.0, abs(F))).max()
    if cols_expected is not None:
        assert cols == cols_expected


def _symmetric(rng, U, r):
    """a symmetric matrix of rank r inside the range of U"""
    dp = U.shape[1]
    V = U @ np.linalg.qr(rng.standard_normal((dp, dp)))[0][:, :r]
    return (V * rng.uniform(0.5, 2.0, r) * rng.choice([-1.0, 1.0], r)) @ V.T


def _dense_operators(rng, U, ranks, nexp=2):
    """operators with every part, K of rank 2 and W of the given ranks, ``nexp`` exponentials, everything inside the range of U"""
    D, dp = U.shape
    P = U @ U.T
    M = len(ranks)
    c, m, n = rng.normal(size=M), rng.normal(size=(M, D)) @ P, rng.normal(size=(M, D)) @ P
    K = np.stack([_symmetric(rng, U, min(2, dp)) for _ in ranks])
    W = np.stack([_symmetric(rng, U, r) for r in ranks])
    ex = (rng.normal(size=(M, nexp)), 0.3 * rng.normal(size=(M, nexp, D)) @ P)
    return c, m, K, n, W, ex


def test_fold_dense_ranks_and_missing_parts():
    rng = np.random.default_rng(51)
    x = _synthetic(rng, 7, 6, 6)
    bra, ket = {k: (v[:3] if k != "U" else v) for k, v in x.items()}, x
    c, m, K, n, W, ex = _dense_operators(rng, x["U"], (0, 1, 3, 6))
    ex[0][1, 0] = 0.0                                                            # a term with w = 0 is left out
    _assert_fold(bra, ket, c, m, K, n, W, ex, cols_expected=1 + 2 + 6 + 2)
    _assert_fold(bra, ket, None, m, K, n, W, ex)
    _assert_fold(bra, ket, c, None, K, n, W, ex)
    _assert_fold(bra, ket, c, m, None, n, W, ex, cols_expected=1 + 6 + 2)
    _assert_fold(bra, ket, c, m, K, None, W, ex)
    _assert_fold(bra, ket, c, m, K, n, None, ex, cols_expected=1 + 2 + 2)
    _assert_fold(bra, ket, c, m, K, n, W, None, cols_expected=1 + 2 + 6)
    _assert_fold(bra, ket, None, None, None, None, W, None, cols_expected=1 + 6)
    _assert_fold(bra, ket, None, None, None, None, None, ex, cols_expected=1 + 2)
    _assert_fold(bra, ket, c[:1], None, None, None, None, None, cols_expected=1)


def test_fold_singular_width_of_methylium():
    """D = 12, d' = 6: the oracle's state after 2 steps, W and a projected onto the non-zero width modes; refused unprojected"""
    from semiclassical_amd import hostmath
    ref = _oracle_after(cases.load("wm_methylium"), 2, 6)
    state = WC.oracle_state(ref)
    U = state["U"]
    assert U.shape == (12, 6)
    c, m, K, n, W, ex = _dense_operators(np.random.default_rng(53), U, (0, 2, 6))
    _assert_fold(state, state, c, m, K, n, W, ex, cols_expected=1 + 2 + 6 + 2)
    fold = lambda W, ex: hostmath.fold_wm_operator_columns(c, m, K, n, W, ex, U)
    raw = W.copy()
    raw[1] = np.eye(12)
    with pytest.raises(ValueError, match="pp of operator 1 .* outside the range"):
        fold(raw, ex)
    null = np.linalg.svd(U.T)[2][-1]
    a = ex[1].copy()
    a[2, 1] += 1e-6 * null
    with pytest.raises(ValueError, match="a of ex of operator 2 .* outside the range"):
        fold(W, (ex[0], a))
    w0 = ex[0].copy()
    w0[2, 1] = 0.0
    fold(W, (w0, a))                                                             # ... but not where w = 0


# ------------------------------------------------------------------------------------------- the split into calls

def test_launch_plan_covers_every_column_once():
    from semiclassical_amd import hostmath
    lam, kind = torch.zeros((3, 8)), torch.zeros((3, 8), dtype=torch.int32)
    lam[:, 0] = 1.0
    lam[0, 1:8], kind[0, 1:8] = torch.arange(1.0, 8.0), torch.tensor([1, 1, 1, 2, 2, 2, 2], dtype=torch.int32)
    lam[1, 1:3], kind[1, 1:3] = 1.0, torch.tensor([1, 2], dtype=torch.int32)
    lam[2, 1], kind[2, 1] = -2.0, 2
    cols, calls = hostmath.wm_operator_launches(lam, kind, 4)
    assert cols == 4 and len(calls) == 5                    # three pieces of operator 0, one of each other: one piece per call
    for cap in (2, 3, 4, 5, 8, 9, 16, 24):
        cols, calls = hostmath.wm_operator_launches(lam, kind, cap)
        assert cols == min(8, cap)
        if cap == 9:
            assert len(calls) == 3
        kind_p, lam_p = torch.cat((kind.reshape(-1), torch.zeros(1, dtype=torch.int32))), torch.cat((lam.reshape(-1), torch.zeros(1)))
        seen = []
        for ops, owners, columns in calls:
            assert 1 <= len(ops) == len(owners) and len(columns) == len(ops) * cols <= cap
            for e, (op, a) in enumerate(zip(ops, owners)):
                mine = columns[e * cols:(e + 1) * cols]
                assert op in (a, 3) and mine[0] == (8 * a if op == a else 24)
                assert all(col == 24 or col // 8 == a for col in mine)
                seen += [col for col in mine if col != 24]
            idx = torch.tensor(columns)
            assert not bool(((kind_p[idx] == 2) & (lam_p[idx] == 0)).any())       # no padding with kind 2
        assert len(seen) == len(set(seen))
        needed = {8 * a + r for a in range(3) for r in range(8) if r == 0 or lam[a, r] != 0}
        assert needed <= set(seen)
    lam[2, 1] = 0.0
    with pytest.raises(ValueError, match="kind-2 column with lam = 0"):
        hostmath.wm_operator_launches(lam, kind, 4)


# ------------------------------------------------------------------------------------------- refusals, declaration

def test_refusals():
    from semiclassical_amd import hostmath
    rng = np.random.default_rng(57)
    U, _ = np.linalg.qr(rng.standard_normal((5, 3)))
    null = np.linalg.svd(U.T)[2][-1]
    inside = U @ rng.standard_normal(3)
    fold = lambda **kw: hostmath.fold_wm_operator_columns(kw.get("c"), kw.get("x"), kw.get("xx"), kw.get("p"), kw.get("pp"), kw.get("ex"), U)
    out = fold(x=inside[None], p=inside[None], xx=np.outer(inside, inside)[None], pp=np.outer(inside, inside)[None],
               ex=(np.ones((1, 1)), inside[None, None]))
    assert out[5] == 4 and out[2].tolist() == [[0, 1, 1, 2]]
    with pytest.raises(ValueError, match="x of operator 1 .* outside the range"):
        fold(x=np.stack([inside, inside + 1e-6 * null]))
    with pytest.raises(ValueError, match="pp of operator 0 .* outside the range"):
        fold(pp=np.eye(5)[None])
    with pytest.raises(ValueError, match="a of ex of operator 0 .* outside the range"):
        fold(ex=(np.ones((1, 2)), np.stack([inside, null])[None]))
    with pytest.raises(ValueError, match="at least one"):
        fold()
    skew = np.outer(inside, inside)
    skew[0, 1] += 1e-6
    with pytest.raises(ValueError, match="pp of operator 0 is not symmetric"):
        fold(pp=skew[None])
    for kw in (dict(pp=np.ones((1, 5))), dict(c=np.ones(2), pp=np.outer(inside, inside)[None]), dict(pp=np.full((1, 5, 5), np.nan)),
               dict(ex=np.ones((1, 1))), dict(ex=(np.ones((1, 2)), np.ones((1, 1, 5)))), dict(ex=(np.ones(1), np.ones((1, 5)))),
               dict(ex=(np.array([[np.inf]]), inside[None, None])), dict(c=np.ones(2), ex=(np.ones((1, 1)), inside[None, None]))):
        with pytest.raises(ValueError, match="operators"):
            fold(**kw)


def test_header_declares_and_lib_binds_the_entry():
    from semiclassical_amd import _lib
    header = open(os.path.join(ROOT, "include", "semiclassical_hip.h")).read()
    assert re.search(r"\bsc_wm_pair_expect_cols\(", header) and "sc_wm_pair_expect_cols" in _lib.SIGNATURES
    decl = re.search(r"int sc_wm_pair_expect_cols\((.*?)\);", header, re.S).group(1)
    old = re.search(r"int sc_wm_pair_expect\((.*?)\);", header, re.S).group(1)
    assert len(decl.split(",")) == len(_lib.SIGNATURES["sc_wm_pair_expect_cols"][1]) == len(old.split(",")) + 3
    assert len(old.split(",")) == len(_lib.SIGNATURES["sc_wm_pair_expect"][1])              # the old entry keeps its signature
    assert _lib.lib.sc_wm_pair_expect_capacity(24, 24) == 76                                # 1 + 24 + 48 = 73 columns fit in one call


def test_c_abi_refusals_before_any_device_work():
    """null arguments, counts and limits are refused before the entry touches the device"""
    from semiclassical_amd._lib import lib
    p = 4096        # never dereferenced

    def args(M=1, cols=1, S=0, D=3, dp=2, first=p, sket=None, ketcol=p, kind=p, last=p):
        return (first, p, p, p, 2, p, p, p, p, p, p, 2, p, D, dp, p, p, p, p, sket, S, ketcol, kind, p, p, M, cols, p, last, None)
    for bad in (dict(first=None), dict(ketcol=None), dict(kind=None), dict(last=None), dict(S=1), dict(M=0), dict(cols=0), dict(S=-1, sket=p)):
        assert lib.sc_wm_pair_expect_cols(*args(**bad)) == -1                       # SC_ERR_BAD_ARGUMENT
    assert lib.sc_wm_pair_expect_cols(*args(S=1)) == -1 and b"null argument" in lib.sc_last_error()
    for D, dp in ((513, 8), (120, 97), (4, 5)):
        assert lib.sc_wm_pair_expect_cols(*args(D=D, dp=dp)) == -2                  # SC_ERR_UNSUPPORTED
        assert b"D <= 512, d' <= 96" in lib.sc_last_error()
    assert lib.sc_wm_pair_expect_cols(*args(M=65536)) == -2 and b"M <= 65535" in lib.sc_last_error()
    assert lib.sc_wm_pair_expect_cols(*args(M=33, cols=3)) == -2 and b"at most 98" in lib.sc_last_error()
    assert lib.sc_wm_pair_expect_cols(*args(D=96, dp=96, M=1, cols=5)) == -2 and b"at most 4" in lib.sc_last_error()
