"""WaltonManolopoulosPropagator.wm_expectation on the host: the restatement of tests/wm_expect_cases.py against
grid quadrature of the oracle's wavefunction, the folded columns against the restatement pair by pair, the split into calls, the
refusals, and the declaration of the entry."""
import os
import re

import numpy as np
import pytest
import torch

from tests import cases, wm_expect_cases as WC

torch.set_default_dtype(torch.float64)      # the oracle follows the reference's global default

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUADRATURE = 1e-10      # x int |psi^* A psi|: the bound of section 4.21
FOLD = 1e-12            # x max(1, |F|) per pair


def _oracle_after(g, steps, ntraj):
    g = dict(g)
    g["zi"], g["probi"] = g["zi"][:, :ntraj], g["probi"][:ntraj]
    ref, pot = cases.oracle_propagator(g), cases.oracle_potential(g)
    for _ in range(steps):
        ref.step(pot, float(g["dt"]))
    return ref


def _grid(state, points, reach=9.0):
    """a uniform grid per axis that covers every Gaussian to `reach` standard deviations of its narrowest real width"""
    D = state["Q"].shape[1]
    width = min(np.linalg.eigvalsh(C.real).min() for C in state["cqq"])
    assert width > 0
    axes = [np.linspace(state["Q"][:, a].min() - reach / np.sqrt(width), state["Q"][:, a].max() + reach / np.sqrt(width), points)
            for a in range(D)]
    x = np.stack([m.reshape(-1) for m in np.meshgrid(*axes, indexing="ij")], axis=1)
    return x, np.prod([ax[1] - ax[0] for ax in axes])


def _check_quadrature(label, ref, points):
    from oracle import norm_oracle
    state = WC.oracle_state(ref)
    # x^T C x sees the symmetric part of C alone; the formula is one for complex symmetric C, and the oracle's C_QQ is symmetric to
    # rounding of its inverses only (8.6e-10 in the D = 2 case, which moves N2 by 4e-12 of int |psi|^2)
    print(f"{label}: |C - C^T| <= {max(abs(C - C.T).max() for C in state['cqq']):.1e}")
    state["cqq"] = 0.5 * (state["cqq"] + state["cqq"].transpose(0, 2, 1))
    x, cell = _grid(state, points)
    psi, grad = WC.wavefunction(state, x)
    want = norm_oracle.wm_wavefunction(ref, torch.from_numpy(x.T.copy()))
    assert cases.rel_err(psi, want) < 1e-12                   # the restated Gaussians are the oracle's wavefunction
    D = x.shape[1]
    u = WC.random_direction(np.random.default_rng(3), state["U"])
    ux = x @ u
    integrands = {"1": psi.conj() * psi, "x": psi.conj() * ux * psi, "x^2": psi.conj() * ux ** 2 * psi,
                  "p": psi.conj() * (-1j * WC.HBAR) * (grad @ u)}
    c, m, K, n = np.zeros(4), np.zeros((4, D)), np.zeros((4, D, D)), np.zeros((4, D))
    c[0], m[1], K[2], n[3] = 1.0, u, 2.0 * np.outer(u, u), u
    E, _, N2 = WC.restated_expectation(state, state, c, m, K, n)
    assert abs(E[0] - N2) <= 1e-14 * abs(N2)
    for a, (name, f) in enumerate(integrands.items()):
        quad, scale = cell * f.sum(), cell * abs(f).sum()
        print(f"{label} <{name}>: restatement {E[a]:.15g}, quadrature {quad:.15g}, difference / int |psi^* A psi| = {abs(E[a] - quad) / scale:.2e}")
        assert abs(E[a] - quad) <= QUADRATURE * scale


def test_restatement_against_quadrature_1d():
    """wm_1d after 3 steps, the first 48 trajectories, 4001 points"""
    _check_quadrature("wm_1d", _oracle_after(cases.load("wm_1d"), 3, 48), 4001)


def test_restatement_against_quadrature_2d():
    """D = 2 with a non-diagonal width matrix and non-zero momenta: 12 trajectories on a Morse surface, 3 steps, 401 x 401 points"""
    from oracle import sc_oracle as orc
    G = torch.tensor([[1.3, 0.4], [0.4, 0.8]])
    ref = orc.WMOracle(G, G, 50.0, 50.0)
    torch.manual_seed(17)
    ref.initial_conditions(torch.tensor([0.6, -0.4]), torch.tensor([0.7, -0.5]), G, ntraj=12)
    pot = orc.MorseOracle(torch.tensor([1.0, 1.4]), torch.tensor([0.02, 0.02]), torch.tensor([0.0, 0.0]))
    for _ in range(3):
        ref.step(pot, 0.05)
    state = WC.oracle_state(ref)
    assert abs(state["cqq"][0][0, 1]) > 0.05
    _check_quadrature("D = 2", ref, 401)


# ------------------------------------------------------------------------------------------- the fold against the direct formula

def _synthetic(rng, n, D, dp, width=1.0, spread=0.3):
    """a state of random complex symmetric widths with a positive definite real part (the recipe of tests/test_wm_norm_large_gpu.py)"""
    U, _ = np.linalg.qr(rng.standard_normal((D, dp)))
    cqq = np.empty((n, D, D), dtype=complex)
    for t in range(n):
        A = rng.standard_normal((D, D)) / np.sqrt(D)
        B = rng.standard_normal((D, D)) / np.sqrt(D)
        cqq[t] = width * (np.eye(D) + 0.2 * (A @ A.T) + 0.3j * (B + B.T))
    return dict(Q=rng.normal(0.0, spread, (n, D)), coef=rng.normal(size=n) + 1j * rng.normal(size=n), cqq=cqq,
                dvec=0.1 * width * (rng.normal(size=(n, D)) + 1j * rng.normal(size=(n, D))), U=U)


def _folded_elements(bra, ket, c, m, K, n):
    from semiclassical_amd import hostmath
    T = torch.from_numpy
    U = ket["U"]
    vx, nvec, lam, kap, R = hostmath.fold_wm_expectation_operators(c, m, K, n, U)
    za, zb, g, sfix, sket = hostmath.wm_expectation_columns(vx, nvec, T(bra["Q"]), T(bra["dvec"] @ U), T(ket["Q"]), T(ket["cqq"]),
                                                            T(ket["dvec"]), T(ket["dvec"] @ U), T(U))
    _, Dp, b = WC.pair_system(bra, ket)
    num = lambda t: None if t is None else t.numpy()
    return WC.column_elements(Dp, b, num(za), num(zb), num(g), num(sfix), num(sket), lam.numpy(), kap.numpy()), R


def _assert_fold(bra, ket, c, m, K, n, R_expected=None):
    _, F = WC.pair_elements(bra, ket, c, m, K, n)
    got, R = _folded_elements(bra, ket, c, m, K, n)
    assert got.shape == F.shape and (abs(got - F) <= FOLD * np.maximum(1.0, abs(F))).all(), abs(got - F).max()
    if R_expected is not None:
        assert R == R_expected


def _dense_operators(rng, U, ranks):
    """operators with every part, K of the given ranks, everything inside the range of U"""
    D, dp = U.shape
    P = U @ U.T
    M = len(ranks)
    c, m, n = rng.normal(size=M), rng.normal(size=(M, D)) @ P, rng.normal(size=(M, D)) @ P
    K = np.zeros((M, D, D))
    for a, r in enumerate(ranks):
        V = U @ np.linalg.qr(rng.standard_normal((dp, dp)))[0][:, :r]
        K[a] = (V * rng.uniform(0.5, 2.0, r) * rng.choice([-1.0, 1.0], r)) @ V.T
    return c, m, K, n


def test_fold_dense_ranks_and_missing_parts():
    rng = np.random.default_rng(41)
    x = _synthetic(rng, 7, 6, 6)
    bra, ket = {k: (v[:3] if k != "U" else v) for k, v in x.items()}, x
    c, m, K, n = _dense_operators(rng, x["U"], (0, 1, 3, 6))
    _assert_fold(bra, ket, c, m, K, n, R_expected=6)
    _assert_fold(bra, ket, None, m, K, n)
    _assert_fold(bra, ket, c, None, K, n)
    _assert_fold(bra, ket, c, m, None, n, R_expected=0)
    _assert_fold(bra, ket, c, m, K, None)
    _assert_fold(bra, ket, c[:1], None, None, None, R_expected=0)


def test_fold_singular_width_of_methylium():
    """D = 12, d' = 6: the oracle's state after 2 steps, every operator projected onto the non-zero width modes"""
    ref = _oracle_after(cases.load("wm_methylium"), 2, 6)
    state = WC.oracle_state(ref)
    assert state["U"].shape == (12, 6)
    c, m, K, n = _dense_operators(np.random.default_rng(43), state["U"], (0, 2, 6))
    _assert_fold(state, state, c, m, K, n, R_expected=6)


def test_refusals():
    from semiclassical_amd import hostmath
    rng = np.random.default_rng(47)
    U, _ = np.linalg.qr(rng.standard_normal((5, 3)))
    null = np.linalg.svd(U.T)[2][-1]
    inside = U @ rng.standard_normal(3)
    fold = lambda **kw: hostmath.fold_wm_expectation_operators(kw.get("c"), kw.get("x"), kw.get("xx"), kw.get("p"), U)
    fold(x=inside[None], p=inside[None], xx=np.outer(inside, inside)[None])
    with pytest.raises(ValueError, match="x of operator 1 .* outside the range"):
        fold(x=np.stack([inside, inside + 1e-6 * null]))
    with pytest.raises(ValueError, match="p of operator 0 .* outside the range"):
        fold(p=null[None])
    with pytest.raises(ValueError, match="xx of operator 0 .* outside the range"):
        fold(xx=np.eye(5)[None])
    with pytest.raises(ValueError, match="at least one"):
        fold()
    skew = np.outer(inside, inside)
    skew[0, 1] += 1e-6
    with pytest.raises(ValueError, match="xx of operator 0 is not symmetric"):
        fold(xx=skew[None])
    for kw in (dict(x=np.ones(5)), dict(c=np.ones(2), x=inside[None]), dict(c=np.array([np.nan])), dict(xx=np.ones((1, 5)))):
        with pytest.raises(ValueError, match="operators"):
            fold(**kw)


def test_launch_plan_covers_every_column_once():
    from semiclassical_amd import hostmath
    lam = torch.zeros((3, 8))
    lam[:, 0] = 1.0
    lam[0, 1:8] = torch.arange(1.0, 8.0)
    lam[1, 1:3] = 1.0
    for cap in (2, 3, 4, 5, 8, 16, 24):
        Rl, calls = hostmath.wm_expectation_launches(lam, cap)
        assert Rl == min(7, cap - 1)
        seen = []
        for pieces in calls:
            assert 1 <= len(pieces) and len(pieces) * (1 + Rl) <= cap
            for a, first, sq in pieces:
                assert len(sq) <= Rl
                seen += [(a, 0)] * first + [(a, r) for r in sq]
        assert len(seen) == len(set(seen))
        needed = {(a, r) for a in range(3) for r in range(8) if r == 0 or lam[a, r] != 0}
        assert needed <= set(seen)


def test_header_declares_and_lib_binds_the_entry():
    from semiclassical_amd import _lib
    header = open(os.path.join(ROOT, "include", "semiclassical_hip.h")).read()
    for name in ("sc_wm_pair_expect", "sc_wm_pair_expect_tiles", "sc_wm_pair_expect_capacity"):
        assert re.search(r"\b%s\(" % name, header) and name in _lib.SIGNATURES
    decl = re.search(r"int sc_wm_pair_expect\((.*?)\);", header, re.S).group(1)
    assert len(decl.split(",")) == len(_lib.SIGNATURES["sc_wm_pair_expect"][1])
    assert _lib.lib.sc_wm_pair_expect_tiles(1, 1) == 1 and _lib.lib.sc_wm_pair_expect_tiles(19, 35) == 2 * 3
    assert _lib.lib.sc_wm_pair_expect_tiles(0, 5) == 0
    cap = _lib.lib.sc_wm_pair_expect_capacity
    assert cap(96, 96) == 4 and cap(512, 96) == 4 and cap(24, 24) == 76 and cap(1, 1) == 99
    assert cap(513, 8) == 0 and cap(120, 97) == 0 and cap(4, 5) == 0 and cap(0, 0) == 0
    assert all(cap(D, dp) >= 4 for D, dp in ((3, 3), (64, 64), (512, 1), (512, 96)))
