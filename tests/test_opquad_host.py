"""Operator correlation functions <phi_0| A e^(-iHt) B |phi_0> with QUADRATIC operators c + m.x + 1/2 x^T K x (DESIGN.md section
4.16), host side (no GPU): a numpy restatement of the Gaussian matrix element -- the reference of tests/test_opquad_gpu.py --
against quadrature, the columns the kernel takes against the direct formula, the refusals, the closed form at t = 0 within the
Monte-Carlo error, the result file's pooling and the C-ABI symbols."""
import os
import re
import types

import numpy as np
import pytest

from tests import cases
from tests.test_cross_host import _random_spd, coherent_overlap, gaussian
from tests.test_opcorr_host import (ZERO, _batch, _store, initial_terms, pinv_sum, position_element, project, restated_rows,
                                    within_five_sigma)


# ------------------------------------------------------------------------------------------- the restatement

def quadratic_element(c, m, K, qa, pa, Ga, qb, pb, Gb):
    """<a|c + m.x + 1/2 x^T K x|b> / <a|b> = c + m.xbar + 1/2 xbar^T K xbar + 1/2 tr(K S), S = (Ga + Gb)^+, xbar the complex mean of
    tests/test_opcorr_host.py::position_element: (n, M) for centres (D,) or (D, n).  No eigendecomposition of K."""
    x = position_element(qa, pa, Ga, qb, pb, Gb)                      # (D, n)
    S = pinv_sum(Ga, Gb)[0]
    return (c[None, :] + (m @ x).T + 0.5 * np.einsum('dn,ade,en->na', x, K, x) + 0.5 * np.einsum('ade,ed->a', K, S)[None, :])


def ket_factors(c, m, K, q, p, Gi, G0, q0, p0):
    """g_ia, (n, M), from the initial points q, p (D, n): the trajectory's Gaussian is the bra"""
    return quadratic_element(c, m, K, q, p, Gi, q0, p0, G0)


def bra_factors(c, m, K, Q, P, Gt, G0, q0, p0):
    """f_ia, (n, M), from the current points Q, P (D, n): phi_0 is the bra"""
    return quadratic_element(c, m, K, q0, p0, G0, Q, P, Gt)


def restated_opquad(bra, ket, Q, P, q, p, cq, Gi, Gt, G0, q0, p0, kept=None):
    """rows (M, 5) of x_ia = f_ia g_ia cq_i (no dynamical phase); bra, ket = (c, m, K)"""
    f = bra_factors(*bra, Q, P, Gt, G0, q0, p0)
    g = ket_factors(*ket, q, p, Gi, G0, q0, p0)
    return restated_rows(f * g * cq[:, None], kept)


def closed_form_t0(bra, ket, G0, q0):
    """X_a(0) = <phi_0|A_a B_a|phi_0> with Sigma = 1/2 G0^+, alpha = c + m.q0 + 1/2 q0^T K q0, a = m + K q0:
    (alpha_A + 1/2 tr K_A Sigma)(alpha_B + 1/2 tr K_B Sigma) + a_A^T Sigma a_B + 1/2 tr(K_A Sigma K_B Sigma)"""
    e, V = np.linalg.eigh(G0)
    keep = abs(e) > ZERO
    Sigma = 0.5 * (V[:, keep] / e[keep]) @ V[:, keep].T
    out = []
    for (cA, mA, KA), (cB, mB, KB) in zip(zip(*bra), zip(*ket)):
        alpha = [c + m @ q0 + 0.5 * q0 @ K @ q0 + 0.5 * np.trace(K @ Sigma) for c, m, K in ((cA, mA, KA), (cB, mB, KB))]
        out.append(alpha[0] * alpha[1] + (mA + KA @ q0) @ Sigma @ (mB + KB @ q0) + 0.5 * np.trace(KA @ Sigma @ KB @ Sigma))
    return np.array(out)


def random_symmetric(rng, D, rank, Ga=None, Gb=None):
    """a random symmetric (D, D) matrix of the given rank with eigenvalues of both signs (rank >= 2), its eigenvectors inside the
    range of Ga + Gb when given"""
    if rank == 0:
        return np.zeros((D, D))
    vectors = rng.normal(size=(rank, D))
    if Ga is not None:
        vectors = project(vectors, Ga, Gb)
    signs = np.where(np.arange(rank) % 2 == 0, 1.0, -1.0)
    return np.einsum('r,rd,re->de', signs * rng.uniform(0.5, 1.5, rank), vectors, vectors)


def t0_operator_pairs(D):
    """the three pairs of the 5 sigma checks (this file and test_opquad_gpu.py): (x_0^2, 1), (x_0 x_4, x_0 x_4), and a mixed pair
    with c, m and K all non-zero and K of full rank"""
    e = np.eye(D)
    K = np.zeros((2, 3, D, D))
    K[0, 0] = 2.0 * np.outer(e[0], e[0])
    K[0, 1] = K[1, 1] = np.outer(e[0], e[4]) + np.outer(e[4], e[0])
    rng = np.random.default_rng(16)
    K[0, 2] = 0.01 * random_symmetric(rng, D, D) + 0.02 * np.eye(D)
    K[1, 2] = 0.01 * random_symmetric(rng, D, D) - 0.015 * np.eye(D)
    assert all(np.linalg.matrix_rank(K[s, 2]) == D for s in (0, 1))
    mixed_a, mixed_b = 0.5 * e[1] - 0.25 * e[3] + 0.1 * e[0], 0.3 * e[2] + 0.2 * e[1] - 0.15 * e[4]
    bra = (np.array([0.0, 0.0, 0.7]), np.array([np.zeros(D), np.zeros(D), mixed_a]), K[0])
    ket = (np.array([1.0, 0.0, -1.3]), np.array([np.zeros(D), np.zeros(D), mixed_b]), K[1])
    return bra, ket


def _t(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.float64))


def folded(c, m, K, G, G0, q0, p0, ket):
    """(u, w, kappa, lam, R) of hostmath.fold_quadratic_operators as numpy"""
    from semiclassical_amd import hostmath
    *cols, R = hostmath.fold_quadratic_operators(_t(c), _t(m), None if K is None else _t(K), _t(G), _t(G0), _t(q0), _t(p0), ket=ket)
    return tuple(a.numpy() for a in cols) + (R,)


def columns_value(cols, q, p):
    """sum_col lam z^p, z = kappa + u.q + i w.p, (n, M): what the kernels compute from the columns; q, p (D, n)"""
    u, w, kap, lam, R = cols
    z = kap[None] + np.einsum('acd,dn->nac', u, q) + 1j * np.einsum('acd,dn->nac', w, p)
    return (lam[None, :, :1] * z[:, :, :1]).sum(2) + (lam[None, :, 1:] * z[:, :, 1:] ** 2).sum(2)


# ------------------------------------------------------------------------------------------- 1. matrix element vs quadrature

@pytest.mark.parametrize("D", [1, 2])
def test_matrix_element_matches_quadrature(D):
    """int phi_a^*(x) (c + m.x + 1/2 x^T K x) phi_b(x) dx / <a|b> by the trapezoid rule (the grid of tests/test_opcorr_host.py)
    against the matrix-element formula; D = 2: non-diagonal Gamma_a != Gamma_b, non-zero momenta, an indefinite K"""
    rng = np.random.default_rng(40 + D)
    Ga, Gb = _random_spd(rng, D), _random_spd(rng, D)
    qa, qb = rng.normal(0.0, 0.8, D), rng.normal(0.0, 0.8, D)
    pa, pb = rng.normal(0.0, 1.2, D), rng.normal(0.0, 1.2, D)
    c, m = rng.normal(size=3), rng.normal(size=(3, D))
    K = np.array([random_symmetric(rng, D, D) for _ in range(3)])
    if D == 2:
        assert np.linalg.eigvalsh(K[0]).min() < 0 < np.linalg.eigvalsh(K[0]).max() and abs(Ga[0, 1]) > 0
    axis = np.arange(-14.0, 14.0 + 1e-9, 0.04)
    x = np.stack([a.ravel() for a in np.meshgrid(*([axis] * D), indexing="ij")])
    weight = np.conj(gaussian(qa, pa, Ga, x)) * gaussian(qb, pb, Gb, x) * 0.04 ** D
    overlap = coherent_overlap(qa, pa, Ga, qb, pb, Gb)
    assert abs(weight.sum() - overlap) <= 1e-12 * abs(overlap)
    quad = (c[:, None] + m @ x + 0.5 * np.einsum('dn,ade,en->an', x, K, x)) @ weight / overlap
    closed = quadratic_element(c, m, K, qa, pa, Ga, qb, pb, Gb)[0]
    dev = abs(closed - quad) / abs(closed)
    print(f"D = {D}: |<a|A|b> / <a|b>| {np.array2string(abs(closed), precision=3)}, deviation from quadrature {dev.max():.2e}")
    assert (dev <= 1e-10).all()


# ------------------------------------------------------------------------------------------- 2. the columns

def _fold_deviation(Gi, Gt, G0, q0, p0, q, p, c, m, K_of):
    """largest deviation of the columns' value from the direct formula over both sides, relative to max(1, |f|); K_of(G): the K of
    a side with the widths G"""
    worst = 0.0
    for ket, G in ((False, Gt), (True, Gi)):
        K = K_of(G)
        cols = folded(c, m, K, G, G0, q0, p0, ket)
        M, D = m.shape
        R = cols[4]
        assert cols[0].shape == cols[1].shape == (M, 1 + R, D) and cols[2].shape == cols[3].shape == (M, 1 + R)
        assert cols[2].dtype == np.complex128 and (cols[3][:, 0] == 1.0).all()
        direct = ket_factors(c, m, K, q, p, G, G0, q0, p0) if ket else bra_factors(c, m, K, q, p, G, G0, q0, p0)
        worst = max(worst, (abs(columns_value(cols, q, p) - direct) / np.maximum(1.0, abs(direct))).max())
    return worst


def test_fold_dense_ranks_and_padding():
    """dense D = 6, K of ranks 0, 1, 3 and 6 within one set: R = 6, the operators of lower rank padded with columns of zeros"""
    rng = np.random.default_rng(26)
    D, n, ranks = 6, 9, (0, 1, 3, 6)
    Gi, Gt, G0 = _random_spd(rng, D), _random_spd(rng, D), _random_spd(rng, D)
    K = np.array([random_symmetric(rng, D, r) for r in ranks])
    q0, p0 = rng.normal(0.0, 0.8, D), rng.normal(0.0, 1.2, D)
    c, m = rng.normal(size=4), rng.normal(size=(4, D))
    dev = _fold_deviation(Gi, Gt, G0, q0, p0, rng.normal(0.0, 0.8, (D, n)), rng.normal(0.0, 1.2, (D, n)), c, m, lambda G: K)
    print(f"dense D = {D}, ranks {ranks}: columns against the direct formula {dev:.2e}")
    assert dev <= 1e-12
    u, w, kap, lam, R = folded(c, m, K, Gt, G0, q0, p0, False)
    assert R == 6
    for a, r in enumerate(ranks):
        assert np.count_nonzero(lam[a, 1:]) == r
        assert not u[a, 1 + r:].any() and not w[a, 1 + r:].any() and not kap[a, 1 + r:].any() and not lam[a, 1 + r:].any()


def test_fold_singular_widths():
    """methylium's Cartesian widths are singular (rank 6 of 12): K projected onto the range of its side"""
    g = cases.load("hk_methylium")
    Gi, Gt, G0 = g["Gamma_i"], g["Gamma_t"], g["Gamma_0"]
    D = Gt.shape[0]
    assert np.count_nonzero(abs(np.linalg.eigvalsh(Gt + G0)) > ZERO) < D
    rng = np.random.default_rng(27)
    m = project(rng.normal(size=(3, D)), Gt, G0)
    seeds = rng.integers(1 << 30, size=3)
    K_of = lambda G: np.array([random_symmetric(np.random.default_rng(s), D, r, G, G0) for s, r in zip(seeds, (2, 6, 1))])
    dev = _fold_deviation(Gi, Gt, G0, g["q0"], g["p0"], g["zi"][:D, :16], g["zi"][D:, :16], rng.normal(size=3), m, K_of)
    print(f"methylium: columns against the direct formula {dev:.2e}")
    assert dev <= 1e-12


# ------------------------------------------------------------------------------------------- 3. refusals

def test_refusals():
    from semiclassical_amd.propagators import HermanKlukPropagator as HK
    g = cases.load("hk_methylium")
    Gt, G0 = g["Gamma_t"], g["Gamma_0"]
    D = Gt.shape[0]
    rng = np.random.default_rng(31)
    c, m = np.zeros(2), project(rng.normal(size=(2, D)), Gt, G0)
    good = np.array([random_symmetric(rng, D, 2, Gt, G0) for _ in range(2)])
    args = (Gt, G0, g["q0"], g["p0"])
    assert folded(c, m, good, *args, False)[4] == 2
    skew = good.copy()
    skew[1, 0, 1] += 1e-9 * abs(good[1]).max()
    with pytest.raises(ValueError, match="symmetric"):
        folded(c, m, skew, *args, False)
    for bad in (np.nan, np.inf):
        broken = good.copy()
        broken[0, 2, 2] = bad
        with pytest.raises(ValueError, match="finite"):
            folded(c, m, broken, *args, True)
    e, V = np.linalg.eigh(Gt + G0)
    null = V[:, abs(e) <= ZERO][:, 0]
    outside = good.copy()
    outside[1] += 1e-6 * abs(good[1]).max() * np.outer(null, null)
    for ket in (False, True):
        with pytest.raises(ValueError, match="operator 1"):
            folded(c, m, outside, *args, ket)
    with pytest.raises(ValueError):
        folded(c, m, good[:, 0], *args, False)                        # K of shape (M, D)
    with pytest.raises(ValueError):
        folded(c, m, np.concatenate((good, good[:1])), *args, False)  # (M + 1, D, D)
    # the propagator's own validation of one side, without a device
    stub = types.SimpleNamespace(dim=D, _is_operator_set=HK._is_operator_set, _operator_set=lambda n, o: HK._operator_set(stub, n, o),
                                 _operator_hessians=HK._operator_hessians)
    side = lambda ops: HK._operator_side(stub, "bra", ops)
    assert side((c, m, good))[2].shape == (2, D, D)
    broken = good.copy()
    broken[0, 2, 2] = np.nan
    for ops in ((c, m, skew), (c, m, broken), (c, m, good[:, 0]), (c, m, np.concatenate((good, good[:1]))), (c, m, good[:1]),
                (c, m, good, good)):
        with pytest.raises(ValueError):
            side(ops)
    # a ket with another M: refused by the preparation of the pair before anything touches the device
    prop = types.SimpleNamespace(_opcorr_ok=True, _operator_side=lambda name, ops: HK._operator_side(stub, name, ops))
    with pytest.raises(ValueError, match="same number"):
        HK._operator_pair(prop, "_opcorr", (c, m, good), (np.zeros(3), np.zeros((3, D)), None), None, None, None, None)


# ------------------------------------------------------------------------------------------- 4. equivalent inputs

def test_no_k_and_zero_k_are_the_linear_operators():
    """(c, m), (c, m, None) and (c, m, zeros) validate to the same side (K = None), the same cache key and the linear path; their
    single column is fold_linear_operators' affine form bit for bit"""
    import torch
    from semiclassical_amd import hostmath
    from semiclassical_amd.propagators import HermanKlukPropagator as HK
    rng = np.random.default_rng(41)
    D, M = 5, 3
    c, m = rng.normal(size=M), rng.normal(size=(M, D))
    stub = types.SimpleNamespace(dim=D, _is_operator_set=HK._is_operator_set, _operator_set=lambda n, o: HK._operator_set(stub, n, o),
                                 _operator_hessians=HK._operator_hessians)
    sides = [HK._operator_side(stub, "bra", ops) for ops in ((c, m), (c, m, None), (c, m, np.zeros((M, D, D))))]
    assert all(s[2] is None for s in sides)
    keys = {HK._operators_key(s, s) for s in sides}
    assert len(keys) == 1
    other = HK._operator_side(stub, "bra", (c, m, np.array([random_symmetric(rng, D, 2)] * M)))
    assert other[2] is not None and HK._operators_key(other, other) not in keys
    assert HK._operators_key(sides[0], other) not in keys and HK._operators_key(other, sides[0]) != HK._operators_key(sides[0], other)
    G, G0 = _random_spd(rng, D), _random_spd(rng, D)
    q0, p0 = rng.normal(size=D), rng.normal(size=D)
    for ket in (False, True):
        lin = hostmath.fold_linear_operators(_t(c), _t(m), _t(G), _t(G0), _t(q0), _t(p0), ket=ket)
        for K in (None, np.zeros((M, D, D))):
            u, w, kap, lam, R = folded(c, m, K, G, G0, q0, p0, ket)
            assert R == 0 and (lam == 1.0).all()
            assert all(np.array_equal(a[:, 0], b.numpy()) for a, b in zip((u, w, kap), lin))


# ------------------------------------------------------------------------------------------- 5. the 5 sigma check, on the CPU

def test_closed_form_matches_quadrature_1d():
    """<phi_0|A B|phi_0> = int |phi_0(x)|^2 A(x) B(x) dx at D = 1 on a grid (9 widths, 25 points per width) against the closed form"""
    rng = np.random.default_rng(51)
    G0, q0, p0 = np.array([[1.7]]), np.array([0.6]), np.array([-0.9])
    bra = (rng.normal(size=4), rng.normal(size=(4, 1)), rng.normal(size=(4, 1, 1)))
    ket = (rng.normal(size=4), rng.normal(size=(4, 1)), rng.normal(size=(4, 1, 1)))
    x = np.arange(-14.0, 14.0 + 1e-9, 0.02)[None, :]
    weight = abs(gaussian(q0, p0, G0, x)) ** 2 * 0.02
    value = lambda s: s[0][:, None] + s[1] @ x + 0.5 * s[2][:, 0] * x ** 2
    quad = (value(bra) * value(ket)) @ weight
    exact = closed_form_t0(bra, ket, G0, q0)
    dev = abs(quad - exact) / abs(exact)
    print(f"closed form at t = 0 against quadrature, D = 1: {dev.max():.2e}")
    assert (dev <= 1e-10).all()


def test_five_sigma_at_t0_on_the_cpu():
    """the restatement on the fixture's (zi, probi) at t = 0 lies within 5 sigma of <phi_0|A B|phi_0> for the three pairs of the GPU
    test (test_opquad_gpu.py::test_standard_errors_cover_the_closed_form); the pairs were chosen to stay within 3 sigma here"""
    from semiclassical_amd import hostmath
    g = cases.load("hk_as5_chi002")
    D, n = g["q0"].shape[0], g["zi"].shape[1]
    q, p = g["zi"][:D], g["zi"][D:]
    bra, ket = t0_operator_pairs(D)
    rows = restated_opquad(bra, ket, q, p, q, p, initial_terms(g), g["Gamma_i"], g["Gamma_t"], g["Gamma_0"], g["q0"], g["p0"])
    X = rows[:, 0] + 1j * rows[:, 1]
    sigma = hostmath.standard_errors(X, rows[:, 2:5], n)
    exact = closed_form_t0(bra, ket, g["Gamma_0"], g["q0"])
    multiples = np.stack((abs((X - exact).real) / sigma.real, abs((X - exact).imag) / np.maximum(sigma.imag, 1e-300)), axis=1)
    for a in range(3):
        print(f"pair {a}: X {X[a]:.6f}  exact {exact[a]:.6f}  sigma {sigma[a]:.2e}  |dev| / sigma {multiples[a, 0]:.2f}, {multiples[a, 1]:.2f}")
    assert (sigma.real > 0.01 * abs(exact)).all() and (sigma.real < 0.5 * abs(exact)).all()      # error bars that mean something
    assert within_five_sigma(X, sigma, exact).all()
    resolved = sigma.imag > 1e-12 * abs(exact)                      # (a degenerate component: sigma is rounding noise)
    assert (multiples[:, 0] <= 3.0).all() and (multiples[:, 1][resolved] <= 3.0).all()


# ------------------------------------------------------------------------------------------- 6. the result file

def _operators(rng, M, D, hessians=True):
    ops = {"bra_c": rng.normal(size=M), "bra_m": rng.normal(size=(M, D)), "ket_c": rng.normal(size=M), "ket_m": rng.normal(size=(M, D))}
    if hessians:
        ops.update(bra_k=np.array([random_symmetric(rng, D, D) for _ in range(M)]), ket_k=np.array([random_symmetric(rng, D, 1) for _ in range(M)]))
    return ops


def _record(rng, nt, ops, n):
    raw, x = _batch(rng, nt, ops["bra_c"].shape[0], n)
    return np.ones(nt, dtype=complex), dict(ops, correlation=raw[:, :, 0] + 1j * raw[:, :, 1], second_moment=n * raw[:, :, 2:5]), x


def test_store_pools_batches_with_k(tmp_path):
    rng = np.random.default_rng(61)
    nt, M, D, n1, n2 = 3, 2, 2, 30, 50
    ops = _operators(rng, M, D)
    a1, r1, x1 = _record(rng, nt, ops, n1)
    a2, r2, x2 = _record(rng, nt, ops, n2)
    store = _store(tmp_path, "two.npz", nt)
    store.add_batch(a1, a1, n1, operators=r1)
    store.add_batch(a2, a2, n2, operators=r2)
    got = dict(np.load(store.path))
    assert all(np.array_equal(got["operator_" + key], ops[key]) for key in ops) and got["operator_bra_k"].shape == (M, D, D)
    x = np.concatenate((n1 * x1, n2 * x2), axis=2) / (n1 + n2)
    assert np.allclose(got["operator_correlation"], x.sum(2), rtol=1e-13, atol=0) and int(got["trajectories"]) == n1 + n2


def test_store_refuses_another_k(tmp_path):
    import torch
    from semiclassical_amd import driver
    rng = np.random.default_rng(62)
    nt, M, D = 3, 2, 2
    ops = _operators(rng, M, D)
    store = _store(tmp_path, "k.npz", nt)
    a, r, _ = _record(rng, nt, ops, 20)
    store.add_batch(a, a, 20, operators=r)
    before = dict(np.load(store.path))
    linear = {key: r[key] for key in r if not key.endswith("_k")}
    for other in (dict(r, bra_k=ops["bra_k"] + 1e-9), dict(r, ket_k=ops["ket_k"][::-1].copy()), linear,
                  dict(linear, bra_k=ops["bra_k"]), dict(r, ket_k=np.zeros((M, D, D)))):
        with pytest.raises(driver.ConfigurationError):
            store.add_batch(a, a, 20, operators=other)
    after = dict(np.load(store.path))
    assert set(before) == set(after) and all(np.array_equal(before[k], after[k]) for k in before)
    # start() refuses before any trajectory runs
    task, times = {"results": {"overwrite": False}}, torch.linspace(0.0, 1.0, nt)
    same = tuple(ops[key] for key in ("bra_c", "bra_m", "ket_c", "ket_m", "bra_k", "ket_k"))
    store.start(task, "HK", times, None, operators=same)
    for other in (same[:4], same[:4] + (same[4] + 1.0, same[5]), same[:5] + (np.zeros((M, D, D)),)):
        with pytest.raises(driver.ConfigurationError):
            store.start(task, "HK", times, None, operators=other)


def test_store_without_k_is_unchanged(tmp_path):
    """a file written without K has the keys it had, accepts a task without K and one with all-zero K, and refuses a K"""
    import torch
    from semiclassical_amd import driver
    rng = np.random.default_rng(63)
    nt, M, D = 3, 2, 2
    ops = _operators(rng, M, D, hessians=False)
    store = _store(tmp_path, "plain.npz", nt)
    a, r, _ = _record(rng, nt, ops, 20)
    store.add_batch(a, a, 20, operators=r)
    keys = set(np.load(store.path).keys())
    assert keys == {"propagator", "times", "autocorrelation", "ic_correlation", "adiabatic_gap", "zero_point_energy", "trajectories",
                    "operator_bra_c", "operator_bra_m", "operator_ket_c", "operator_ket_m", "operator_correlation",
                    "operator_correlation_second_moment", "operator_correlation_error"}
    assert keys - set(driver.CorrelationStore.OPERATOR_KEYS + driver.CorrelationStore.OPERATOR_ERROR_KEYS) == {
        "propagator", "times", "autocorrelation", "ic_correlation", "adiabatic_gap", "zero_point_energy", "trajectories"}
    store.add_batch(a, a, 20, operators=r)
    assert set(np.load(store.path).keys()) == keys and int(np.load(store.path)["trajectories"]) == 40
    task, times = {"results": {"overwrite": False}}, torch.linspace(0.0, 1.0, nt)
    same = tuple(ops[key] for key in ("bra_c", "bra_m", "ket_c", "ket_m"))
    zeros = np.zeros((M, D, D))
    store.start(task, "HK", times, None, operators=same)
    store.start(task, "HK", times, None, operators=same + (zeros, zeros))
    before = dict(np.load(store.path))
    quadratic = same + (np.array([random_symmetric(rng, D, 1)] * M), zeros)
    with pytest.raises(driver.ConfigurationError):
        store.start(task, "HK", times, None, operators=quadratic)
    with pytest.raises(driver.ConfigurationError):
        store.add_batch(a, a, 20, operators=dict(r, bra_k=quadratic[4], ket_k=zeros))
    after = dict(np.load(store.path))
    assert set(before) == set(after) and all(np.array_equal(before[k], after[k]) for k in before)


def test_driver_loads_k(tmp_path):
    from semiclassical_amd import driver
    rng = np.random.default_rng(64)
    M, D = 2, 3
    c, m = np.zeros(M), np.ones((M, D))
    k, k2 = (np.array([random_symmetric(rng, D, 2) for _ in range(M)]) for _ in range(2))
    load = lambda **arrays: (np.savez(tmp_path / "o.npz", **arrays), driver._load_operators(str(tmp_path / "o.npz"), D))[1]
    assert len(load(bra_c=c, bra_m=m)) == 4                          # as before
    out = load(bra_c=c, bra_m=m, bra_k=k)
    assert len(out) == 6 and np.array_equal(out[4], k) and np.array_equal(out[5], k)      # the ket takes the bra's, K included
    out = load(bra_c=c, bra_m=m, bra_k=k, ket_k=k2)
    assert np.array_equal(out[2], c) and np.array_equal(out[5], k2)
    out = load(bra_c=c, bra_m=m, bra_k=k, ket_c=c + 1.0, ket_m=m)
    assert np.array_equal(out[4], k) and not out[5].any()            # a ket of its own without ket_k is linear
    out = load(bra_c=c, bra_m=m, ket_k=k2)
    assert not out[4].any() and np.array_equal(out[5], k2)
    bra, ket = driver.ROW_FAMILIES[1].as_run(out)
    assert len(bra) == len(ket) == 3 and bra[2] is out[4] and ket[2] is out[5] and ket[0] is out[2]
    assert driver.ROW_FAMILIES[1].as_run(out[:4]) == ((out[0], out[1]), (out[2], out[3]))
    skew = k.copy()
    skew[0, 0, 1] += 1.0
    for bad in (k[:, 0], k[:1], skew, np.full((M, D, D), np.nan)):
        with pytest.raises(driver.ConfigurationError):
            load(bra_c=c, bra_m=m, bra_k=bad)


# ------------------------------------------------------------------------------------------- 7. ABI

def test_symbols_are_declared_bound_and_exported():
    from semiclassical_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "semiclassical_hip.h")).read()
    for name in ("sc_hk_opquad", "sc_hk_opquad_initial", "sc_hk_opquad_rows"):
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    declared = set(re.findall(r"^(?:int|int64_t|const char \*)\s*(sc_\w+)\s*\(", header, flags=re.M))
    assert declared and declared <= set(_lib.SIGNATURES), declared - set(_lib.SIGNATURES)
    assert all(hasattr(_lib.lib, name) for name in declared)
    assert int(re.search(r"#define SC_ABI_VERSION\s+(\d+)", header).group(1)) == 18
    assert _lib.lib.sc_abi_version() == _lib.ABI_VERSION == 18
    rows = _lib.lib.sc_hk_opquad_rows
    assert rows(1, 1) == 1 and rows(64, 500) == 1 and rows(65, 1) == 2 and rows(130, 65) == 3 and rows(0, 5) == 0 and rows(5, 0) == 0
