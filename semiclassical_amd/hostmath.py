"""Small host-side linear algebra of the propagators (O(D^3), once per run).

Everything here is plain fp64 torch on the CPU: eigen-decompositions of the
D x D width matrices and the constants the HIP kernels consume.  It mirrors the
setup code of reference semiclassical/propagators.py (cited per function) and is
deliberately kept off the GPU so that results do not depend on the device
eigen-solver (eigenvector gauge).
"""
import math

import numpy as np
import torch

from .units import hbar

ZERO = 1.0e-8          # reference propagators.py:16
C128 = torch.complex128


def _eigh(A):
    return torch.linalg.eigh(A, UPLO='U')


def as_f64(x):
    return torch.as_tensor(x, dtype=torch.float64, device='cpu').detach().clone()


def sym_sqrtm(A):
    """A^{1/2} and pseudo-inverse A^{-1/2}, complex (D,D).  propagators.py:25-59"""
    w, V = _eigh(A)
    keep = abs(w) > ZERO
    wc, Vc = w.type(C128), V.type(C128)
    root = torch.einsum('ij,j,kj->ik', Vc, torch.sqrt(wc), Vc)
    iroot = torch.einsum('ij,j,kj->ik', Vc[:, keep], 1.0 / torch.sqrt(wc[keep]), Vc[:, keep])
    return root, iroot


def psd_sqrt_real(A):
    """real symmetric L with L L = A for a symmetric non-negative A (eigenvalues below zero by rounding are clamped)"""
    w, V = _eigh(A)
    return torch.einsum('ij,j,kj->ik', V, torch.sqrt(torch.clamp(w, min=0.0)), V)


def wavepacket_norm_factor(G):
    """(det'(G) / pi^rank)^(1/4), det' over the non-zero eigenvalues.  propagators.py:244-250, 284"""
    e, _ = _eigh(G)
    keep = abs(e) > ZERO
    return float((torch.prod(e[keep]) / np.pi ** int(torch.count_nonzero(keep))) ** 0.25)


def is_symmetric_non_negative(A, eps=1.0e-6):
    """propagators.py:61-82"""
    if torch.sum(abs(A - A.T)) / torch.sum(abs(A)) > eps:
        return False
    w, _ = _eigh(A)
    return bool((w >= -ZERO).all())


def is_diagonal(A):
    return bool((A - torch.diag(torch.diagonal(A)) == 0).all())


def sampling_matrices(Gamma_i, Gamma_0):
    """U, iGi0, iLz, detLz, d' of initial_conditions.  propagators.py:493-531"""
    wp, Vp = _eigh(Gamma_0 + Gamma_i)
    nzp = wp > ZERO
    U = Vp[:, nzp].type(C128)
    iGi0 = torch.einsum('ij,j,kj->ik', Vp[:, nzp], 1.0 / wp[nzp], Vp[:, nzp])
    iLp = torch.einsum('i,ji->ij', torch.sqrt(wp[nzp] / 2), Vp[:, nzp])
    wq, Vq = _eigh(Gamma_i @ iGi0 @ Gamma_0)
    nzq = wq > ZERO
    iLq = torch.einsum('i,ji->ij', 1.0 / torch.sqrt(2 * wq[nzq]), Vq[:, nzq])
    dprime = int(torch.count_nonzero(nzp))
    assert dprime == int(torch.count_nonzero(nzq)), \
        "number of non-zero modes for sampling of positions and momenta have to be the same"
    iLz = torch.block_diag(iLq, iLp)
    detLz = torch.prod(2 * torch.sqrt(wq[nzq] / wp[nzp]))
    return U, iGi0, iLz, detLz, dprime


class ThermalConstants(object):
    """Normal modes of the harmonic INITIAL surface and the Glauber-Sudarshan P function of its canonical density operator at
    ``temperature`` = k_B T in Hartree (not in the reference).

    The ground state of the surface has the width Gamma_0 and the masses m: W = m^-1/2 Gamma_0 m^-1/2 hbar = L diag(omega) L^T.
    The d'' modes with omega_k > ZERO are the thermal modes (the rule of ``sampling_matrices`` for the range of a singular
    width); zero modes carry no thermal population.  In mass-weighted normal coordinates the centres of the mixture are
    Q_k ~ N(0, hbar nbar_k / omega_k), P_k ~ N(0, hbar nbar_k omega_k), nbar_k = 1 / (exp(hbar omega_k / k_B T) - 1); their
    Cartesian images are a = q0 + map_q Q, b = map_p P with map_q = m^-1/2 L, map_p = m^1/2 L (D, d'').

    ``diag``: Gamma_0 is diagonal and every mode is thermal -- mode k is coordinate k (no eigen-solver, no reordering) and the
    maps are per-mode scales ``scale_q`` = m^-1/2, ``scale_p`` = m^1/2.  ``p0``, if given, has to be zero: the minimum of the
    initial surface is at rest.  ValueError for p0 != 0, a negative or non-finite temperature, or masses that are not (D,)
    positive numbers."""

    def __init__(self, Gamma_0, masses, temperature, p0=None):
        Gamma_0, masses = as_f64(Gamma_0), as_f64(masses)
        D = Gamma_0.shape[0]
        if masses.dim() != 1 or masses.shape[0] != D or not bool((masses > 0).all()) or not bool(torch.isfinite(masses).all()):
            raise ValueError(f"thermal ensemble: masses of shape ({D},), positive, are expected, got shape {tuple(masses.shape)}")
        temperature = float(temperature)
        if not (temperature >= 0.0 and math.isfinite(temperature)):
            raise ValueError(f"thermal ensemble: the temperature k_B T has to be a non-negative number, got {temperature}")
        if p0 is not None and bool((as_f64(p0) != 0).any()):
            raise ValueError("thermal ensemble: p0 has to be zero -- the initial surface is harmonic around (q0, 0); a moving "
                             "wavepacket is not its thermal state")
        isq = 1.0 / torch.sqrt(masses)
        full_diag = is_diagonal(Gamma_0) and bool((torch.diagonal(Gamma_0) * isq * isq * hbar > ZERO).all())
        if full_diag:
            omega, L = torch.diagonal(Gamma_0) * isq * isq * hbar, torch.eye(D, dtype=torch.float64)
        else:
            w, V = _eigh(isq.unsqueeze(1) * Gamma_0 * isq.unsqueeze(0) * hbar)
            keep = w > ZERO
            omega, L = w[keep], V[:, keep]
        self.dim, self.dmodes, self.diag = D, int(omega.shape[0]), bool(full_diag)
        if self.dmodes == 0:
            raise ValueError("thermal ensemble: Gamma_0 has no mode with a positive frequency")
        self.temperature, self.masses = temperature, masses
        self.omega, self.L = omega.contiguous(), L.contiguous()
        self.scale_q, self.scale_p = isq.contiguous(), torch.sqrt(masses).contiguous()
        self.map_q = (isq.unsqueeze(1) * L).contiguous()
        self.map_p = (torch.sqrt(masses).unsqueeze(1) * L).contiguous()
        if temperature > 0.0:
            self.nbar = 1.0 / torch.expm1(hbar * omega / temperature)
        else:
            self.nbar = torch.zeros_like(omega)
        self.sigma_q = torch.sqrt(hbar * self.nbar / omega)
        self.sigma_p = torch.sqrt(hbar * self.nbar * omega)

    def draw_centres(self, ntraj, generator=None):
        """(ntraj, 2 d'') centres (Q | P) from torch's CPU generator"""
        g = torch.randn((int(ntraj), 2 * self.dmodes), dtype=torch.float64, generator=generator)
        return g * torch.cat((self.sigma_q, self.sigma_p)).unsqueeze(0)

    def cartesian(self, centres):
        """(a (n, D), b (n, D)) of centres (n, 2 d'') at t = 0, on the host"""
        c = torch.as_tensor(centres, dtype=torch.float64).cpu()
        return c[:, :self.dmodes] @ self.map_q.T, c[:, self.dmodes:] @ self.map_p.T


class OverlapConstants(object):
    """constants of <q,p,Gi|q',p',Gj>.  propagators.py:125-179, 230"""

    def __init__(self, Gi, Gj):
        assert Gi.shape == Gj.shape, "width matrices Gi and Gj have to have the same shape"
        ei, _ = _eigh(Gi)
        ej, _ = _eigh(Gj)
        self.rank = int(torch.count_nonzero(abs(ei) > ZERO))
        assert self.rank == int(torch.count_nonzero(abs(ej) > ZERO)), \
            "Gi and Gj have to have the same rank and null space."
        detGi = torch.prod(ei[abs(ei) > ZERO])
        detGj = torch.prod(ej[abs(ej) > ZERO])
        eij, Vij = _eigh(Gi + Gj)
        keep = abs(eij) > ZERO
        self.B = torch.einsum('ij,j,kj->ik', Vij[:, keep], 1.0 / eij[keep], Vij[:, keep])   # (Gi+Gj)^+
        detGij = torch.prod(eij[keep])
        self.A = Gi @ self.B @ Gj
        self.C = Gj @ self.B
        self.fac = float(torch.sqrt(2.0 ** self.rank * torch.sqrt(detGi) * torch.sqrt(detGj) / detGij))
        self.diag = is_diagonal(self.A) and is_diagonal(self.B) and is_diagonal(self.C)


class PrefactorConstants(object):
    """constants of the HK prefactor matrix, eqn (29).  propagators.py:438-440, 969-994

    diag:   Gamma_i, Gamma_t diagonal with d' == D -- the sandwiches become elementwise scalings and the
            projection onto U (an orthogonal matrix when d' == D) leaves the determinant unchanged.
    dense:  L1 = U^T Gt^{1/2}, L2 = U^T Gt^{-1/2}, R1 = Gi^{-1/2} U, R2 = Gi^{1/2} U.
    """

    def __init__(self, Gamma_i, Gamma_t, U):
        D, dprime = U.shape
        self.dim, self.dprime = D, dprime
        sqGi, isqGi = sym_sqrtm(Gamma_i)
        sqGt, isqGt = sym_sqrtm(Gamma_t)
        self.sqGi, self.isqGi, self.sqGt, self.isqGt = sqGi, isqGi, sqGt, isqGt
        self.diag = (dprime == D and is_diagonal(Gamma_i) and is_diagonal(Gamma_t)
                     and bool((torch.diagonal(Gamma_i) > ZERO).all()) and bool((torch.diagonal(Gamma_t) > ZERO).all()))
        if self.diag:
            self.st = torch.sqrt(torch.diagonal(Gamma_t)).contiguous()
            self.si = torch.sqrt(torch.diagonal(Gamma_i)).contiguous()
        else:
            self.L1 = (U.T @ sqGt).contiguous()
            self.L2 = (U.T @ isqGt).contiguous()
            self.R1 = (isqGi @ U).contiguous()
            self.R2 = (sqGi @ U).contiguous()


class NacConstants(object):
    """constants of nacQ / nacq.  propagators.py:886-903 (constant coupling vector tau1, tau2 = 0)"""

    def __init__(self, Gamma_0, Gamma_i, iGi0, p0, masses, tau1, tau2_sum=0.0):
        n1 = -hbar ** 2 * tau1 / masses
        G = Gamma_0 @ iGi0
        self.rn = (G @ Gamma_i @ n1).contiguous()
        self.gn = (G.T @ n1).contiguous()
        self.p0n1 = float(torch.dot(p0, n1))
        self.n2 = float(-hbar ** 2 * 0.5 * tau2_sum)


def fold_linear_operators(c, m, G_traj, G_0, q0, p0, ket):
    """(u, w, kappa): the Gaussian matrix element of the linear operators c_a + m_a.x between phi_0 = |q0, p0, G_0> and a
    trajectory's Gaussian |q, p, G_traj>, divided by their overlap, as one affine form  kappa_a + u_a.q + i w_a.p  per operator
    (DESIGN.md section 4.14).  From  <a|x|b> / <a|b> = (G_a + G_b)^+ (G_a q_a + G_b q_b + i (p_b - p_a) / hbar)  with
    S = (G_traj + G_0)^+:  u = G_traj S m,  kappa = c + m.S (G_0 q0 -+ i p0 / hbar),  w = +- S m / hbar -- the upper signs for
    ``ket`` False (phi_0 is the bra: <phi_0|A|q, p>), the lower ones for ``ket`` True (<q, p|B|phi_0>).
    c (M,), m (M, D) real; returns real (M, D), real (M, D), complex (M,).  Singular widths: the pseudo-inverse of
    OverlapConstants; every m_a has to lie in the range of G_traj + G_0 (relative 1e-8, the test of reduced_density), else
    ValueError."""
    e, V = _eigh(G_traj + G_0)
    keep = abs(e) > ZERO
    S = torch.einsum('ij,j,kj->ik', V[:, keep], 1.0 / e[keep], V[:, keep])
    outside = torch.linalg.norm(m - (m @ V[:, keep]) @ V[:, keep].T, dim=1) > 1.0e-8 * torch.linalg.norm(m, dim=1)
    if bool(outside.any()):
        raise ValueError(f"operators: the vector(s) m of operator(s) {torch.nonzero(outside).flatten().tolist()} lie outside the "
                         "range of the sum of the widths: the matrix element along a null direction does not exist")
    Sm = m @ S                                              # rows S m_a (S is symmetric)
    sign = 1.0 if ket else -1.0
    kappa = torch.complex(c + Sm @ (G_0 @ q0), sign / hbar * (Sm @ p0))
    return (Sm @ G_traj).contiguous(), (-sign / hbar * Sm).contiguous(), kappa.contiguous()


def fold_thermal_linear_operators(c, m, G_traj, G_0, q0, tc, ket):
    """(u, w, kappa, ut, wt): ``fold_linear_operators`` for a thermal ensemble, where the fixed Gaussian
    is |a_i, b_i, G_0> with the trajectory's own centre a_i = q0 + map_q Qc_i, b_i = map_p Pc_i (``tc``: the ThermalConstants)
    in the place of (q0, p0 = 0).  The element is  kappa_a + u_a.q + i w_a.p + ut_a.Qc + i wt_a.Pc  with (u, w, kappa) those of
    ``fold_linear_operators`` at p0 = 0 and, S = (G_traj + G_0)^+,  ut = map_q^T G_0 S m,  wt = -+ map_p^T S m / hbar  (upper sign:
    ``ket`` False) -- the kernels never see the Cartesian maps.  With ``tc.diag`` the maps are per-mode scales and ut, wt are
    elementwise products.  Returns real (M, D) twice, complex (M,), real (M, d'') twice; the refusals of
    ``fold_linear_operators``."""
    u, w, kappa = fold_linear_operators(c, m, G_traj, G_0, q0, torch.zeros_like(q0), ket)
    ut, wt = _centre_vectors(w, G_0, tc, ket)
    return u, w, kappa, ut, wt


def _centre_vectors(w, G_0, tc, ket):
    """(ut, wt), rows (., d''), of the rows w = -+ S m / hbar (., D) of ``fold_linear_operators``:  ut = map_q^T G_0 S m,
    wt = -+ map_p^T S m / hbar"""
    sign = 1.0 if ket else -1.0
    SmG0 = (-sign * hbar * w) @ G_0                         # rows (G_0 S m_a)^T: w = -+ S m / hbar
    if tc.diag:
        ut, wt = SmG0 * tc.scale_q.unsqueeze(0), -w * tc.scale_p.unsqueeze(0)
    else:
        ut, wt = SmG0 @ tc.map_q, -w @ tc.map_p
    return ut.contiguous(), wt.contiguous()


def _kept_eigenpairs(Ka, a, name):
    """(lambda_r, v_r as rows) of the symmetric matrix ``Ka`` of operator ``a`` without the pairs of |lambda_r| <= 1e-12 max |lambda|;
    ValueError for a matrix that is not symmetric to 1e-12 of its largest entry"""
    if float(abs(Ka - Ka.T).max()) > 1.0e-12 * float(abs(Ka).max()):
        raise ValueError(f"operators: {name} of operator {a} is not symmetric")
    lam, vec = _eigh(0.5 * (Ka + Ka.T))
    big = abs(lam) > 1.0e-12 * float(abs(lam).max())
    return lam[big], vec[:, big].T.contiguous()


def fold_quadratic_operators(c, m, K, G_traj, G_0, q0, p0, ket):
    """(u, w, kappa, lam, R): the Gaussian matrix element of the quadratic operators c_a + m_a.x + 1/2 x^T K_a x between phi_0 and a
    trajectory's Gaussian, divided by their overlap, as 1 + R COLUMNS per operator.  With x the complex
    mean of ``fold_linear_operators`` and S = (G_traj + G_0)^+ the element is  c + m.x + 1/2 x^T K x + 1/2 tr(K S); with the
    symmetric eigendecomposition K = sum_r lambda_r v_r v_r^T it reads  sum_col lam_col z_col^(p_col),
    z_col = kappa_col + u_col.q + i w_col.p:  column 0 the linear part (p = 1, lam = 1, kappa = that of (c, m) + 1/2 tr(K S)),
    columns 1 ... R the eigenvectors ((u, w, kappa) of the linear operator (0, v_r), p = 2, lam = lambda_r / 2).  Eigenpairs with
    |lambda_r| <= 1e-12 max |lambda| are dropped; R is the largest number kept by an operator, the others are padded with columns
    of zeros.  c (M,), m (M, D), K (M, D, D) real or None (= zeros); returns real (M, 1 + R, D) twice, complex (M, 1 + R), real
    (M, 1 + R) and R.  ValueError for a K that is not symmetric to 1e-12 of its largest entry, a non-finite K, and an m or a kept
    eigenvector outside the range of G_traj + G_0 (the test of ``fold_linear_operators``)."""
    M, D = m.shape
    u0, w0, k0 = fold_linear_operators(c, m, G_traj, G_0, q0, p0, ket)
    kept = []                                               # per operator: (lambda_r, v_r) of the eigenpairs kept
    if K is not None:
        if tuple(K.shape) != (M, D, D):
            raise ValueError(f"operators: K of shape ({M}, {D}, {D}) is expected, got {tuple(K.shape)}")
        if not bool(torch.isfinite(K).all()):
            raise ValueError("operators: non-finite entry in K")
        e, V = _eigh(G_traj + G_0)
        keep = abs(e) > ZERO
        S = torch.einsum('ij,j,kj->ik', V[:, keep], 1.0 / e[keep], V[:, keep])
        k0 = k0.clone()
        for a in range(M):
            Ka = K[a]
            kept.append(_kept_eigenpairs(Ka, a, "K"))
            k0[a] += 0.5 * float(torch.sum(Ka * S))         # tr(K S), both symmetric
    R = max((int(lam.shape[0]) for lam, _ in kept), default=0)
    u, w = torch.zeros((M, 1 + R, D), dtype=torch.float64), torch.zeros((M, 1 + R, D), dtype=torch.float64)
    kappa, lam_out = torch.zeros((M, 1 + R), dtype=C128), torch.zeros((M, 1 + R), dtype=torch.float64)
    u[:, 0], w[:, 0], kappa[:, 0], lam_out[:, 0] = u0, w0, k0, 1.0
    if R == 0:
        return u, w, kappa, lam_out, R
    fold = lambda vec: fold_linear_operators(torch.zeros(vec.shape[0], dtype=torch.float64), vec, G_traj, G_0, q0, p0, ket)
    try:
        ur, wr, kr = fold(torch.cat([vec for _, vec in kept]))          # the eigenvectors of every operator in one call
    except ValueError:
        for a, (lam, vec) in enumerate(kept):                           # ... and one by one to name the operator
            try:
                fold(vec)
            except ValueError:
                raise ValueError(f"operators: K of operator {a} has a component outside the range of the sum of the widths: the "
                                 "matrix element along a null direction does not exist")
        raise
    at = 0
    for a, (lam, vec) in enumerate(kept):
        r = int(lam.shape[0])
        u[a, 1:1 + r], w[a, 1:1 + r], kappa[a, 1:1 + r], lam_out[a, 1:1 + r] = ur[at:at + r], wr[at:at + r], kr[at:at + r], 0.5 * lam
        at += r
    return u, w, kappa, lam_out, R


def fold_thermal_quadratic_operators(c, m, K, G_traj, G_0, q0, tc, ket):
    """(u, w, kappa, lam, ut, wt, R): ``fold_quadratic_operators`` for a thermal ensemble, where the fixed
    Gaussian is |a_i, b_i, G_0> with the trajectory's own centre (``tc``: the ThermalConstants) in the place of (q0, p0 = 0).  A
    column is  z_col = kappa_col + u_col.q + i w_col.p + ut_col.Qc + i wt_col.Pc  and the element  sum_col lam_col z_col^(p_col):
    (u, w, kappa, lam, R) are those of ``fold_quadratic_operators`` at p0 = 0 (1/2 tr(K S) inside kappa of column 0), (ut, wt)
    those of ``fold_thermal_linear_operators`` for (c, m) in column 0 and for the linear operator (0, v_r) of every kept
    eigenvector in the columns 1 ... R, zeros in the padding.  Returns real (M, 1 + R, D) twice, complex (M, 1 + R), real
    (M, 1 + R), real (M, 1 + R, d'') twice and R; the refusals of ``fold_quadratic_operators``."""
    u, w, kappa, lam, R = fold_quadratic_operators(c, m, K, G_traj, G_0, q0, torch.zeros_like(q0), ket)
    M, C1, D = u.shape
    ut, wt = _centre_vectors(w.reshape(M * C1, D), G_0, tc, ket)       # column by column: the padding stays zero
    return u, w, kappa, lam, ut.reshape(M, C1, -1), wt.reshape(M, C1, -1), R


def fold_expectation_operators(c, m, K, n, W, Gamma_t):
    """(uq, up, lam, kappa, R): the matrix element of the operators  c_a + m_a.x + 1/2 x^T K_a x + n_a.p + 1/2 p^T W_a p  between two
    Gaussians |q_i, p_i, Gamma_t>, |q_j, p_j, Gamma_t> of ONE width, divided by their overlap, as 1 + R columns per operator
    (DESIGN.md section 4.21).  With B = (2 Gamma_t)^+ and the complex pair means
        xbar = (q_i + q_j) / 2 + i B (p_j - p_i) / hbar,    pbar = (p_i + p_j) / 2 + i hbar Gamma_t (q_i - q_j) / 2
    the element is  kappa_a + sum_col lam_col z_col^(p_col),  z_col = a_i + conj(a_j),  a_i = uq_col.q_i + up_col.p_i:
        a linear form v.xbar has uq = v / 2, up = -i B v / hbar;   a form v.pbar has up = v / 2, uq = i hbar Gamma_t v / 2;
    column 0 (p = 1, lam = 1) is the sum of the x-form of m and the p-form of n, columns 1 ... R (p = 2, lam = lambda_r / 2) the kept
    eigenpairs of K (x-forms), then of W (p-forms), by the drop rule of ``fold_quadratic_operators``;
    kappa_a = c_a + 1/2 tr(K_a B) + hbar^2 / 4 tr(W_a Gamma_t).  R is the largest number of columns kept by an operator, the others
    are padded with columns of zeros.
    c (M,), m, n (M, D), K, W (M, D, D) real, any of them None (= zeros) but not all; returns complex (M, 1 + R, D) twice, real
    (M, 1 + R), complex (M,) and R.  ValueError for shapes that do not agree, a non-finite entry, a K or W that is not symmetric to
    1e-12 of its largest entry, and an m, n or kept eigenvector outside the range of Gamma_t (relative 1e-8, the test of
    reduced_density), naming the operator."""
    Gamma_t = as_f64(Gamma_t)
    D = Gamma_t.shape[0]
    parts = {}
    for name, val, tail in (("c", c, ()), ("x", m, (D,)), ("xx", K, (D, D)), ("p", n, (D,)), ("pp", W, (D, D))):
        if val is None:
            continue
        try:
            t = as_f64(val)
        except (TypeError, ValueError, RuntimeError) as err:
            raise ValueError(f"operators: {name}: a real array is expected ({err})")
        if t.dim() != 1 + len(tail) or tuple(t.shape[1:]) != tail:
            raise ValueError(f"operators: {name} of shape {('M',) + tail} is expected, got {tuple(t.shape)}")
        if not bool(torch.isfinite(t).all()):
            raise ValueError(f"operators: non-finite entry in {name}")
        parts[name] = t
    if not parts:
        raise ValueError("operators: at least one of c, x, xx, p, pp has to be given")
    counts = {name: int(t.shape[0]) for name, t in parts.items()}
    M = next(iter(counts.values()))
    if M < 1 or any(v != M for v in counts.values()):
        raise ValueError(f"operators: the parts have to hold the same number M >= 1 of operators, got {counts}")
    e, V = _eigh(Gamma_t)
    keep = abs(e) > ZERO
    Vk = V[:, keep]
    B = torch.einsum('ij,j,kj->ik', Vk, 0.5 / e[keep], Vk)          # (2 Gamma_t)^+

    def in_range(vec, a, what):
        outside = torch.linalg.norm(vec - (vec @ Vk) @ Vk.T, dim=1) > 1.0e-8 * torch.linalg.norm(vec, dim=1)
        if bool(outside.any()):
            raise ValueError(f"operators: {what} of operator {a} has a component outside the range of Gamma_t: the matrix element "
                             "along a null direction does not exist")

    x_form = lambda vec: (torch.complex(0.5 * vec, torch.zeros_like(vec)), torch.complex(torch.zeros_like(vec), -(vec @ B) / hbar))
    p_form = lambda vec: (torch.complex(torch.zeros_like(vec), 0.5 * hbar * (vec @ Gamma_t)), torch.complex(0.5 * vec, torch.zeros_like(vec)))
    kappa = torch.zeros(M, dtype=C128)
    if "c" in parts:
        kappa += parts["c"]
    cols = []                                               # per operator: (lam, uq, up) of the squared columns
    for a in range(M):
        lam_a, uq_a, up_a = [], [], []
        for name, form, weight in (("xx", x_form, B), ("pp", p_form, 0.5 * hbar ** 2 * Gamma_t)):
            if name not in parts:
                continue
            Ma = parts[name][a]
            lam, vec = _kept_eigenpairs(Ma, a, name)
            in_range(vec, a, name)
            kappa[a] += 0.5 * float(torch.sum(Ma * weight))   # 1/2 tr(K B), hbar^2 / 4 tr(W Gamma_t): both factors symmetric
            uq, up = form(vec)
            lam_a.append(0.5 * lam)
            uq_a.append(uq)
            up_a.append(up)
        cols.append((torch.cat(lam_a), torch.cat(uq_a), torch.cat(up_a)) if lam_a else None)
    R = max((int(t[0].shape[0]) for t in cols if t is not None), default=0)
    uq, up = torch.zeros((M, 1 + R, D), dtype=C128), torch.zeros((M, 1 + R, D), dtype=C128)
    lam_out = torch.zeros((M, 1 + R), dtype=torch.float64)
    lam_out[:, 0] = 1.0
    for name, form in (("x", x_form), ("p", p_form)):
        if name in parts:
            for a in range(M):
                in_range(parts[name][a:a + 1], a, name)
            fq, fp = form(parts[name])
            uq[:, 0] += fq
            up[:, 0] += fp
    for a, t in enumerate(cols):
        if t is not None:
            r = int(t[0].shape[0])
            lam_out[a, 1:1 + r], uq[a, 1:1 + r], up[a, 1:1 + r] = t
    return uq.contiguous(), up.contiguous(), lam_out.contiguous(), kappa.contiguous(), R


def fold_wm_expectation_operators(c, m, K, n, U):
    """(vx, nvec, lam, kappa, R): the operators  c_a + m_a.x + 1/2 x^T K_a x + n_a.p  (p = -i hbar d/dx acting on the ket) between two
    Walton-Manolopoulos Gaussians g_i, g_j of per-trajectory widths, divided by their overlap, as 1 + R columns per operator
    (DESIGN.md section 4.24).  With the pair mean  xbar = Q_i + U D'^-1 b'  and the covariance  U D'^-1 U^T  the element is
        kappa_a + sum_col lam_col f_col,    f_0 = l_0,    f_col = l_col^2 + (U^T v_col)^T D'^-1 (U^T v_col)  (col = 1 ... R),
        l_0 = m.xbar - i hbar [ n.d_j - (C_j n).(xbar - Q_j) ],    l_col = v_col.xbar:
    column 0 (lam = 1) is the x-form of m plus the p-form of n, columns 1 ... R (lam = lambda_r / 2) the kept eigenpairs of K by the
    drop rule of ``fold_quadratic_operators``; kappa_a = c_a.  This part does not depend on the trajectories: ``vx`` (M, 1 + R, D)
    holds m and the eigenvectors, ``nvec`` (M, D) the vectors n, or None without p; ``wm_expectation_columns`` makes the columns of
    a state from them.  R is the largest number of columns kept by an operator, the others are padded with columns of zeros.
    c (M,), m, n (M, D), K (M, D, D) real, any of them None (= zeros) but not all; U (D, d') real with orthonormal columns spans the
    non-zero width modes.  ValueError for shapes that do not agree, a non-finite entry, a K that is not symmetric to 1e-12 of its
    largest entry, and an m, n or kept eigenvector outside the range of U (relative 1e-8, the test of reduced_density), naming the
    operator."""
    U = as_f64(U)
    D = U.shape[0]
    parts = {}
    for name, val, tail in (("c", c, ()), ("x", m, (D,)), ("xx", K, (D, D)), ("p", n, (D,))):
        if val is None:
            continue
        try:
            t = as_f64(val)
        except (TypeError, ValueError, RuntimeError) as err:
            raise ValueError(f"operators: {name}: a real array is expected ({err})")
        if t.dim() != 1 + len(tail) or tuple(t.shape[1:]) != tail:
            raise ValueError(f"operators: {name} of shape {('M',) + tail} is expected, got {tuple(t.shape)}")
        if not bool(torch.isfinite(t).all()):
            raise ValueError(f"operators: non-finite entry in {name}")
        parts[name] = t
    if not parts:
        raise ValueError("operators: at least one of c, x, xx, p has to be given")
    counts = {name: int(t.shape[0]) for name, t in parts.items()}
    M = next(iter(counts.values()))
    if M < 1 or any(v != M for v in counts.values()):
        raise ValueError(f"operators: the parts have to hold the same number M >= 1 of operators, got {counts}")

    def in_range(vec, a, what):
        outside = torch.linalg.norm(vec - (vec @ U) @ U.T, dim=1) > 1.0e-8 * torch.linalg.norm(vec, dim=1)
        if bool(outside.any()):
            raise ValueError(f"operators: {what} of operator {a} has a component outside the range of the widths: the matrix "
                             "element along a null direction does not exist")

    for name in ("x", "p"):
        if name in parts:
            for a in range(M):
                in_range(parts[name][a:a + 1], a, name)
    kept = []
    if "xx" in parts:
        for a in range(M):
            lam, vec = _kept_eigenpairs(parts["xx"][a], a, "xx")
            in_range(vec, a, "xx")
            kept.append((0.5 * lam, vec))
    R = max((int(lam.shape[0]) for lam, _ in kept), default=0)
    vx = torch.zeros((M, 1 + R, D), dtype=torch.float64)
    lam_out = torch.zeros((M, 1 + R), dtype=torch.float64)
    lam_out[:, 0] = 1.0
    if "x" in parts:
        vx[:, 0] = parts["x"]
    for a, (lam, vec) in enumerate(kept):
        r = int(lam.shape[0])
        lam_out[a, 1:1 + r], vx[a, 1:1 + r] = lam, vec
    kappa = torch.zeros(M, dtype=C128)
    if "c" in parts:
        kappa += parts["c"]
    nvec = parts["p"].contiguous() if "p" in parts else None
    return vx.contiguous(), nvec, lam_out.contiguous(), kappa.contiguous(), R


def wm_expectation_columns(vx, nvec, Qi, dvecp_i, Qj, cqq_j, dvec_j, dvecp_j, U):
    """(za, zb, g, sfix, sket): the columns of ``fold_wm_expectation_operators`` for bras i and kets j, as sc_wm_pair_expect takes
    them.  The linear form of column col is
        l_col = za[col][i] + zb[col][j] + g_col . b' + s_col^T D'^-1 b',    s_col = sfix[col] (+ sket[a][j] for column 0 of operator a),
    with D', b' of the pair (C_j dQ enters through b' alone: for n = U n',  (C_j n).(Q_i - Q_j) = -n'.(b' - conj d'_i - d'_j)):
        x-form of v:   za = v.Q_i,   sfix = U^T v;
        p-form of n:   za = i hbar n'.conj(d'_i),   zb = -i hbar n.d_j + i hbar n'.d'_j,   g = -i hbar n',   sket = i hbar U^T C_j n.
    vx (M, 1 + R, D), nvec (M, D) or None on the host; Qi (ni, D), dvecp_i (ni, d'), Qj (nj, D), cqq_j (nj, D, D), dvec_j (nj, D),
    dvecp_j (nj, d'), U (D, d') on one device.  Returns za (C, ni), zb (C, nj), g, sfix (C, d') complex, C = M (1 + R), and sket
    (M, nj, d') complex or None (no p)."""
    dev = Qi.device
    M, C1, D = vx.shape
    Uc = U.type(C128)
    v = vx.reshape(M * C1, D).to(dev)
    za = (v @ Qi.T).type(C128)
    zb = torch.zeros((M * C1, Qj.shape[0]), dtype=C128, device=dev)
    sfix = (v @ U).type(C128)
    g = torch.zeros_like(sfix)
    sket = None
    if nvec is not None:
        nv = nvec.to(dev).type(C128)                       # (M, D)
        npr = nv @ Uc                                       # n' = U^T n
        col0 = torch.arange(M, device=dev) * C1
        za[col0] += 1j * hbar * (npr @ dvecp_i.conj().T)
        zb[col0] += -1j * hbar * (nv @ dvec_j.T) + 1j * hbar * (npr @ dvecp_j.T)
        g[col0] += -1j * hbar * npr
        sket = (1j * hbar * torch.einsum('jab,mb,ak->mjk', cqq_j, nv, Uc)).contiguous()
    return za.contiguous(), zb.contiguous(), g.contiguous(), sfix.contiguous(), sket


def wm_expectation_launches(lam, cap):
    """The operator set of ``fold_wm_expectation_operators`` cut into calls of sc_wm_pair_expect that hold at most ``cap`` >= 2
    columns each.  A call carries operators of 1 + R' columns, R' = min(R, cap - 1); an operator of more squared columns is cut into
    several such pieces (F is the sum of its columns: the first piece carries column 0 and kappa, the others a column 0 of zeros),
    pieces whose lam are all zero are left out.  lam (M, 1 + R).  Returns (R', calls): every call a list of pieces
    (operator, carries column 0, [indices of its squared columns in 1 ... R]), cap // (1 + R') pieces at the most."""
    M, C1 = lam.shape
    Rl = min(C1 - 1, cap - 1)
    pieces = []
    for a in range(M):
        pieces.append((a, True, list(range(1, 1 + Rl))))
        for r0 in range(1 + Rl, C1, max(Rl, 1)):
            sq = list(range(r0, min(r0 + Rl, C1)))
            if bool((lam[a, sq] != 0).any()):
                pieces.append((a, False, sq))
    per = cap // (1 + Rl)
    return Rl, [pieces[k:k + per] for k in range(0, len(pieces), per)]


def fold_wm_operator_columns(c, m, K, n, W, ex, U):
    """(vx, vp, kind, lam, kappa, cols): the operators  c_a + m_a.x + 1/2 x^T K_a x + n_a.p + 1/2 p^T W_a p + sum_e w_a,e exp(-a_a,e . x)
    (p = -i hbar d/dx acting on the ket) between two Walton-Manolopoulos Gaussians g_i, g_j of per-trajectory widths, divided by their
    overlap, as ``cols`` columns per operator.  With the pair mean xbar and the covariance B = U D'^-1 U^T of
    ``fold_wm_expectation_operators`` and L_j(x) = d_j - C_j (x - Q_j), the ket's logarithmic derivative, the element is
        kappa_a + sum_col lam_col f_col,     kind 0: f = l,     kind 1: f = l^2 + s^T D'^-1 s,     kind 2: f = exp(-l + 1/2 s^T D'^-1 s),
        x-form of v:  l = v.xbar,  s = U^T v;          p-form of w:  l = -i hbar w.L_j(xbar),  s = i hbar U^T C_j w  (per ket):
    column 0 (kind 0, lam = 1) is the x-form of m plus the p-form of n; then the kept eigenpairs of K (kind 1, x-forms, lam =
    lambda_r / 2), the kept eigenpairs of W (kind 1, p-forms, lam = mu_r / 2: p^T W p g_j = -hbar^2 [L_j^T W L_j - tr(W C_j)] g_j; the
    constant hbar^2 / 2 sum_r mu_r w_r^T C_j w_r is added by ``wm_operator_columns``), both by the drop rule of
    ``fold_quadratic_operators``, and the exponential terms with w_e != 0 (kind 2, x-forms of a_e, lam = w_e); kappa_a = c_a.  cols is
    1 + the largest number of such columns of an operator, the others are padded with columns of kind 0, lam = 0 and zero vectors.
    c (M,), m, n (M, D), K, W (M, D, D) real, ex = (w (M, P), a (M, P, D)) real, any of them None (= zeros) but not all; U (D, d') real
    with orthonormal columns spans the non-zero width modes.  Returns vx, vp (M, cols, D) real -- the vectors of the x-forms and of
    the p-forms --, kind (M, cols) int32, lam (M, cols) real, kappa (M,) complex.  ValueError for shapes that do not agree, a
    non-finite entry, a K or W that is not symmetric to 1e-12 of its largest entry, and an m, n, kept eigenvector or a_e outside the
    range of U (relative 1e-8, the test of ``fold_wm_expectation_operators``), naming the operator and the part."""
    U = as_f64(U)
    D = U.shape[0]
    parts = {}
    for name, val, tail in (("c", c, ()), ("x", m, (D,)), ("xx", K, (D, D)), ("p", n, (D,)), ("pp", W, (D, D))):
        if val is None:
            continue
        try:
            t = as_f64(val)
        except (TypeError, ValueError, RuntimeError) as err:
            raise ValueError(f"operators: {name}: a real array is expected ({err})")
        if t.dim() != 1 + len(tail) or tuple(t.shape[1:]) != tail:
            raise ValueError(f"operators: {name} of shape {('M',) + tail} is expected, got {tuple(t.shape)}")
        if not bool(torch.isfinite(t).all()):
            raise ValueError(f"operators: non-finite entry in {name}")
        parts[name] = t
    counts = {name: int(t.shape[0]) for name, t in parts.items()}
    if ex is not None:
        if not isinstance(ex, (tuple, list)) or len(ex) != 2:
            raise ValueError("operators: ex = (w, a) with w of shape (M, P) and a of shape (M, P, D) is expected")
        try:
            ew, ea = as_f64(ex[0]), as_f64(ex[1])
        except (TypeError, ValueError, RuntimeError) as err:
            raise ValueError(f"operators: ex: a pair (w, a) of real arrays is expected ({err})")
        if ew.dim() != 2 or ea.dim() != 3 or tuple(ea.shape) != tuple(ew.shape) + (D,):
            raise ValueError(f"operators: ex = (w, a) with w of shape (M, P) and a of shape (M, P, {D}) is expected, got "
                             f"{tuple(ew.shape)} and {tuple(ea.shape)}")
        if not bool(torch.isfinite(ew).all()) or not bool(torch.isfinite(ea).all()):
            raise ValueError("operators: non-finite entry in ex")
        counts["ex"] = int(ew.shape[0])
    if not counts:
        raise ValueError("operators: at least one of c, x, xx, p, pp, ex has to be given")
    M = next(iter(counts.values()))
    if M < 1 or any(v != M for v in counts.values()):
        raise ValueError(f"operators: the parts have to hold the same number M >= 1 of operators, got {counts}")

    def in_range(vec, a, what):
        outside = torch.linalg.norm(vec - (vec @ U) @ U.T, dim=1) > 1.0e-8 * torch.linalg.norm(vec, dim=1)
        if bool(outside.any()):
            raise ValueError(f"operators: {what} of operator {a} has a component outside the range of the widths: the matrix "
                             "element along a null direction does not exist")

    for name in ("x", "p"):
        if name in parts:
            for a in range(M):
                in_range(parts[name][a:a + 1], a, name)
    columns = []                                            # per operator: (kind, lam, x-form vector or None, p-form vector or None)
    for a in range(M):
        mine = []
        for name in ("xx", "pp"):
            if name in parts:
                lam, vec = _kept_eigenpairs(parts[name][a], a, name)
                in_range(vec, a, name)
                for r in range(int(lam.shape[0])):
                    mine.append((1, 0.5 * float(lam[r]), vec[r], None) if name == "xx" else (1, 0.5 * float(lam[r]), None, vec[r]))
        if ex is not None:
            used = torch.nonzero(ew[a] != 0).reshape(-1)
            if used.numel():
                in_range(ea[a, used], a, "a of ex")
            mine += [(2, float(ew[a, e]), ea[a, e], None) for e in used]
        columns.append(mine)
    cols = 1 + max(len(mine) for mine in columns)
    vx, vp = torch.zeros((M, cols, D), dtype=torch.float64), torch.zeros((M, cols, D), dtype=torch.float64)
    kind, lam_out = torch.zeros((M, cols), dtype=torch.int32), torch.zeros((M, cols), dtype=torch.float64)
    lam_out[:, 0] = 1.0
    if "x" in parts:
        vx[:, 0] = parts["x"]
    if "p" in parts:
        vp[:, 0] = parts["p"]
    for a, mine in enumerate(columns):
        for k, (kd, lm, xv, pv) in enumerate(mine):
            kind[a, 1 + k], lam_out[a, 1 + k] = kd, lm
            if xv is not None:
                vx[a, 1 + k] = xv
            if pv is not None:
                vp[a, 1 + k] = pv
    kappa = torch.zeros(M, dtype=C128)
    if "c" in parts:
        kappa += parts["c"]
    return vx.contiguous(), vp.contiguous(), kind.contiguous(), lam_out.contiguous(), kappa.contiguous(), cols


def wm_operator_columns(vx, vp, kind, lam, Qi, dvecp_i, Qj, cqq_j, dvec_j, dvecp_j, U):
    """(za, zb, g, sfix, sket, ketcol, kind): the columns of ``fold_wm_operator_columns`` for bras i and kets j, as
    sc_wm_pair_expect_cols takes them.  The linear form of column col is
        l_col = za[col][i] + zb[col][j] + g_col . b' + s_col^T D'^-1 b',    s_col = sfix[col] (+ sket[ketcol[col]][j]),
    with the x-forms and p-forms of ``wm_expectation_columns``, the p-form now on any column: every column with a non-zero p-form
    vector w gets a slot p of  sket[p][j] = i hbar U^T C_j w  (the slots in the order of the columns).  zb of column 0 of operator a
    takes the per-ket constant  hbar^2 sum_col lam_col w_col^T C_j w_col  over a's kind-1 p-form columns (lam = mu / 2): the tr(W C_j)
    of the ket-side identity.  vx, vp (M, cols, D), kind, lam (M, cols) on the host; the trajectories' operands as in
    ``wm_expectation_columns``, on one device.  Returns za (C, ni), zb (C, nj), g, sfix (C, d') complex, C = M cols, sket (S, nj, d')
    complex or None (S = 0), ketcol, kind (C,) int32 on the device."""
    dev = Qi.device
    M, C1, D = vx.shape
    Uc = U.type(C128)
    v = vx.reshape(M * C1, D).to(dev)
    za = (v @ Qi.T).type(C128)
    zb = torch.zeros((M * C1, Qj.shape[0]), dtype=C128, device=dev)
    sfix = (v @ U).type(C128)
    g = torch.zeros_like(sfix)
    wflat = vp.reshape(M * C1, D)
    slots = torch.nonzero((wflat != 0).any(1)).reshape(-1)          # the columns with a p-form, on the host
    ketcol = torch.full((M * C1,), -1, dtype=torch.int32)
    ketcol[slots] = torch.arange(slots.numel(), dtype=torch.int32)
    sket = None
    if slots.numel():
        sd = slots.to(dev)
        w = wflat[slots].to(dev).type(C128)                 # (S, D)
        wpr = w @ Uc                                        # w' = U^T w
        za[sd] += 1j * hbar * (wpr @ dvecp_i.conj().T)
        zb[sd] += -1j * hbar * (w @ dvec_j.T) + 1j * hbar * (wpr @ dvecp_j.T)
        g[sd] += -1j * hbar * wpr
        Cw = torch.einsum('jab,sb->sja', cqq_j, w)          # (S, nj, D)
        sket = (1j * hbar * (Cw @ Uc)).contiguous()
        squared = kind.reshape(-1)[slots] == 1
        if bool(squared.any()):
            wCw = torch.einsum('sa,sja->sj', w, Cw)[squared.to(dev)]                        # w^T C_j w
            weight = (hbar ** 2 * lam.reshape(-1)[slots][squared]).to(dev).type(C128)
            owner = (torch.div(slots[squared], C1, rounding_mode='floor') * C1).to(dev)      # column 0 of the column's operator
            zb.index_add_(0, owner, weight.unsqueeze(1) * wCw)
    return (za.contiguous(), zb.contiguous(), g.contiguous(), sfix.contiguous(), sket, ketcol.to(dev),
            kind.reshape(-1).to(torch.int32).contiguous().to(dev))


def wm_operator_launches(lam, kind, cap):
    """The operator set of ``fold_wm_operator_columns`` cut into calls of sc_wm_pair_expect_cols that hold at most ``cap`` >= 2
    columns each: the cut of ``wm_expectation_launches``, whatever the kinds of the columns 1 ... (F is the sum of its columns).
    lam, kind (M, cols).  Returns (cols', calls), a call being (ops, owners, columns): ``owners`` the operators its pieces belong to
    (the caller adds the pieces of an operator), ``ops`` the operators whose kappa they carry -- M, an operator of kappa = 0, for a
    later piece --, ``columns`` the len(ops) cols' flat indices a cols + r of its columns, where M cols stands for a column of zeros
    with kind 0 and lam = 0: column 0 of a later piece and every padding (never a kind-2 column: 0 x inf; ValueError for a set that
    holds a kind-2 column with lam = 0 itself)."""
    M, C1 = lam.shape
    if bool(((kind == 2) & (lam == 0)).any()):
        raise ValueError("operators: a kind-2 column with lam = 0 (0 x exp may be 0 x inf: leave the term out)")
    Rl, cut = wm_expectation_launches(lam, cap)
    calls = []
    for pieces in cut:
        ops, owners, columns = [], [], []
        for a, first, sq in pieces:
            ops.append(a if first else M)
            owners.append(a)
            columns += [a * C1 if first else M * C1] + [a * C1 + r for r in sq] + [M * C1] * (Rl - len(sq))
        calls.append((ops, owners, columns))
    return 1 + Rl, calls


def fold_exponential_operators(w, a, Gamma_t):
    """(uq, up, mu): the matrix element of the operators  sum_e w_a,e exp(-a_a,e . x)  between two Gaussians |q_i, p_i, Gamma_t>,
    |q_j, p_j, Gamma_t> of ONE width, divided by their overlap, as P PRODUCT columns per operator.  With
    B = (2 Gamma_t)^+ and the pair mean xbar of ``fold_expectation_operators`` the element of one term is
        w exp(-a.xbar + 1/2 a^T B a) = mu exp(-alpha_i) conj(exp(-alpha_j)),    alpha_i = uq.q_i + up.p_i,
        uq = a / 2,   up = -i B a / hbar,   mu = w exp(1/2 a^T B a)       (real a: a.xbar = alpha_i + conj(alpha_j)).
    w (M, P) real or complex, a (M, P, D) real; returns complex (M, P, D) twice and complex (M, P).  A term with w = 0 is padding:
    its forms are zero, whatever its a.  ValueError for shapes that do not agree, M < 1, a non-finite entry, and an a with w != 0
    outside the range of Gamma_t (relative 1e-8, the test of ``fold_expectation_operators``), naming the operator and the term."""
    Gamma_t = as_f64(Gamma_t)
    D = Gamma_t.shape[0]
    try:
        w = torch.as_tensor(w)
        w = w.detach().cpu().to(C128) if w.is_complex() else as_f64(w).to(C128)
        a = as_f64(a)
    except (TypeError, ValueError, RuntimeError) as err:
        raise ValueError(f"operators: ex: a pair (w, a) of arrays, a real, is expected ({err})")
    if w.dim() != 2 or a.dim() != 3 or tuple(a.shape) != tuple(w.shape) + (D,) or w.shape[0] < 1:
        raise ValueError(f"operators: ex = (w, a) with w of shape (M, P), M >= 1, and a of shape (M, P, {D}) is expected, got "
                         f"{tuple(w.shape)} and {tuple(a.shape)}")
    if not bool(torch.isfinite(torch.view_as_real(w)).all()) or not bool(torch.isfinite(a).all()):
        raise ValueError("operators: non-finite entry in ex")
    e, V = _eigh(Gamma_t)
    keep = abs(e) > ZERO
    Vk = V[:, keep]
    B = torch.einsum('ij,j,kj->ik', Vk, 0.5 / e[keep], Vk)          # (2 Gamma_t)^+
    used = w != 0
    a = a * used.unsqueeze(2)
    outside = torch.linalg.norm(a - (a @ Vk) @ Vk.T, dim=2) > 1.0e-8 * torch.linalg.norm(a, dim=2)
    if bool(outside.any()):
        op, term = (int(t) for t in torch.nonzero(outside)[0])
        raise ValueError(f"operators: a of term {term} of operator {op} of ex has a component outside the range of Gamma_t: the "
                         "matrix element along a null direction does not exist")
    aB = a @ B                                                       # rows (B a)^T, B symmetric
    mu = w * torch.exp(0.5 * (aB * a).sum(2))
    if not bool(torch.isfinite(torch.view_as_real(mu)).all()):
        op, term = (int(t) for t in torch.nonzero(~torch.isfinite(torch.view_as_real(mu)).all(2))[0])
        raise ValueError(f"operators: term {term} of operator {op} of ex: w exp(a^T B a / 2) is not finite")
    uq = torch.complex(0.5 * a, torch.zeros_like(a))
    up = torch.complex(torch.zeros_like(a), -aB / hbar)
    return uq.contiguous(), up.contiguous(), mu.contiguous()


def time_grid(nt, dt):
    """t_k of the propagator: t accumulates `t += dt` (propagators.py:655), not k*dt"""
    t, out = 0.0, np.empty(nt)
    for k in range(nt):
        out[k] = t
        t += dt
    return out


class WMConstants(object):
    """constants of the Walton-Manolopoulos prefactor, reference propagators.py:1102-1130, 1227-1238, 1264, 1295

    Everything is expressed in the projected space of dimension e = 2 d' (see csrc/sc_wm.hip).
    """

    def __init__(self, Gamma_0, Gamma_i, Gamma_t, iGi0, U, alpha, beta):
        D, dp = U.shape
        Ur = U.real.contiguous() if U.is_complex() else U
        pdet = lambda G, s: torch.prod((lambda e: e[abs(e) > ZERO] / s)(_eigh(G)[0]))
        detG0, detGi, detGt = pdet(Gamma_0, np.pi), pdet(Gamma_i, np.pi), pdet(Gamma_t, np.pi)
        detGi0 = pdet(Gamma_0 + Gamma_i, 2 * np.pi)
        self.pre = float(detG0 ** 0.5 * detGt ** 0.25 * detGi ** 0.25 / torch.sqrt(detGi0))     # :1598-1599
        self.pre_coef = float(detG0 ** 0.25 * detGt ** 0.25 * detGi ** 0.25 / torch.sqrt(detGi0))    # :1408-1409
        e0, V0 = _eigh(Gamma_0)
        keep = e0 > ZERO
        iGamma_0 = torch.einsum('ij,j,kj->ik', V0[:, keep], 1.0 / e0[keep], V0[:, keep])      # :1130
        self.dim, self.dprime = D, dp
        self.U = Ur.contiguous()
        self.Gt, self.G0, self.iGi0 = Gamma_t.contiguous(), Gamma_0.contiguous(), iGi0.contiguous()
        self.S = (iGi0 @ Gamma_0).contiguous()
        self.Cqq = (Gamma_0 - Gamma_0 @ iGi0 @ Gamma_0).contiguous()                          # (69)
        E = 2 * dp
        Cst = torch.zeros((E, E), dtype=C128)
        Cst[:dp, :dp] = 2 * alpha * (Ur.T @ Gamma_0 @ Ur) + Ur.T @ Gamma_i @ Ur
        Cst[dp:, dp:] = 2 * beta * (Ur.T @ iGamma_0 @ Ur)
        Cst[dp:, :dp] += -2j / hbar * (Ur.T @ Ur)
        self.Cst = Cst.contiguous()
        Bq = torch.zeros((D, E), dtype=C128)
        Bq[:, :dp] = Gamma_i @ Ur
        Bq[:, dp:] = -1j / hbar * Ur
        self.Bq = Bq.contiguous()
        self.inv_scale_a = 1.0 / (2.0 * math.sqrt(alpha * beta))
        self.inv_two_pi = 1.0 / (2.0 * np.pi)


def rotate_second_moments(m3, theta):
    """second moments (S_rr, S_ii, S_ri) of complex terms c_i -> those of c_i e^{i theta} (rows of m3 (..., 3), theta (...,)).
    Exact for a phase shared by every term: the 2 x 2 matrix [[S_rr, S_ri], [S_ri, S_ii]] is conjugated by the rotation."""
    m3 = np.asarray(m3, dtype=np.float64)
    c, s = np.cos(theta), np.sin(theta)
    rr, ii, ri = m3[..., 0], m3[..., 1], m3[..., 2]
    return np.stack((c * c * rr - 2.0 * c * s * ri + s * s * ii,
                     s * s * rr + 2.0 * c * s * ri + c * c * ii,
                     c * s * (rr - ii) + (c * c - s * s) * ri), axis=-1)


def standard_errors(mean, m3, ntraj):
    """sigma_Re + i sigma_Im of a Monte-Carlo mean = sum_i c_i with weights 1/N inside c_i, from the sums m3 = (S_rr, S_ii, S_ri)
    of the same terms:  sigma_Re = sqrt(max(N S_rr - (Re mean)^2, 0) / (N - 1)), sigma_Im likewise; NaN for N = 1"""
    mean = np.asarray(mean, dtype=np.complex128)
    m3 = np.asarray(m3, dtype=np.float64)
    n = float(ntraj)
    with np.errstate(invalid="ignore", divide="ignore"):
        den = (n - 1.0) if n > 1 else np.nan
        sr = np.sqrt(np.maximum(n * m3[..., 0] - mean.real ** 2, 0.0) / den)
        si = np.sqrt(np.maximum(n * m3[..., 1] - mean.imag ** 2, 0.0) / den)
    return sr + 1j * si


# ---- batch means: error bars of anything linear in C_auto(t) or k_ic(t) ----

def valid_error_blocks(B):
    """B blocks: a power of two in 2 ... 64 (sc_error_blocks_valid, csrc/sc_common.h)"""
    return isinstance(B, (int, np.integer)) and 2 <= B <= 64 and (B & (B - 1)) == 0


def error_block(i, B):
    """The partition of a batch into B blocks, the host's copy of sc_error_block (csrc/sc_common.h): block of the trajectory with
    rank-local index ``i`` (an integer or an integer array).  Groups of four consecutive trajectories are dealt round robin to
    the blocks.  The trajectories are independent draws, so any fixed partition is valid; this one is what the whole-loop kernels
    already keep apart: their wavefront slot holds the trajectories with (i >> 2) mod slots == slot, and the slot count either
    does not wrap or is a multiple of B, so block = slot mod B."""
    return (np.asarray(i, dtype=np.int64) >> 2) & (B - 1)


def block_counts(n, B):
    """n_b: how many of the trajectories 0 ... n - 1 fall into each of the B blocks of ``error_block``; follows from n alone"""
    if not valid_error_blocks(B):
        raise ValueError(f"the number of blocks has to be a power of two in 2 ... 64, got {B}")
    groups, rest = divmod(int(n), 4)
    counts = np.full(B, 4 * (groups // B), dtype=np.int64)
    counts[:groups % B] += 4
    counts[groups % B] += rest
    return counts


def block_standard_error(values, counts):
    """Standard error of a pooled estimate from its values on B blocks (batch means).

    ``values`` (B, ...): a functional LINEAR in the correlation functions evaluated on each block's own estimate (the block's
    sum times N / n_b); ``counts`` (B,): the trajectories n_b of the blocks.  With N = sum n_b and the pooled value
    F = sum_b n_b F_b / N the result is sqrt(sum_b n_b (F_b - F)^2 / ((B' - 1) N)) over the B' non-empty blocks -- the ANOVA form,
    exact for unequal n_b; with one sample per block it is the per-sample standard error.  Blocks with n_b = 0 are dropped; fewer
    than two non-empty blocks give NaN.  Complex values: sigma_Re + i sigma_Im, as ``standard_errors``."""
    values = np.asarray(values)
    counts = np.asarray(counts, dtype=np.float64)
    assert values.shape[0] == counts.shape[0], "one value per block"
    keep = counts > 0
    values, counts = values[keep], counts[keep]
    nb = counts.shape[0]
    if nb < 2:
        return np.full(values.shape[1:], np.nan + (1j * np.nan if np.iscomplexobj(values) else 0.0))
    total = counts.sum()
    w = counts.reshape((nb,) + (1,) * (values.ndim - 1))
    pooled = (w * values).sum(axis=0) / total
    dev = values - pooled
    if np.iscomplexobj(values):
        return (np.sqrt((w * dev.real ** 2).sum(axis=0) / ((nb - 1) * total))
                + 1j * np.sqrt((w * dev.imag ** 2).sum(axis=0) / ((nb - 1) * total)))
    return np.sqrt((w * dev ** 2).sum(axis=0) / ((nb - 1) * total))
