"""Numpy restatement of WaltonManolopoulosPropagator.wm_operator_expectation: the direct formula of
tests/wm_expect_cases.py extended by the quadratic momentum part -- the ket-side identity with W as given -- and by exponentials, with
np.linalg.inv, no fold and no eigendecomposition; and the same model evaluated from the columns of sc_wm_pair_expect_cols."""
import numpy as np

from tests import wm_expect_cases as WC

HBAR = WC.HBAR


def _parts(D, c, m, K, n, W, ex):
    given = [t for t in (c, m, K, n, W) if t is not None] + ([ex[0]] if ex is not None else [])
    M = len(given[0])
    z = lambda t, shape: np.zeros((M,) + shape) if t is None else np.asarray(t, dtype=float)
    w, a = (np.zeros((M, 0)), np.zeros((M, 0, D))) if ex is None else (np.asarray(ex[0], dtype=float), np.asarray(ex[1], dtype=float))
    return M, z(c, ()), z(m, (D,)), z(K, (D, D)), z(n, (D,)), z(W, (D, D)), w, a


def pair_terms(bra, ket, c=None, m=None, K=None, n=None, W=None, ex=None):
    """(T, terms): the terms of F_a,ij, a list of arrays (M, ni, nj) whose sum is F, of
        c + m.x + 1/2 x^T K x + n.p + 1/2 p^T W p + sum_e w_e exp(-a_e.x)      (p = -i hbar d/dx on the ket):
    with xbar = Q_i + U D'^-1 b', B = U D'^-1 U^T and L = d_j - C_j (xbar - Q_j)
        c;   m.xbar;   1/2 xbar^T K xbar + 1/2 tr(K B);   -i hbar n.L;
        -hbar^2 / 2 [ L^T W L + tr(W C_j B C_j) - tr(W C_j) ];   w_e exp(-a_e.xbar + 1/2 a_e^T B a_e)  for every e"""
    U = ket["U"]
    M, c, m, K, n, W, w, a = _parts(U.shape[0], c, m, K, n, W, ex)
    T, Dp, b = WC.pair_system(bra, ket)
    iD = np.linalg.inv(Dp)
    xbar = bra["Q"][:, None, :] + np.einsum('ak,ijkl,ijl->ija', U, iD, b, optimize=True)
    B = np.einsum('ak,ijkl,bl->ijab', U, iD, U, optimize=True)
    C = ket["cqq"]
    L = ket["dvec"][None, :, :] - np.einsum('jab,ijb->ija', C, xbar - ket["Q"][None, :, :])
    CBC = np.einsum('jab,ijbc,jcd->ijad', C, B, C, optimize=True)
    ones = np.ones(T.shape)
    terms = [c[:, None, None] * ones, np.einsum('ma,ija->mij', m, xbar),
             0.5 * np.einsum('ija,mab,ijb->mij', xbar, K, xbar, optimize=True) + 0.5 * np.einsum('mab,ijab->mij', K, B),
             -1j * HBAR * np.einsum('ma,ija->mij', n, L),
             -0.5 * HBAR ** 2 * (np.einsum('ija,mab,ijb->mij', L, W, L, optimize=True) + np.einsum('mab,ijba->mij', W, CBC)
                                 - np.einsum('mab,jba->mj', W, C)[:, None, :])]
    for e in range(w.shape[1]):
        ae = a[:, e]
        terms.append(w[:, e, None, None] * np.exp(-np.einsum('ma,ija->mij', ae, xbar)
                                                  + 0.5 * np.einsum('ma,ijab,mb->mij', ae, B, ae, optimize=True)))
    return T, terms


def restated_expectation(bra, ket, c=None, m=None, K=None, n=None, W=None, ex=None):
    """(E, A, N2): E_a = sum_ij T_ij F_a,ij,  A_a = sum_ij |T_ij| sum |terms of F_a,ij| -- the sum of the absolute terms, so that
    cancellation inside F (a Morse V) does not hide in a bound relative to it --,  N2 = sum_ij T_ij"""
    T, terms = pair_terms(bra, ket, c, m, K, n, W, ex)
    F = sum(terms)
    return (T[None] * F).sum(axis=(1, 2)), (abs(T)[None] * sum(abs(t) for t in terms)).sum(axis=(1, 2)), T.sum()


def column_terms(Dp, b, za, zb, g, sfix, sket, ketcol, kind, lam):
    """lam_col f_col (C, ni, nj) from the columns as sc_wm_pair_expect_cols reads them (include/semiclassical_hip.h): za (C, ni), zb
    (C, nj), g, sfix (C, d'), sket (S, nj, d') or None, ketcol, kind (C,), lam (C,)"""
    C = len(kind)
    ni, nj, dp = b.shape
    iD = np.linalg.inv(Dp)
    s = np.broadcast_to(sfix[:, None, :], (C, nj, dp)).astype(complex)                        # (C, nj, d')
    for col in np.nonzero(np.asarray(ketcol) >= 0)[0]:
        s[col] += sket[ketcol[col]]
    st = s.transpose(1, 2, 0)                                                                 # (nj, d', C)
    sDb = np.einsum('jkc,ijkl,ijl->cij', st, iD, b, optimize=True)
    sDs = np.einsum('jkc,ijkc->cij', st, np.einsum('ijkl,jlc->ijkc', iD, st, optimize=True))
    l = za[:, :, None] + zb[:, None, :] + np.einsum('ck,ijk->cij', g, b) + sDb
    kd = np.asarray(kind)[:, None, None]
    with np.errstate(over="ignore", invalid="ignore"):
        f = np.where(kd == 0, l, np.where(kd == 1, l * l + sDs, np.exp(np.where(kd == 2, -l + 0.5 * sDs, 0.0))))
    return np.asarray(lam).reshape(-1)[:, None, None] * f


def column_elements(Dp, b, za, zb, g, sfix, sket, ketcol, kind, lam, kap):
    """(F, Fabs): F_a,ij = kap_a + sum of the operator's columns (M, ni, nj), lam (M, cols), and |kap_a| + sum |lam_col f_col|"""
    M, cols = lam.shape
    t = column_terms(Dp, b, za, zb, g, sfix, sket, ketcol, kind, lam).reshape(M, cols, *b.shape[:2])
    return kap[:, None, None] + t.sum(1), abs(kap)[:, None, None] + abs(t).sum(1)


def morse_operator(depth, rate, masses=None, harmonic=None):
    """(c, K, W, ex) of  p^T m^-1 p / 2 + sum_k depth_k (1 - exp(-rate_k x_k))^2 + 1/2 x^T diag(harmonic) x  as ONE operator:
    depth_k - 2 depth_k exp(-rate_k x_k) + depth_k exp(-2 rate_k x_k)"""
    depth, rate = np.asarray(depth, dtype=float), np.asarray(rate, dtype=float)
    D = len(depth)
    masses = np.ones(D) if masses is None else np.asarray(masses, dtype=float)
    K = None if harmonic is None else np.diag(np.asarray(harmonic, dtype=float))[None]
    w = np.concatenate((-2.0 * depth, depth))[None]
    a = np.concatenate((np.diag(rate), np.diag(2.0 * rate)))[None]
    return np.array([depth.sum()]), K, np.diag(1.0 / masses)[None], (w, a)
