"""Expectation values of quadratic operators in the HK wavepacket: a numpy restatement of the closed form
from the pair means, with no eigendecomposition -- the reference of tests/test_expect_host.py and tests/test_expect_gpu.py -- and the
evaluation of the folded columns on the host."""
import numpy as np

from tests.test_density_host import HBAR, ZERO, overlap_constants, pair_exponents


def zeros_for(M, D, c=None, m=None, K=None, n=None, W=None):
    """the five parts as arrays, None -> zeros"""
    return (np.zeros(M) if c is None else np.asarray(c, dtype=float), np.zeros((M, D)) if m is None else np.asarray(m, dtype=float),
            np.zeros((M, D, D)) if K is None else np.asarray(K, dtype=float), np.zeros((M, D)) if n is None else np.asarray(n, dtype=float),
            np.zeros((M, D, D)) if W is None else np.asarray(W, dtype=float))


def pair_terms(q, p, v, G, bra=None):
    """T_ij = v_i^* O_ij v_j (ni, nj) and the pair means xbar, pbar (D, ni, nj); q, p (D, n), v (n,); ``bra`` = (q, p, v) of another
    set of bras (default: the kets)"""
    qi, pi, vi = (q, p, v) if bra is None else bra
    ni = qi.shape[1]
    qq, pp = np.concatenate((qi, q), 1), np.concatenate((pi, p), 1)
    E, fac = pair_exponents(qq, pp, G)
    T = fac * np.conj(vi)[:, None] * v[None, :] * np.exp(E[:ni, ni:])
    _, B, _, _ = overlap_constants(G)
    dp = p[:, None, :] - pi[:, :, None]                 # (D, i, j): p_j - p_i
    dq = qi[:, :, None] - q[:, None, :]                 # q_i - q_j
    xbar = 0.5 * (qi[:, :, None] + q[:, None, :]) + 1j / HBAR * np.einsum('ab,bij->aij', B, dp)
    pbar = 0.5 * (pi[:, :, None] + p[:, None, :]) + 0.5j * HBAR * np.einsum('ab,bij->aij', G, dq)
    return T, xbar, pbar


def pair_factors(q, p, G, c, m, K, n, W, bra=None):
    """F_a,ij (M, ni, nj) of the direct formula:
    c + m.xbar + 1/2 xbar^T K xbar + 1/2 tr(K B) + n.pbar + 1/2 pbar^T W pbar + hbar^2 / 4 tr(W G)"""
    _, xbar, pbar = pair_terms(q, p, np.ones(q.shape[1]), G, bra=None if bra is None else (bra[0], bra[1], np.ones(bra[0].shape[1])))
    _, B, _, _ = overlap_constants(G)
    F = (c[:, None, None] + np.einsum('ma,aij->mij', m, xbar) + 0.5 * np.einsum('aij,mab,bij->mij', xbar, K, xbar, optimize=True)
         + np.einsum('ma,aij->mij', n, pbar) + 0.5 * np.einsum('aij,mab,bij->mij', pbar, W, pbar, optimize=True))
    return F + (0.5 * np.einsum('mab,ba->m', K, B) + 0.25 * HBAR ** 2 * np.einsum('mab,ba->m', W, G))[:, None, None]


def restated_expectation(q, p, v, G, c=None, m=None, K=None, n=None, W=None, M=None, bra=None):
    """(E, A, N2): E_a = sum_ij T_ij F_a,ij, A_a = sum_ij |T_ij F_a,ij| (M,), N2 = sum_ij T_ij (complex)"""
    D = q.shape[0]
    if M is None:
        M = next(len(t) for t in (c, m, K, n, W) if t is not None)
    c, m, K, n, W = zeros_for(M, D, c, m, K, n, W)
    T, _, _ = pair_terms(q, p, v, G, bra=bra)
    terms = T[None, :, :] * pair_factors(q, p, G, c, m, K, n, W, bra=bra)
    return terms.sum(axis=(1, 2)), abs(terms).sum(axis=(1, 2)), T.sum()


def folded_factors(q, p, fold, bra=None):
    """F_a,ij (M, ni, nj) from the columns of hostmath.fold_expectation_operators: kappa_a + sum_col lam z^p, z = a_i + conj(a_j)"""
    uq, up, lam, kappa, R = (np.asarray(t) for t in fold)
    qi, pi = (q, p) if bra is None else bra[:2]
    a_bra = np.einsum('mcd,di->mci', uq, qi) + np.einsum('mcd,di->mci', up, pi)
    a_ket = np.einsum('mcd,dj->mcj', uq, q) + np.einsum('mcd,dj->mcj', up, p)
    z = a_bra[:, :, :, None] + np.conj(a_ket)[:, :, None, :]
    power = np.where(np.arange(1 + int(R)) == 0, 1, 2)[None, :, None, None]
    return kappa[:, None, None] + np.einsum('mc,mcij->mij', lam, z ** power)


def projector(G):
    """onto the range of G"""
    e, V = np.linalg.eigh(G)
    V = V[:, abs(e) > ZERO]
    return V @ V.T


def symmetric(rng, D, rank=None, P=None):
    """a random real symmetric (D, D) matrix of the given rank (default D), indefinite, inside the range projected by P"""
    rank = D if rank is None else rank
    Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    lam = rng.uniform(0.3, 1.5, rank) * np.where(np.arange(rank) % 2 == 0, 1.0, -1.0)
    S = (Q[:, :rank] * lam) @ Q[:, :rank].T
    if P is not None:
        S = P @ S @ P
    return 0.5 * (S + S.T)


def standard_operators(rng, G):
    """the six operators of the engine tests: x and p along one random direction u projected onto the range of G, their squares,
    one mixed operator with all five parts, and the constant 1 -> (c, m, K, n, W), each with M = 6.  The x parts of the mixed
    operator are in units of the mean position width of one Gaussian, its p parts in units of the mean momentum width, so that
    the five parts have the same order of magnitude whatever the units of the model."""
    D = G.shape[0]
    P = projector(G)
    _, B, _, _ = overlap_constants(G)
    rank = round(np.trace(P))
    scale_x, scale_p = 1.0 / np.sqrt(np.trace(B) / rank), 1.0 / np.sqrt(0.5 * HBAR ** 2 * np.trace(G) / rank)
    u = P @ (rng.uniform(0.5, 1.5, D) * rng.choice([-1.0, 1.0], D))
    u /= np.linalg.norm(u)
    c, m, K, n, W = zeros_for(6, D)
    m[0] = u
    K[1] = 2.0 * np.outer(u, u)
    n[2] = u
    W[3] = 2.0 * np.outer(u, u)
    c[4], m[4], n[4] = 0.3, scale_x * (P @ rng.standard_normal(D)), scale_p * (P @ rng.standard_normal(D))
    K[4], W[4] = scale_x ** 2 * symmetric(rng, D, P=P), scale_p ** 2 * symmetric(rng, D, P=P)
    c[5] = 1.0
    return c, m, K, n, W
