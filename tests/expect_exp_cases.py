"""Expectation values of operators with exp(-a.x) terms in the HK wavepacket: the numpy restatement of
tests/expect_cases.py with  sum_e w_e exp(-a_e.xbar_ij + 1/2 a_e^T B a_e)  added to the direct formula, the sum of ABSOLUTE terms
that the bounds of tests/test_expect_exp_host.py and tests/test_expect_exp_gpu.py refer to, the evaluation of the folded product
columns on the host, the Morse surfaces of the goldens as such operators, and the operator set of the engine tests."""
import numpy as np

from tests import expect_cases as EC
from tests.test_density_host import HBAR, overlap_constants


def exponential_sums(q, p, G, w, a, bra=None):
    """(S, |S|): sum_e t_e and sum_e |t_e| of the terms t_e = w_a,e exp(-a_a,e . xbar_ij + 1/2 a^T B a), (M, ni, nj) each;
    w (M, P), a (M, P, D) real.  Terms with w = 0 are skipped (operator by operator: the term array of H at D = 60 is large)."""
    ones = lambda t: np.ones(t.shape[1])
    _, xbar, _ = EC.pair_terms(q, p, ones(q), G, bra=None if bra is None else (bra[0], bra[1], ones(bra[0])))
    _, B, _, _ = overlap_constants(G)
    w, a = np.asarray(w), np.asarray(a, dtype=float)
    total, size = np.zeros((len(w),) + xbar.shape[1:], dtype=complex), np.zeros((len(w),) + xbar.shape[1:])
    for op in range(len(w)):
        used = np.nonzero(w[op])[0]
        if len(used):
            av = a[op, used]
            t = w[op, used, None, None] * np.exp(-np.einsum('ed,dij->eij', av, xbar) + 0.5 * np.einsum('ed,df,ef->e', av, B, av)[:, None, None])
            total[op], size[op] = t.sum(axis=0), abs(t).sum(axis=0)
    return total, size


def restated_expectation(q, p, v, G, c=None, m=None, K=None, n=None, W=None, w=None, a=None, bra=None):
    """(E, At, N2): E_a = sum_ij T_ij F_a,ij with F the direct formula of expect_cases.pair_factors plus the exponential terms,
    At_a = sum_ij |T_ij| (|c + traces| + sum |each linear, quadratic and exponential term|), the sum of absolute terms (M,), and
    N2 = sum_ij T_ij (complex).  Any part may be None (= zeros); M from the ones given."""
    D = q.shape[0]
    M = next(len(t) for t in (c, m, K, n, W, w) if t is not None)
    c, m, K, n, W = EC.zeros_for(M, D, c, m, K, n, W)
    w, a = (np.zeros((M, 0)), np.zeros((M, 0, D))) if w is None else (np.asarray(w), np.asarray(a, dtype=float))
    T, xbar, pbar = EC.pair_terms(q, p, v, G, bra=bra)
    _, B, _, _ = overlap_constants(G)
    ex, ex_size = exponential_sums(q, p, G, w, a, bra=bra)
    F = EC.pair_factors(q, p, G, c, m, K, n, W, bra=bra) + ex
    const = c + 0.5 * np.einsum('mab,ba->m', K, B) + 0.25 * HBAR ** 2 * np.einsum('mab,ba->m', W, G)
    size = (abs(const)[:, None, None] + abs(np.einsum('ma,aij->mij', m, xbar)) + abs(np.einsum('ma,aij->mij', n, pbar))
            + abs(0.5 * np.einsum('aij,mab,bij->mij', xbar, K, xbar, optimize=True))
            + abs(0.5 * np.einsum('aij,mab,bij->mij', pbar, W, pbar, optimize=True)) + ex_size)
    return (T[None] * F).sum(axis=(1, 2)), (abs(T)[None] * size).sum(axis=(1, 2)), T.sum()


def folded_exponential_factors(q, p, fold, bra=None):
    """sum_e ea_i eb_j (M, ni, nj) from hostmath.fold_exponential_operators: ea_i = mu exp(-alpha_i), eb_j = conj(exp(-alpha_j)),
    alpha_i = uq.q_i + up.p_i -- the product columns as the engine forms them"""
    uq, up, mu = (np.asarray(t) for t in fold)
    qi, pi = (q, p) if bra is None else bra[:2]
    alpha = lambda qq, pp: np.einsum('med,di->mei', uq, qq) + np.einsum('med,di->mei', up, pp)
    ea, eb = mu[:, :, None] * np.exp(-alpha(qi, pi)), np.conj(np.exp(-alpha(q, p)))
    return np.einsum('mei,mej->mij', ea, eb)


def morse_surface(g):
    """the potential of a golden as (const, w (P,), a (P, D), K (D, D)): V = const + sum_e w_e exp(-a_e.x) + 1/2 x^T K x.
    'morse': D_k (1 - exp(-a_k x_k))^2 with a = sqrt(2 omega chi), D = omega / (4 chi) and the engine's fix-up chi = 0 -> 1e-4 where
    not all chi are zero; 'nonharmonic': eps / (2 b^2) (1 - exp(-b x))^2 + (1 - eps) x^2 / 2."""
    kind = str(g["potential"])
    if kind == "morse":
        omega, chi = np.asarray(g["omega"], dtype=float), np.array(g["chi"], dtype=float)
        assert chi.any()
        chi[chi == 0.0] += 1.0e-4
        rate, depth = np.sqrt(2.0 * omega * chi), 0.25 * omega / chi
        K = np.zeros((len(rate), len(rate)))
    elif kind == "nonharmonic":
        eps, rate = np.asarray(g["eps"], dtype=float), np.asarray(g["b"], dtype=float)
        depth, K = 0.5 * eps / rate ** 2, np.diag(1.0 - eps)
    else:
        raise ValueError(kind)
    return depth.sum(), np.concatenate((-2.0 * depth, depth)), np.concatenate((np.diag(rate), np.diag(2.0 * rate))), K


def standard_operators(rng, G, g):
    """the five operators of the engine tests -> dict(c, m, K, n, W, w, a), each with M = 5 (P = 2 D + 1 exponential terms, unused
    ones with w = 0):
      0  exp(-a.x) along one random direction projected onto the range of G, |a| one inverse position width of a Gaussian,
      1  the Morse V of the golden g,
      2  the full H = p^2 / 2 + V (unit masses),
      3  one operator with all six parts, the five of expect_cases.standard_operators plus two exponentials of weights 0.7, -0.4,
      4  the constant 1."""
    D = G.shape[0]
    Pr = EC.projector(G)
    _, B, _, _ = overlap_constants(G)
    inv_width = 1.0 / np.sqrt(np.trace(B) / round(np.trace(Pr)))
    c5, m5, K5, n5, W5 = EC.standard_operators(rng, G)
    direction = lambda: (lambda u: inv_width * u / np.linalg.norm(u))(Pr @ (rng.uniform(0.5, 1.5, D) * rng.choice([-1.0, 1.0], D)))
    const, wv, av, Kv = morse_surface(g)
    P = 2 * D + 1
    c, m, K, n, W = EC.zeros_for(5, D)
    w, a = np.zeros((5, P)), np.zeros((5, P, D))
    w[0, 0], a[0, 0] = 1.0, direction()
    for op in (1, 2):
        c[op], K[op], w[op, :2 * D], a[op, :2 * D] = const, Kv, wv, av
    W[2] = np.eye(D)
    c[3], m[3], K[3], n[3], W[3] = c5[4], m5[4], K5[4], n5[4], W5[4]
    w[3, :2], a[3, 0], a[3, 1] = (0.7, -0.4), direction(), 0.5 * direction()
    c[4] = 1.0
    return dict(c=c, m=m, K=K, n=n, W=W, w=w, a=a)


LABELS = ("exp(-a.x)", "V", "H", "mixed", "1")
