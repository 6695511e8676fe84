"""Shared pieces of the direct tests of the Walton-Manolopoulos prefactor (test_wm_inverse_host.py, test_wm_inverse_gpu.py): the
per-trajectory WM terms of one trajectory restated in numpy.clongdouble, seeded inputs in three families of monodromy blocks, the
fp64 oracle's values of the same terms, and the error bound of the determinant tests (tests/det_cases.py).

The reference (wm_terms with the extended types) follows WMOracle._prefactor, autocorrelation_qp and the per-trajectory term of
ic_correlation (oracle/sc_oracle.py) formula by formula -- not the kernels' re-association -- with both inverses taken by a hand
written Gauss-Jordan elimination with partial pivoting over the whole column and both determinants by det_cases.det_longdouble.
What the host hands to the kernels as constants is an input here too, in the fp64 values the oracle computes: the width matrices,
the eigenvector basis U of Gamma_0 + Gamma_i, the pseudo-inverses (Gamma_0 + Gamma_i)^+, Gamma_0^+, the pseudo-determinants
behind the normalisation, pi and hbar.  The reference is exact arithmetic on those numbers; the kernels' part -- two inversions,
two determinants and the contractions between and behind them -- is what the comparison measures.

The same function with complex128 and a plain Gauss-Jordan whose pivot search is limited to a window of rows is the host model
of a defective kernel: the far-pivot family has to push it beyond the bound, and the full search has to keep it."""
import functools
import zlib

import numpy as np

from tests.det_cases import CLD, LD, det_longdouble

HBAR = 1.0

# (D, d'): the smallest shapes at which something changes in sc_wm_correlate
#   (8, 8), (12, 6)      register kernel; (12, 6) far-pivot / momentum-heavy also its flagged re-run in the LDS kernel
#   (16, 16)             LDS kernel with 64 threads, augmented width w2 = 4 d' = 64 = threads
#   (20, 20)             LDS kernel, 256 threads
#   (32, 32)             global scratch, E = 2 d' = 64: the last order one pivot candidate per lane covers
#   (33, 33), (40, 33)   E = 66; (40, 33): rank-deficient, dense rotated widths
#   (64, 64)             w2 = 256: the last width one column per thread covers
#   (65, 65), (70, 66)   w2 = 260, 264; (70, 66): M' (order d') is beyond 64 rows as well
#   (96, 96)
#   (129, 129)           first inversion w2 = 516 (left half beyond 256 columns), second inversion w2 = 258
SHAPES = ((8, 8), (12, 6), (16, 16), (20, 20), (32, 32), (33, 33), (40, 33), (64, 64), (65, 65), (70, 66), (96, 96), (129, 129))
FAMILIES = ("natural", "momentum-heavy", "far-pivot")
WINDOW = 64                       # rows below the diagonal the pivot search of lds_gauss_jordan used to look at
FAR_FACTOR = 2.0 ** 20            # far-pivot: the entry 64 or more rows below the diagonal over the entries within 64 rows
NEAR_FACTOR = 2.0 ** 16           # the same construction at d' <= 64, where no well-conditioned far pivot exists
ERR64_CAP = 1e-9                  # conditioning cap: the fp64 oracle's own error on every trajectory used
QUANTITIES = ("detA", "detM", "CQQ", "dvec", "cq", "kq")
# Seeds.  The bound of a trajectory is 16 x the oracle's own error on it, and for a single complex number that error now and then lands
# far below its typical size (the oracle right by accident), which says nothing about a kernel.  The seed of a case is the first one
# for which every trajectory's bound is at least twice the oracle's largest error of the case for every quantity -- a property of
# oracle and reference alone.  The oracle's rounding depends on the CPU its LAPACK runs on (which of a case's numbers come out luckily
# is not the same on every processor); the seeds below meet the criterion on both kinds of CPU the suite has been run on.  Every
# trajectory of every case is compared; nothing is filtered at run time.
SEED = {
    (8, 8, "momentum-heavy"): 18,
    (16, 16, "momentum-heavy"): 16,
    (20, 20, "momentum-heavy"): 10,
    (32, 32, "momentum-heavy"): 29,
    (33, 33, "momentum-heavy"): 12,
    (40, 33, "momentum-heavy"): 15,
    (64, 64, "momentum-heavy"): 27,
    (65, 65, "momentum-heavy"): 23,
    (70, 66, "momentum-heavy"): 12,
    (96, 96, "momentum-heavy"): 2,
    (129, 129, "momentum-heavy"): 13,
    (8, 8, "far-pivot"): 2,
    (16, 16, "far-pivot"): 6,
    (20, 20, "far-pivot"): 6,
    (32, 32, "far-pivot"): 8,
    (33, 33, "far-pivot"): 12,
    (64, 64, "far-pivot"): 1,
    (65, 65, "far-pivot"): 6,
    (70, 66, "far-pivot"): 1,
    (96, 96, "far-pivot"): 5,
    (129, 129, "far-pivot"): 2,
}


NTRAJ = 4                         # trajectories per case


def order(quantity, dp):
    """order of the matrix behind a quantity: E = 2 d' (first inversion), d' for detM"""
    return dp if quantity == "detM" else 2 * dp


# ------------------------------------------------------------------------------------------------------------- eliminations
def gauss_jordan(A, window=None):
    """inverse of one square complex matrix by Gauss-Jordan elimination of [A | I] with partial pivoting, in the type of A
    (complex128 or clongdouble), one rank-1 update per column; `window`: the pivot search looks at that many rows from the
    diagonal down (None: the whole column).  Returns (inverse, determinant)."""
    A = np.array(A)
    n = A.shape[0]
    aug = np.concatenate((A, np.eye(n, dtype=A.dtype)), axis=1)
    det = A.dtype.type(1.0)
    for k in range(n):
        hi = n if window is None else min(n, k + window)
        col = aug[k:hi, k]
        p = k + int(np.argmax(col.real * col.real + col.imag * col.imag))
        if p != k:
            aug[[k, p]] = aug[[p, k]]
            det = -det
        piv = aug[k, k]
        det = det * piv
        if piv == 0:
            return np.full((n, n), np.nan, dtype=A.dtype), A.dtype.type(0.0)
        aug[k] = aug[k] / piv
        colk = aug[:, k].copy()
        colk[k] = 0
        aug -= np.outer(colk, aug[k])
    return aug[:, n:], det


def inverse_longdouble(A):
    return gauss_jordan(np.asarray(A, dtype=CLD))[0]


# ------------------------------------------------------------------------------------------------------------------- inputs
def _rng(*key):
    return np.random.default_rng([zlib.crc32(str(k).encode()) for k in key])


def _mm(*mats):
    """matrix product without BLAS (numpy's own einsum loops): the same bits whatever the thread count of the host"""
    out = mats[0]
    for m in mats[1:]:
        out = np.einsum('ij,jk->ik', out, m)
    return out


def _expm(X):
    """exp(X) of a matrix of small norm: scaling by 2^-6, Taylor series, squaring"""
    Y = X / 64.0
    term, out = np.eye(X.shape[0]), np.eye(X.shape[0])
    for k in range(1, 16):
        term = _mm(term, Y) / k
        out = out + term
    for _ in range(6):
        out = _mm(out, out)
    return out


class Case(object):
    """inputs of one (shape, family): n trajectories; arrays are numpy float64, the trajectory index comes first"""


def _blocks_natural(rng, D, n):
    """M = exp(J S), S symmetric of spectral norm about 0.6 (a symmetric Gaussian matrix of order N has norm sqrt(2 N)):
    symplectic, a few steps of a coupled potential"""
    out = np.empty((n, 4, D, D))
    J = np.block([[np.zeros((D, D)), np.eye(D)], [-np.eye(D), np.zeros((D, D))]])
    for t in range(n):
        S = rng.standard_normal((2 * D, 2 * D))
        S = 0.5 * (S + S.T)
        S *= 0.6 / np.sqrt(4.0 * D)
        M = _expm(_mm(J, S))
        out[t] = M[:D, :D], M[:D, D:], M[D:, :D], M[D:, D:]
    return out


def momentum_heavy_parameters(D):
    """(momentum scale, noise amplitude, alpha = beta).  Up to D = 40 the construction of
    test_wm_weak_fixed_order_pivots_are_rerun_with_pivoting as it stands: 30, 0.5, 0.05.  |det(A'/s)| then grows like 10^(4.5 D)
    and leaves the range of fp64 before D = 65 -- in the oracle as in the kernels, which both form it as a plain product.  The
    larger shapes therefore keep the noise at the spectral norm it has at D = 32 and take a momentum scale and a cell width with
    which |det| stays representable at D = 129 (about 10^(1.7 D)); the imaginary part of the Filinov matrix is still several
    times its real part."""
    return (30.0, 0.5, 0.05) if D <= 40 else (3.0, 0.5 * np.sqrt(32.0 / D), 1.0)


def _blocks_momentum_heavy(rng, D, n):
    """I + a N(0, 1) in all four blocks, Mpq and Mpp times the momentum scale"""
    scale, amp, _ = momentum_heavy_parameters(D)
    out = np.empty((n, 4, D, D))
    for k, s in enumerate((1.0, 1.0, scale, scale)):
        out[:, k] = s * ((np.eye(D) if k in (0, 3) else 0.0) + amp * rng.standard_normal((n, D, D)))
    return out


def far_pivot_pairs(dp):
    """The index pairings of the far-pivot family in the projected space (d' indices): K = [(k, m)], P = [(m, j)].
    d' >= 65: K pairs k with k + 64 (as many k < 4 as there are; from d' = 129 column 0 with row 128 instead), P is empty: the kick
    puts i c at (k + 64, k) of the upper left block of A'.  d' <= 64: K pairs k with m_k, P pairs m_k with j_k; the product of drift and kick then puts i c at row d' + j_k
    of column k, with j_k = k + 64 - d' (64 rows below the diagonal) where 2 d' > 64 + k, and half the block further down where no
    row is that far (E <= 64: a strongly permuting case, nothing more)."""
    if dp > WINDOW:
        pairs = [(k, k + WINDOW) for k in range(4) if k + WINDOW < dp]
        if dp > 2 * WINDOW:            # column 0 with row 128: beyond two candidates per lane, the loop of the pivot search
            pairs[0] = (0, 2 * WINDOW)
        return pairs, []
    ks = [k for k in range(4) if 0 <= k + WINDOW - dp < dp] if 2 * dp > WINDOW else list(range(min(2, dp // 3)))
    js = [k + WINDOW - dp if 2 * dp > WINDOW else (k + dp // 2) % dp for k in ks]
    free = [i for i in range(dp) if i not in ks and i not in js]
    ms = free[len(free) // 2:][:len(ks)]
    return list(zip(ks, ms)), list(zip(ms, js))


def far_factor(dp):
    return FAR_FACTOR if dp > WINDOW else NEAR_FACTOR


def far_pivot_entries(dp):
    """(row, column) of A'/s (order 2 d') at which the family puts its dominant entries of columns k"""
    K, P = far_pivot_pairs(dp)
    if not P:
        return [(m, k) for k, m in K]
    j_of = dict(P)
    return [(dp + j_of[m], k) for k, m in K]


def _blocks_far_pivot(rng, case, n):
    """A free drift followed by a strong kick, M = [[1, 0], [c K, 1]] [[1, B], [0, 1]]: Mqq = 1, Mqp = B, Mpq = c K, Mpp = 1 + c K B
    with symmetric K (0/1 pairing) and B = P + small dense symmetric noise, all inside the non-zero subspace (U . U^T).  It is
    symplectic, so the Filinov matrix stays that of a physical trajectory (complex symmetric, C_QQ and M' of moderate size).
    With G = Mp'^T Mq' = [[c K, c K B], [1 + c B K, B + c B K B]] the imaginary part of A' holds c K in its upper left and
    2 G_ll - G_tr^T - 2 = c B K in its lower left block: isolated entries c (far_pivot_entries) in columns whose other entries
    are of order 1, in rows that carry an entry c of their own in another column.  The real part of the upper left block is
    2 alpha G0' + Gi' + Gt' (diagonal in the basis U the three widths share); c = far_factor(d') times its largest diagonal entry in
    the columns k, times 1 ... 1.25 per trajectory."""
    D, dp, U = case.D, case.dp, case.U
    K, P = far_pivot_pairs(dp)
    diag = np.diag(_mm(U.T, 2.0 * case.alpha * case.G0 + case.Gi + case.Gt, U))
    dmax = max(diag[k] for k, _ in K)
    Km, Pm = np.zeros((dp, dp)), np.zeros((dp, dp))
    for a, b in K:
        Km[a, b] = Km[b, a] = 1.0
    for a, b in P:
        Pm[a, b] = Pm[b, a] = 1.0
    out = np.zeros((n, 4, D, D))
    for t in range(n):
        c = far_factor(dp) * dmax * rng.uniform(1.0, 1.25)
        B = rng.standard_normal((dp, dp))
        B = 0.25 * (B + B.T) / np.sqrt(dp)
        B[Pm > 0] = 0.0
        B = Pm + B
        out[t, 0] = np.eye(D)
        out[t, 1] = _mm(U, B, U.T)
        out[t, 2] = c * _mm(U, Km, U.T)
        out[t, 3] = np.eye(D) + c * _mm(U, Km, B, U.T)
    return out


def _widths(rng, D, dp):
    """Gamma_i, Gamma_t, Gamma_0: a shared dense rotation (three Householder reflections), eigenvalues 0.5 ... 2 of their own
    each, the same D - d' of them zero"""
    Q = np.eye(D)
    for _ in range(3):
        v = rng.standard_normal(D)
        Q = _mm(Q, np.eye(D) - 2.0 * np.outer(v, v) / np.dot(v, v))
    out = []
    for _ in range(3):
        w = rng.uniform(0.5, 2.0, D)
        w[:D - dp] = 0.0
        G = _mm(Q, np.diag(w), Q.T)
        out.append(0.5 * (G + G.T))
    return out


@functools.lru_cache(maxsize=None)
def inputs(D, dp, family):
    """seeded inputs of one shape and family; built once, shared, read-only"""
    import torch
    from oracle import sc_oracle as orc
    rng = _rng("wm-inverse", D, dp, family, SEED.get((D, dp, family), 0))
    n = NTRAJ
    c = Case()
    c.D, c.dp, c.family, c.n = D, dp, family, n
    c.Gi, c.Gt, c.G0 = _widths(rng, D, dp)
    c.alpha = c.beta = momentum_heavy_parameters(D)[2] if family == "momentum-heavy" else 0.5
    c.q0, c.p0 = rng.normal(0.0, 0.3, D), rng.normal(0.0, 0.3, D)
    spread = 0.3 / np.sqrt(D)
    c.q, c.p = c.q0 + spread * rng.standard_normal((n, D)), c.p0 + spread * rng.standard_normal((n, D))
    c.Q, c.P = c.q0 + spread * rng.standard_normal((n, D)), c.p0 + spread * rng.standard_normal((n, D))
    c.S = rng.uniform(-2.0, 2.0, n)
    c.probi = rng.uniform(0.5, 2.0, n)
    c.tau1, c.tau2 = rng.normal(0.0, 0.05, D), rng.normal(0.0, 0.05, D)
    c.n1, c.n2 = -HBAR ** 2 * c.tau1, -HBAR ** 2 * 0.5 * float(np.sum(c.tau2))        # unit masses
    # host constants, as the oracle computes them
    T = lambda x: torch.from_numpy(np.array(x, order="C"))
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        U, iGi0, _, _, dprime = orc.ic_sampling_matrices(T(c.Gi), T(c.G0))
        ref = orc.WMOracle(T(c.Gi), T(c.Gt), c.alpha, c.beta)
        ref.Gamma_0 = T(c.G0)
        ref._prepare()
    finally:
        torch.set_num_threads(threads)
    assert dprime == dp
    c.U, c.iGi0 = U.real.numpy().copy(), iGi0.numpy().copy()
    c.iG0 = ref.iGamma_0.numpy().copy()
    c.dets = tuple(float(x) for x in (ref.detG0, ref.detGt, ref.detGi, ref.detGi0))
    if family == "natural":
        c.blocks = _blocks_natural(rng, D, n)
    elif family == "momentum-heavy":
        c.blocks = _blocks_momentum_heavy(rng, D, n)
    else:
        c.blocks = _blocks_far_pivot(rng, c, n)
    for v in vars(c).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def reference_state(c):
    """y [2D + 4 D^2 + 1, n] (the reference's layout) and zi [2D, n] of a case"""
    n, D = c.n, c.D
    y = np.concatenate((c.Q.T, c.P.T, c.blocks.transpose(1, 2, 3, 0).reshape(4 * D * D, n), c.S[None, :]), axis=0)
    return y, np.concatenate((c.q.T, c.p.T), axis=0)


class ConstantCoupling(object):
    """potential with unit masses and constant first and second derivative couplings (nothing else of it is used)"""

    def __init__(self, tau1, tau2):
        import torch
        self.tau1, self.tau2 = torch.from_numpy(np.array(tau1)), torch.from_numpy(np.array(tau2))

    def dimensions(self):
        return self.tau1.shape[0]

    def masses(self):
        import torch
        return torch.ones(self.tau1.shape[0], dtype=torch.float64)

    def derivative_coupling_1st(self, r):
        return self.tau1.to(r.device).unsqueeze(1).expand_as(r)

    def derivative_coupling_2nd(self, r):
        return self.tau2.to(r.device).unsqueeze(1).expand_as(r)


# ---------------------------------------------------------------------------------------------------------------- the terms
def wm_terms(c, t, chk, ct=CLD, inverse=None, det=None, ntraj_norm=None):
    """The WM terms of trajectory t of case c in the complex type ct (clongdouble: the reference), formula by formula as in
    WMOracle._prefactor (eqns 50-84), autocorrelation_qp (85) and ic_correlation (100).  chk: sqrt(c2) sgn of the HK prefactor
    (an input).  inverse(A) -> (A^-1, det A) and det(A) -> det A default to the full-search Gauss-Jordan and det_longdouble;
    with det = None and an `inverse` given, the determinant the inversion returns is used.  The principal roots of detA and
    detM carry the sign +1."""
    rt = LD if ct is CLD else np.float64
    R, C = (lambda a: np.asarray(a, dtype=rt)), (lambda a: np.asarray(a, dtype=ct))
    if inverse is None:
        inverse, det = gauss_jordan, (det_longdouble if ct is CLD else None)
    D, dp = c.D, c.dp
    hb, ih, im = rt(HBAR), rt(1.0) / rt(HBAR), ct(1j)
    pi = rt(np.pi)                                     # the fp64 constant of the oracle and of the engine, held exactly
    Mqq, Mqp, Mpq, Mpp = (R(b) for b in c.blocks[t])
    Gi, Gt, G0, iGi0, iG0, U = R(c.Gi), R(c.Gt), R(c.G0), R(c.iGi0), R(c.iG0), R(c.U)
    q, p, Q, P, q0, p0 = R(c.q[t]), R(c.p[t]), R(c.Q[t]), R(c.P[t]), R(c.q0), R(c.p0)
    one, zero = np.eye(D, dtype=rt), np.zeros((D, D), dtype=rt)
    Mqz, Mpz = np.hstack((Mqq, Mqp)), np.hstack((Mpq, Mpp))
    Eqz, Epz = np.hstack((one, zero)), np.hstack((zero, one))
    # _expand_L
    gradL = im * ih * C(np.concatenate((Mqq.T @ P - p, Mqp.T @ P)))
    hessL = im * ih * C(np.block([[Mpq.T @ Mqq, Mpq.T @ Mqp], [Mqp.T @ Mpq, Mqp.T @ Mpp]]))
    alpha, beta = rt(c.alpha), rt(c.beta)
    filinov = np.block([[alpha * G0, zero], [zero, beta * iG0]])
    A = (C(2 * filinov) - hessL + C(Mqz.T @ Gt @ Mqz + Eqz.T @ Gi @ Eqz)
         + 2 * im * ih * C(Mpz.T @ Mqz - Epz.T @ Eqz))                                        # (50)
    U2 = np.block([[U, np.zeros_like(U)], [np.zeros_like(U), U]])
    Ap = C(U2.T) @ A @ C(U2)
    s = 2 * np.sqrt(alpha * beta)
    As = Ap / s
    iAs, detA_gj = inverse(As)
    detA = det(As) if det is not None else detA_gj
    iA = C(U2) @ (iAs / s) @ C(U2.T)
    BQ = C(Gt @ Mqz) + im * ih * C(Mpz)                                                       # (53)
    Bq = C(Gi @ Eqz) - im * ih * C(Epz)                                                       # (54)
    b0 = gradL - im * ih * C(Mqz.T @ P - Eqz.T @ p)                                           # (55)
    Gtt = C(Gt) - BQ @ iA @ BQ.T                                                              # (57)
    Gti = BQ @ iA @ Bq.T                                                                      # (59)
    pi_t = C(P) - im * hb * (BQ @ iA @ b0)                                                    # (60)
    pi_i = C(p) + im * hb * (Bq @ iA @ b0)
    G0c, iGi0c = C(G0), C(iGi0)
    Cqq = G0c - G0c @ iGi0c @ G0c                                                             # (69)
    CQQ = Gtt - Gti @ iGi0c @ Gti.T                                                           # (70)
    CqQ = G0c @ iGi0c @ Gti.T                                                                 # (71)
    PIq = C(p0) - G0c @ iGi0c @ (C(p0) - pi_i)                                                # (72)
    PIQ = pi_t + Gti @ iGi0c @ (C(p0) - pi_i)                                                 # (73)
    eps = 0.5 * (b0 @ iA @ b0) - 0.5 * ih * ih * ((C(p0) - pi_i) @ iGi0c @ (C(p0) - pi_i))    # (74)
    M = C(U.T) @ (G0c + CQQ) @ C(U)                                                           # (78)
    Ms = M / (2 * pi)
    iMs, detM_gj = inverse(Ms)
    detM = det(Ms) if det is not None else detM_gj
    iM = C(U) @ (iMs / (2 * pi)) @ C(U.T)
    Rqq = Cqq - CqQ @ iM @ CqQ.T                                                              # (79)
    RQQ = G0c - G0c @ iM @ G0c                                                                # (80)
    RqQ = CqQ @ iM @ G0c                                                                      # (81)
    Pq = PIq - CqQ @ iM @ (PIQ - C(p0))                                                       # (82)
    PQ = C(p0) + G0c @ iM @ (PIQ - C(p0))                                                     # (83)
    gamma = eps - 0.5 * ih * ih * ((PIQ - C(p0)) @ iM @ (PIQ - C(p0)))                        # (84)
    dq, dQ = C(q0 - q), C(q0 - Q)
    detG0, detGt, detGi, detGi0 = (rt(x) for x in c.dets)
    pre = (np.sqrt(detG0) * np.sqrt(np.sqrt(detGt)) * np.sqrt(np.sqrt(detGi)) / np.sqrt(detGi0) * ct(chk)
           * np.exp(im * ih * rt(c.S[t])) / np.sqrt(ct(detA)) / np.sqrt(ct(detM)))
    ex = (gamma - 0.5 * (dq @ Rqq @ dq) - 0.5 * (dQ @ RQQ @ dQ) + dq @ RqQ @ dQ
          - im * ih * (Pq @ dq) + im * ih * (PQ @ dQ))
    weight = rt(ntraj_norm if ntraj_norm is not None else c.n) * rt(c.probi[t]) * (2 * pi * hb) ** D
    cq = pre * np.exp(ex) / weight                                                            # (85), Monte-Carlo weight applied
    n1, n2 = C(c.n1), ct(c.n2)
    nacqQ = n1 @ RqQ @ n1
    nacQ = n2 + (dQ @ RQQ @ n1 - dq @ RqQ @ n1 - im * ih * (PQ @ n1))
    nacq = n2 + (dq @ Rqq @ n1 - n1 @ RqQ @ dQ + im * ih * (Pq @ n1))
    kq = ih * ih * (nacqQ + nacQ * nacq) * cq                                                 # (100)
    dvec = CqQ.T @ dq + im * ih * PIQ
    return {"As": As, "detA": detA, "CQQ": CQQ, "dvec": dvec, "Ms": Ms, "detM": detM, "cq": cq, "kq": kq}


@functools.lru_cache(maxsize=None)
def reference(D, dp, family):
    """extended-precision terms of every trajectory of a case, with the HK factor 1 (what set_initial_conditions leaves and the
    WM launch of the tests reads); computed once, shared between the host and the GPU tests"""
    c = inputs(D, dp, family)
    return tuple(wm_terms(c, t, 1.0) for t in range(c.n))


@functools.lru_cache(maxsize=None)
def oracle_terms(D, dp, family):
    """the fp64 oracle's values of the same terms: WMOracle (torch, LAPACK) on the same inputs, HK factor 1, signs +1; the
    per-trajectory k term is ic_correlation without its sum -> list of dicts per trajectory"""
    import torch
    from oracle import sc_oracle as orc
    torch.set_default_dtype(torch.float64)
    c = inputs(D, dp, family)
    T = lambda x: torch.from_numpy(np.array(x, order="C"))
    y, zi = reference_state(c)
    ref = orc.WMOracle(T(c.Gi), T(c.Gt), c.alpha, c.beta)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)       # a handful of matrices: nothing to gain, and batched LAPACK on several threads can stall
    try:
        ref.set_initial_conditions(T(c.q0), T(c.p0), T(c.G0), T(zi), T(c.probi))
        ref.tracker = orc.SignTracker()                   # first sighting of every determinant: signs +1
        ref.y = T(y)
        ref._prefactor()
    finally:
        torch.set_num_threads(threads)
    ref.c = torch.ones(c.n, dtype=orc.C128)
    ref.tracker.state["prefactorC"]["signs"] = torch.ones(c.n, dtype=orc.C128)
    cq_qp = ref.autocorrelation_qp()
    cq = cq_qp / ref._mc_weight()
    q, Q = T(zi[:D]).type(orc.C128), T(y[:D]).type(orc.C128)
    q0 = T(c.q0).unsqueeze(1).expand(-1, c.n).type(orc.C128)
    n1 = T(c.n1).unsqueeze(1).expand(-1, c.n).type(orc.C128)
    e = torch.einsum
    nacqQ = e('in,ijn,jn->n', n1, ref.RqQ, n1)
    nacQ = c.n2 + (e('in,ijn,jn->n', q0 - Q, ref.RQQ, n1) - e('in,ijn,jn->n', q0 - q, ref.RqQ, n1)
                   - 1j / HBAR * e('in,in->n', ref.PQ, n1))
    nacq = c.n2 + (e('in,ijn,jn->n', q0 - q, ref.Rqq, n1) - e('in,jin,jn->n', q0 - Q, ref.RqQ, n1)
                   + 1j / HBAR * e('in,in->n', ref.Pq, n1))
    kq = 1.0 / HBAR ** 2 * (nacqQ + nacQ * nacq) * cq
    dvec = e('jin,jn->in', ref.CqQ, q0 - q) + 1j / HBAR * ref.PIQ
    out = []
    for t in range(c.n):
        out.append({"detA": ref.detA[t].numpy(), "detM": ref.detM[t].numpy(), "CQQ": ref.CQQ[:, :, t].numpy(),
                    "dvec": dvec[:, t].numpy(), "cq": cq[t].numpy(), "kq": kq[t].numpy()})
    return out


# ----------------------------------------------------------------------------------------------------------------- the bound
def rel_err(got, ref):
    """max |got - ref| / max |ref| over the elements of one quantity of one trajectory, evaluated in extended precision"""
    ref = np.asarray(ref, dtype=CLD)
    return float(np.max(np.abs(np.asarray(got).astype(CLD) - ref)) / np.max(np.abs(ref)))


def err64(D, dp, family, t, quantity):
    """error of the fp64 oracle for one trajectory and quantity against the extended-precision reference"""
    return rel_err(oracle_terms(D, dp, family)[t][quantity], reference(D, dp, family)[t][quantity])


def accuracy_bound(D, dp, family, t, quantity):
    """the rule of the determinant tests: 16 x the fp64 oracle's own error plus a floor of a few ulps per elimination step"""
    return 16.0 * err64(D, dp, family, t, quantity) + 4.0 * order(quantity, dp) * 2.0 ** -52

