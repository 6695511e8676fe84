"""Numpy restatement of WaltonManolopoulosPropagator.wm_expectation: the direct formula with np.linalg.inv and
slogdet -- no fold, no eigendecomposition --, the same model evaluated from the folded columns, and the states it is fed with.

A state is a dict  Q (n, D) real, coef (n,), cqq (n, D, D), dvec (n, D) complex, U (D, d') real:  psi(x) = sum_n coef_n g_n(x),
g_n(x) = exp(-1/2 (x - Q_n)^T cqq_n (x - Q_n) + dvec_n . (x - Q_n));  optionally cqqp (n, d', d') in the place of U^T cqq U.
"""
import numpy as np

HBAR = 1.0


def oracle_state(ref, sel=slice(None)):
    """the state of a WMOracle (oracle/sc_oracle.py), as oracle/norm_oracle.py:wm_norm reads it"""
    from oracle import norm_oracle
    import torch
    v = norm_oracle.wm_coefficients(ref)
    q, _ = ref.initial_positions_and_momenta()
    Q, _ = ref.current_positions_and_momenta()
    q0 = ref.q0.unsqueeze(1).expand_as(q).type(torch.complex128)
    dvec = torch.einsum('ban,bn->an', ref.CqQ, q0 - q) + 1j / HBAR * ref.PIQ
    U = ref.U.real if ref.U.is_complex() else ref.U
    return dict(Q=Q.numpy().T[sel].copy(), coef=v.numpy()[sel].copy(), cqq=ref.CQQ.permute(2, 0, 1).numpy()[sel].copy(),
                dvec=dvec.numpy().T[sel].copy(), U=U.numpy().copy())


def engine_state(prop, sel=slice(None)):
    """the state of the engine's propagator: its own _export() and _qp"""
    coef, cqq, dvec = (t.cpu().numpy() for t in prop._export())
    return dict(Q=prop._qp.cpu().numpy()[:, :prop.dim][sel].copy(), coef=coef[sel].copy(), cqq=cqq[sel].copy(), dvec=dvec[sel].copy(),
                U=prop._wm_bufs["U"].cpu().numpy().copy())


def projected(U, C):
    """U^T C_n U of every trajectory (einsum with optimize: numpy's plain contraction of three operands takes seconds at D = 64)"""
    return np.einsum('ak,nab,bl->nkl', U, C, U, optimize=True)


def pair_system(bra, ket):
    """(T, Dp, b): T_ij = conj(v_i) O_ij v_j (ni, nj), D'_ij (ni, nj, d', d') and b'_ij (ni, nj, d') of every pair; the determinant
    through slogdet (principal square root)"""
    U = ket["U"]
    dQ = ket["Q"][None, :, :] - bra["Q"][:, None, :]                                          # (ni, nj, D)
    project = lambda s: s["cqqp"] if "cqqp" in s else projected(U, s["cqq"])      # (a test may set C' itself)
    Dp = project(bra).conj()[:, None] + project(ket)[None, :]
    CdQ = np.einsum('jab,ijb->ija', ket["cqq"], dQ)
    b = np.einsum('ija,ak->ijk', CdQ, U, optimize=True) + (bra["dvec"] @ U).conj()[:, None, :] + (ket["dvec"] @ U)[None, :, :]
    sign, logabs = np.linalg.slogdet(Dp / (2 * np.pi))
    ex = (-0.5 * np.einsum('ija,ija->ij', dQ, CdQ) - np.einsum('ja,ija->ij', ket["dvec"], dQ)
          + 0.5 * np.einsum('ijk,ijk->ij', b, np.linalg.solve(Dp, b[..., None])[..., 0]))
    T = np.conj(bra["coef"])[:, None] * np.exp(ex - 0.5 * logabs) / np.sqrt(sign) * ket["coef"][None, :]
    return T, Dp, b


def _parts(D, c, m, K, n):
    M = next(len(t) for t in (c, m, K, n) if t is not None)
    z = lambda t, shape: np.zeros((M,) + shape) if t is None else np.asarray(t, dtype=float)
    return M, z(c, ()), z(m, (D,)), z(K, (D, D)), z(n, (D,))


def pair_elements(bra, ket, c=None, m=None, K=None, n=None):
    """(T, F): F_a,ij (M, ni, nj) of  c + m.x + 1/2 x^T K x + n.p,  the direct formula:
        xbar = Q_i + U D'^-1 b',   B = U D'^-1 U^T,
        F = c + m.xbar + 1/2 xbar^T K xbar + 1/2 tr(K B) - i hbar [ n.d_j - (C_j n).(xbar - Q_j) ]"""
    U = ket["U"]
    M, c, m, K, n = _parts(U.shape[0], c, m, K, n)
    T, Dp, b = pair_system(bra, ket)
    iD = np.linalg.inv(Dp)
    xbar = bra["Q"][:, None, :] + np.einsum('ak,ijkl,ijl->ija', U, iD, b, optimize=True)
    B = np.einsum('ak,ijkl,bl->ijab', U, iD, U, optimize=True)
    Cn = np.einsum('jab,mb->mja', ket["cqq"], n)                                              # (M, nj, D)
    F = (c[:, None, None] + np.einsum('ma,ija->mij', m, xbar) + 0.5 * np.einsum('ija,mab,ijb->mij', xbar, K, xbar)
         + 0.5 * np.einsum('mab,ijab->mij', K, B)
         - 1j * HBAR * ((n @ ket["dvec"].T)[:, None, :] - np.einsum('mja,ija->mij', Cn, xbar - ket["Q"][None, :, :])))
    return T, F


def restated_expectation(bra, ket, c=None, m=None, K=None, n=None):
    """(E, A, N2): E_a = sum_ij T_ij F_a,ij, A_a = sum_ij |T_ij F_a,ij|, N2 = sum_ij T_ij"""
    T, F = pair_elements(bra, ket, c, m, K, n)
    terms = T[None] * F
    return terms.sum(axis=(1, 2)), abs(terms).sum(axis=(1, 2)), T.sum()


def column_elements(Dp, b, za, zb, g, sfix, sket, lam, kap):
    """F_a,ij (M, ni, nj) from the columns as sc_wm_pair_expect reads them (include/semiclassical_hip.h): za (C, ni), zb (C, nj), g,
    sfix (C, d'), sket (M, nj, d') or None, lam (M, 1 + R), kap (M,)"""
    M, C1 = lam.shape
    ni, nj, dp = b.shape
    iD = np.linalg.inv(Dp)
    s = np.broadcast_to(sfix[:, None, :], (M * C1, nj, dp)).astype(complex)                   # (C, nj, d')
    if sket is not None:
        s[np.arange(M) * C1] += sket
    st = s.transpose(1, 2, 0)                                                                 # (nj, d', C)
    sDb = np.einsum('jkc,ijkl,ijl->cij', st, iD, b, optimize=True)
    sDs = np.einsum('jkc,ijkc->cij', st, np.einsum('ijkl,jlc->ijkc', iD, st, optimize=True))
    l = za[:, :, None] + zb[:, None, :] + np.einsum('ck,ijk->cij', g, b) + sDb
    squared = (np.arange(M * C1) % C1 != 0)[:, None, None]
    f = np.where(squared, l * l + sDs, l).reshape(M, C1, ni, nj)
    return kap[:, None, None] + np.einsum('mc,mcij->mij', lam, f)


def wavefunction(state, x):
    """(psi, grad psi) on the grid x (nx, D): (nx,), (nx, D)"""
    dx = x[None, :, :] - state["Q"][:, None, :]                                               # (n, nx, D)
    Cdx = np.einsum('nab,nxb->nxa', state["cqq"], dx)
    gauss = state["coef"][:, None] * np.exp(-0.5 * np.einsum('nxa,nxa->nx', dx, Cdx) + np.einsum('na,nxa->nx', state["dvec"], dx))
    return gauss.sum(0), np.einsum('nx,nxa->xa', gauss, state["dvec"][:, None, :] - Cdx)


def random_direction(rng, U):
    """a unit vector in the range of U"""
    u = U @ rng.standard_normal(U.shape[1])
    return u / np.linalg.norm(u)


def standard_operators(rng, U):
    """(c, m, K, n) of the four operators 1, u.x, u.p, (u.x)^2 along one random unit vector u in the range of U"""
    D = U.shape[0]
    u = random_direction(rng, U)
    c, m, K, n = np.zeros(4), np.zeros((4, D)), np.zeros((4, D, D)), np.zeros((4, D))
    c[0], m[1], n[2], K[3] = 1.0, u, u, 2.0 * np.outer(u, u)
    return c, m, K, n
