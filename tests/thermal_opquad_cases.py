"""Host restatement of the thermal correlation functions with QUADRATIC operators and the exact traces
they estimate.

``thermal_opquad_terms`` multiplies the thermal terms cq_i of tests/thermal_cases.py (``thermal_terms``, used, not changed) by the
two Gaussian matrix elements in their DIRECT form -- ``quadratic_element`` of tests/test_opquad_host.py with the trajectory's own
centre in the place of (q0, p0) --, with no eigendecomposition of K and none of the folded columns the kernels take.
``exact_operator_traces`` evaluates Tr[rho e^{iH_es t} A e^{-iH_gs t} B] in the truncated Fock basis of the initial surface, x_j x_k
built from the matrices of x_j.
"""
import numpy as np

from tests import thermal_cases as tcs
from tests.test_opcorr_host import restated_rows
from tests.test_opquad_host import quadratic_element
from tests.thermal_opcorr_cases import centre_images, estimate

hbar = tcs.hbar


def with_K(ops, D):
    """(c, m, K) as arrays, a K left out or None as zeros"""
    c, m = np.asarray(ops[0], dtype=float), np.asarray(ops[1], dtype=float)
    K = np.zeros((c.shape[0], D, D)) if len(ops) == 2 or ops[2] is None else np.asarray(ops[2], dtype=float)
    return c, m, K


def thermal_factors(prop, tc, centres, t, bra, ket, frozen_bra=False):
    """(f, g), complex (n, M) each, at the oracle propagator's current state, whose clock reads ``t``:
    f_ia = <a_i(t), b_i(t), Gamma_0|A_a|Q_i, P_i, Gamma_t> / <.|.>, g_ia = <q_i, p_i, Gamma_i|B_a|a_i(0), b_i(0), Gamma_0> / <.|.>.
    ``frozen_bra``: the bra centre left at t = 0 (the mistake the tests have to catch)."""
    D = prop.q0.shape[0]
    a0, b0 = centre_images(prop, tc, centres, 0.0)
    at, bt = (a0, b0) if frozen_bra else centre_images(prop, tc, centres, t)
    qi, pi = (x.numpy() for x in prop.initial_positions_and_momenta())
    qt, pt = (x.numpy() for x in prop.current_positions_and_momenta())
    Gi, Gt, G0 = prop.Gamma_i.numpy(), prop.Gamma_t.numpy(), prop.Gamma_0.numpy()
    f = quadratic_element(*with_K(bra, D), at, bt, G0, qt, pt, Gt)
    g = quadratic_element(*with_K(ket, D), qi, pi, Gi, a0, b0, G0)
    return f, g


def thermal_opquad_terms(prop, tc, centres, t, bra, ket, frozen_bra=False, cq=None):
    """x_ia = f_ia g_ia cq_i, complex (n, M), without the phase e^{i E0 t / hbar}; ``cq``: terms already at hand"""
    if cq is None:
        cq = tcs.thermal_terms(prop, tc, centres, t)[0].numpy()
    f, g = thermal_factors(prop, tc, centres, t, bra, ket, frozen_bra)
    return f * g * cq[:, None]


def run_restatement(prop, pot, tc, centres, dt, nt, bra, ket, E0=0.0, frozen=(False,)):
    """{flag: (X, sigma)}, complex (nt, M) each, with the phase, for every ``frozen_bra`` flag (one pass over the trajectories)"""
    M = np.asarray(bra[0]).shape[0]
    out = {flag: (np.zeros((nt, M), dtype=complex), np.zeros((nt, M), dtype=complex)) for flag in frozen}
    for k in range(nt):
        cq = tcs.thermal_terms(prop, tc, centres, prop.t)[0].numpy()
        for flag, (X, S) in out.items():
            x = thermal_opquad_terms(prop, tc, centres, prop.t, bra, ket, flag, cq)
            X[k], S[k] = estimate(x, np.exp(1j / hbar * prop.t * E0))
        prop.step(pot, dt)
    return out


def rows_of_terms(x, kept=None):
    """the raw rows (M, 5) the kernels write for terms x (n, M)"""
    return restated_rows(x, kept)


def thermal_covariance(tc):
    """Sigma_T = map_q diag(hbar (2 nbar_k + 1) / (2 omega_k)) map_q^T"""
    map_q = tc.map_q.numpy()
    return (map_q * (hbar * (2.0 * tc.nbar.numpy() + 1.0) / (2.0 * tc.omega.numpy()))[None, :]) @ map_q.T


def closed_form_t0(bra, ket, q0, tc):
    """X_a(0) = (alpha_A + 1/2 tr K_A Sigma_T)(alpha_B + 1/2 tr K_B Sigma_T) + a_A^T Sigma_T a_B + 1/2 tr(K_A Sigma_T K_B Sigma_T),
    alpha = c + m.q0 + 1/2 q0^T K q0, a = m + K q0: the closed form of tests/test_opquad_host.py with Sigma -> Sigma_T"""
    q0 = np.asarray(q0, dtype=float)
    D = q0.shape[0]
    Sigma = thermal_covariance(tc)
    out = []
    for (cA, mA, KA), (cB, mB, KB) in zip(zip(*with_K(bra, D)), zip(*with_K(ket, D))):
        alpha = [c + m @ q0 + 0.5 * q0 @ K @ q0 + 0.5 * np.trace(K @ Sigma) for c, m, K in ((cA, mA, KA), (cB, mB, KB))]
        out.append(alpha[0] * alpha[1] + (mA + KA @ q0) @ Sigma @ (mB + KB @ q0) + 0.5 * np.trace(KA @ Sigma @ KB @ Sigma))
    return np.array(out)


def exact_operator_traces(omega, L, masses, q0, pos_gs, hess_gs, kT, times, nbasis, bra, ket):
    """X_a(t) = Tr[rho e^{iH_es t} A_a e^{-iH_gs t} B_a], complex (nt, M): the Fock-basis code of tests/thermal_opcorr_cases.py with
    A_a = c_a + m_a.x + 1/2 x^T K_a x, x_j = q0_j + sum_k map_q[j, k] Q_k, and x_j x_k the product of the two matrices"""
    omega, masses, q0 = np.asarray(omega, dtype=float), np.asarray(masses, dtype=float), np.asarray(q0, dtype=float)
    d, D = omega.shape[0], q0.shape[0]
    eyes = [np.eye(nb) for nb in nbasis]

    def embed(op, k):
        mats = list(eyes)
        mats[k] = op
        out = mats[0]
        for m in mats[1:]:
            out = np.kron(out, m)
        return out
    Q, R, num = [], [], []
    c = np.sqrt(hbar * omega / 2)
    for k, nb in enumerate(nbasis):
        a, ad = tcs._ladder(nb)
        Q.append(embed(np.sqrt(hbar / (2 * omega[k])) * (a + ad), k))
        R.append(embed(ad - a, k))
        num.append(np.diag(embed(ad @ a, k)))
    E_es = sum(hbar * omega[k] * (num[k] + 0.5) for k in range(d))
    dim = E_es.shape[0]
    Hmw = L.T @ (hess_gs / np.sqrt(np.outer(masses, masses))) @ L
    Qg = L.T @ (np.sqrt(masses) * (np.asarray(pos_gs) - q0))
    H = np.zeros((dim, dim))
    for k in range(d):
        H -= 0.5 * c[k] ** 2 * R[k] @ R[k]
    dQ = [Q[k] - Qg[k] * np.eye(dim) for k in range(d)]
    for k in range(d):
        for l in range(d):
            H += 0.5 * Hmw[k, l] * dQ[k] @ dQ[l]
    E_gs, V = np.linalg.eigh(0.5 * (H + H.T))
    if kT > 0:
        wgt = np.exp(-(E_es - E_es.min()) / kT)
        wgt /= wgt.sum()
    else:
        wgt = np.zeros(dim)
        wgt[np.argmin(E_es)] = 1.0
    map_q = L / np.sqrt(masses)[:, None]
    x = [q0[j] * np.eye(dim) + sum(map_q[j, k] * Q[k] for k in range(d)) for j in range(D)]

    def matrix(ops, a):
        cs, ms, Ks = ops
        out = cs[a] * np.eye(dim) + sum(ms[a, j] * x[j] for j in range(D))
        for j in range(D):
            for k in range(D):
                if Ks[a, j, k] != 0.0:
                    out = out + 0.5 * Ks[a, j, k] * (x[j] @ x[k])
        return out
    bra, ket = with_K(bra, D), with_K(ket, D)
    M = bra[0].shape[0]
    X = np.zeros((len(times), M), dtype=complex)
    for a in range(M):
        AV, VtB = matrix(bra, a) @ V, V.T @ matrix(ket, a)
        for i, t in enumerate(times):
            es, gs = wgt * np.exp(1j * E_es * t / hbar), np.exp(-1j * E_gs * t / hbar)
            X[i, a] = np.sum(es * np.einsum('nj,j,jn->n', AV, gs, VtB))
    return X


def exactness_pairs():
    """the four pairs of the exactness check on the 2-D model: (x_0^2, 1); the same mixed quadratic operator on both sides;
    (x_0 x_1, x_0 x_1); a mixed quadratic bra against a linear ket"""
    z = np.zeros((2, 2))
    bra = (np.array([0.0, 0.7, 0.0, 0.2]), np.array([[0.0, 0.0], [0.4, -0.3], [0.0, 0.0], [0.1, 0.5]]),
           np.array([[[2.0, 0.0], [0.0, 0.0]], [[0.5, 0.2], [0.2, -0.3]], [[0.0, 1.0], [1.0, 0.0]], [[0.3, -0.4], [-0.4, 0.1]]]))
    ket = (np.array([1.0, 0.7, 0.0, -0.3]), np.array([[0.0, 0.0], [0.4, -0.3], [0.0, 0.0], [0.6, 0.2]]),
           np.array([z, [[0.5, 0.2], [0.2, -0.3]], [[0.0, 1.0], [1.0, 0.0]], z]))
    return bra, ket


def folded_value(cols, q, p, Qc, Pc):
    """sum_col lam z^p, z = kappa + u.q + i w.p + ut.Qc + i wt.Pc, (n, M): what the kernels compute from the columns of
    hostmath.fold_thermal_quadratic_operators (as numpy); q, p (D, n), Qc, Pc (d'', n)"""
    u, w, kap, lam, ut, wt = cols[:6]
    z = (kap[None] + np.einsum('acd,dn->nac', u, q) + 1j * np.einsum('acd,dn->nac', w, p)
         + np.einsum('acd,dn->nac', ut, Qc) + 1j * np.einsum('acd,dn->nac', wt, Pc))
    return (lam[None, :, :1] * z[:, :, :1]).sum(2) + (lam[None, :, 1:] * z[:, :, 1:] ** 2).sum(2)
