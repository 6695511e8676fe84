"""Host restatement of the thermal operator correlation functions and the exact traces they estimate.

``thermal_opcorr_terms`` multiplies the thermal terms cq_i of tests/thermal_cases.py (``thermal_terms``, used, not changed) by the
two Gaussian matrix elements in their DIRECT form (``position_element`` of tests/test_opcorr_host.py with the trajectory's own
centre in the place of (q0, p0)), not the folded one the kernels take.  ``exact_operator_traces`` evaluates
Tr[rho e^{iH_es t} A e^{-iH_gs t} B] with the operators in the truncated Fock basis of the initial surface, where
x_j = q0_j + sum_k map_q[j, k] Q_k.
"""
import numpy as np

from tests import thermal_cases as tcs
from tests.test_opcorr_host import position_element, restated_rows

hbar = tcs.hbar


def centre_images(prop, tc, centres, t):
    """(a(t), b(t)), (D, n) each: the Cartesian images of the centres rotated to the time t"""
    Qt, Pt, _ = tcs.rotated(tc, centres, t)
    return (prop.q0.unsqueeze(1) + tc.map_q @ Qt).numpy(), (tc.map_p @ Pt).numpy()


def thermal_factors(prop, tc, centres, t, bra, ket, frozen_bra=False):
    """(f, g), complex (n, M) each, at the oracle propagator's current state, whose clock reads ``t``:
    f_ia = cA_a + mA_a.<a_i(t), b_i(t), Gamma_0|x|Q_i, P_i, Gamma_t> / <.|.>, g_ia = cB_a + mB_a.<q_i, p_i, Gamma_i|x|a_i(0),
    b_i(0), Gamma_0> / <.|.>.  ``frozen_bra``: the bra centre left at t = 0 (the mistake the tests have to catch)."""
    a0, b0 = centre_images(prop, tc, centres, 0.0)
    at, bt = (a0, b0) if frozen_bra else centre_images(prop, tc, centres, t)
    qi, pi = (x.numpy() for x in prop.initial_positions_and_momenta())
    qt, pt = (x.numpy() for x in prop.current_positions_and_momenta())
    Gi, Gt, G0 = prop.Gamma_i.numpy(), prop.Gamma_t.numpy(), prop.Gamma_0.numpy()
    f = np.asarray(bra[0])[None, :] + (np.asarray(bra[1]) @ position_element(at, bt, G0, qt, pt, Gt)).T
    g = np.asarray(ket[0])[None, :] + (np.asarray(ket[1]) @ position_element(qi, pi, Gi, a0, b0, G0)).T
    return f, g


def thermal_opcorr_terms(prop, tc, centres, t, bra, ket, frozen_bra=False):
    """x_ia = f_ia g_ia cq_i, complex (n, M), without the phase e^{i E0 t / hbar}"""
    cq = tcs.thermal_terms(prop, tc, centres, t)[0].numpy()
    f, g = thermal_factors(prop, tc, centres, t, bra, ket, frozen_bra)
    return f * g * cq[:, None]


def estimate(x, phase=1.0):
    """(X, sigma) of terms x (n, M) with the weight 1 / N inside: the sums and the standard errors sigma_Re + i sigma_Im of the
    per-sample values N x phase (ddof = 1)"""
    n = x.shape[0]
    s = n * x * phase
    return s.mean(0), (s.real.std(0, ddof=1) + 1j * s.imag.std(0, ddof=1)) / np.sqrt(n)


def run_restatement(prop, pot, tc, centres, dt, nt, bra, ket, E0=0.0, frozen=(False,)):
    """{flag: (X, sigma)}, complex (nt, M) each: the loop of thermal_cases.run_restatement on the operator terms, with the phase,
    for every ``frozen_bra`` flag asked for (one pass over the trajectories)"""
    M = np.asarray(bra[0]).shape[0]
    out = {flag: (np.zeros((nt, M), dtype=complex), np.zeros((nt, M), dtype=complex)) for flag in frozen}
    for k in range(nt):
        cq = tcs.thermal_terms(prop, tc, centres, prop.t)[0].numpy()
        for flag, (X, S) in out.items():
            f, g = thermal_factors(prop, tc, centres, prop.t, bra, ket, flag)
            X[k], S[k] = estimate(f * g * cq[:, None], np.exp(1j / hbar * prop.t * E0))
        prop.step(pot, dt)
    return out


def rows_of_terms(x, kept=None):
    """the raw rows (M, 5) the kernels write for terms x (n, M)"""
    return restated_rows(x, kept)


def closed_form_t0(bra, ket, q0, tc):
    """X_a(0) = (cA + mA.q0)(cB + mB.q0) + mA^T map_q diag(hbar (2 nbar_k + 1) / (2 omega_k)) map_q^T mB"""
    q0, map_q = np.asarray(q0), tc.map_q.numpy()
    var = hbar * (2.0 * tc.nbar.numpy() + 1.0) / (2.0 * tc.omega.numpy())
    return ((bra[0] + bra[1] @ q0) * (ket[0] + ket[1] @ q0)
            + np.einsum('ak,k,ak->a', np.asarray(bra[1]) @ map_q, var, np.asarray(ket[1]) @ map_q))


def exact_operator_traces(omega, L, masses, q0, pos_gs, hess_gs, kT, times, nbasis, bra, ket):
    """X_a(t) = Tr[rho e^{iH_es t} A_a e^{-iH_gs t} B_a], complex (nt, M), in the product Fock basis of the initial surface with
    ``nbasis`` functions per mode: the surfaces and the density of thermal_cases.exact_traces (H_es carries its zero-point energy),
    the operators A_a = cA_a + mA_a.x with x_j = q0_j + sum_k map_q[j, k] Q_k, map_q = m^-1/2 L.  All modes thermal."""
    omega, masses, q0 = np.asarray(omega, dtype=float), np.asarray(masses, dtype=float), np.asarray(q0, dtype=float)
    d = omega.shape[0]
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

    def matrix(cm, a):
        coef = np.asarray(cm[1])[a] @ map_q
        return (cm[0][a] + np.asarray(cm[1])[a] @ q0) * np.eye(dim) + sum(coef[k] * Q[k] for k in range(d))
    M = np.asarray(bra[0]).shape[0]
    X = np.zeros((len(times), M), dtype=complex)
    for a in range(M):
        AV, VtB = matrix(bra, a) @ V, V.T @ matrix(ket, a)
        for i, t in enumerate(times):
            es, gs = wgt * np.exp(1j * E_es * t / hbar), np.exp(-1j * E_gs * t / hbar)
            X[i, a] = np.sum(es * np.einsum('nj,j,jn->n', AV, gs, VtB))
    return X


def exactness_pairs():
    """the four pairs of the exactness check on the 2-D model: (1, 1); the same mixed operator on both sides; (x_0, 1); two
    different mixed operators"""
    bra = (np.array([1.0, 0.7, 0.0, 0.2]), np.array([[0.0, 0.0], [0.4, -0.3], [1.0, 0.0], [0.1, 0.5]]))
    ket = (np.array([1.0, 0.7, 1.0, -0.3]), np.array([[0.0, 0.0], [0.4, -0.3], [0.0, 0.0], [0.6, 0.2]]))
    return bra, ket
