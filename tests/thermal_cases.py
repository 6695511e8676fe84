"""Host restatement of the thermal Herman-Kluk estimator in torch / numpy, and the exact traces it
estimates.

``thermal_terms`` forms the per-trajectory terms cq_i, kq_i from an oracle propagator's q(t), p(t), S, c (oracle/sc_oracle.py,
used, not changed) run on the same ``zi``: the oracle's own overlap class evaluates the two overlaps with the per-trajectory
centres on the diagonal of its (n, n) result.  ``exact_traces`` evaluates Tr[rho e^{iH_es t} e^{-iH_gs t}] and
hbar^-2 Tr[rho e^{iH_es t} T^+ e^{-iH_gs t} T], T = n1.grad + n2, in a truncated Fock basis of the initial surface.
"""
import numpy as np
import torch

from oracle import sc_oracle as orc

hbar = orc.hbar


def rotated(tc, centres, t):
    """(Q(t), P(t)) (d'', n) of centres (n, 2 d'') and the phase Phi (n,)"""
    dm = tc.dmodes
    c = torch.as_tensor(centres, dtype=torch.float64).cpu()
    Q0, P0 = c[:, :dm].T, c[:, dm:].T
    w = tc.omega.unsqueeze(1)
    cs, sn = torch.cos(w * t), torch.sin(w * t)
    Qt, Pt = Q0 * cs + P0 / w * sn, P0 * cs - w * Q0 * sn
    phi = torch.exp(0.5j / hbar * torch.sum(Q0 * P0 - Qt * Pt, 0))
    return Qt, Pt, phi


def _diag_overlap(cso, q, p, a, b, chunk=64):
    """<q_i, p_i | a_i, b_i> per trajectory: the diagonal of the oracle's (n, n) overlaps, in chunks of trajectories"""
    n = q.shape[1]
    out = torch.zeros(n, dtype=torch.complex128)
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        out[lo:hi] = torch.diagonal(cso(q[:, lo:hi], p[:, lo:hi], a[:, lo:hi], b[:, lo:hi]))
    return out


def thermal_terms(prop, tc, centres, t, potential=None, with_phase=True):
    """(cq, kq), complex (n,) each, of the oracle propagator ``prop`` at its current state, whose clock reads ``t``: the terms
    whose sums are C_T(t) and k_ic,T(t) up to the phase e^{i E0 t / hbar}.  ``potential``: the oracle potential (constant coupling)
    for kq, None: kq = 0.  ``with_phase`` False drops Phi (the mistake the tests have to catch)."""
    q0 = prop.q0.unsqueeze(1)
    Q0, P0, _ = rotated(tc, centres, 0.0)
    Qt, Pt, phi = rotated(tc, centres, t)
    a0, b0, at, bt = q0 + tc.map_q @ Q0, tc.map_p @ P0, q0 + tc.map_q @ Qt, tc.map_p @ Pt
    qi, pi = prop.initial_positions_and_momenta()
    qt, pt = prop.current_positions_and_momenta()
    vi = _diag_overlap(prop.csoi0, qi, pi, a0, b0)
    vt = _diag_overlap(prop.csot0, qt, pt, at, bt)
    cq = vt.conj() * vi * prop.semiclassical_prefactor() * torch.exp(1j / hbar * prop.classical_action()) / prop._mc_weight()
    if with_phase:
        cq = phi * cq
    if potential is None:
        return cq, torch.zeros_like(cq)
    im = 1.0 / potential.masses()
    n1 = -hbar ** 2 * torch.einsum('k,kn->kn', im, potential.derivative_coupling_1st(qi))
    n2 = -hbar ** 2 * 0.5 * torch.einsum('k,kn->n', im, potential.derivative_coupling_2nd(qi))
    G = prop.Gamma_0 @ prop.iGi0
    R = G @ prop.Gamma_i
    PIt, PIi = bt + G @ (pt - bt), b0 + G @ (pi - b0)
    nacQ = n2 + torch.einsum('in,ij,jn->n', at - qt, R, n1) - 1j / hbar * torch.einsum('in,in->n', PIt, n1)
    nacq = n2 + torch.einsum('in,ij,jn->n', a0 - qi, R, n1) + 1j / hbar * torch.einsum('in,in->n', PIi, n1)
    return cq, nacQ * nacq * cq / hbar ** 2


def run_restatement(prop, pot, tc, centres, dt, nt, E0=0.0, with_phase=True):
    """the loop of orc.run_loop on the thermal terms: C (nt,), k (nt,) complex with the phase e^{i E0 t}, the per-trajectory terms
    cq, kq (nt, n) WITHOUT it, and the standard errors sigma_C, sigma_k (sigma_Re + i sigma_Im) of the phased sums"""
    n = prop.ntraj
    C, K = np.zeros(nt, dtype=complex), np.zeros(nt, dtype=complex)
    sC, sK = np.zeros(nt, dtype=complex), np.zeros(nt, dtype=complex)
    cqs, kqs = np.zeros((nt, n), dtype=complex), np.zeros((nt, n), dtype=complex)
    for k in range(nt):
        cq, kq = (x.numpy() for x in thermal_terms(prop, tc, centres, prop.t, pot, with_phase))
        phase = np.exp(1j / hbar * prop.t * E0)
        cqs[k], kqs[k] = cq, kq
        for terms, total, sigma in ((cq, C, sC), (kq, K, sK)):
            x = n * terms * phase                    # per-sample values: their mean is the estimate
            total[k] = x.mean()
            sigma[k] = (x.real.std(ddof=1) + 1j * x.imag.std(ddof=1)) / np.sqrt(n)
        prop.step(pot, dt)
    return C, K, cqs, kqs, sC, sK


# ---------------------------------------------------------------------------------------------------------------- exact traces

def _ladder(nb):
    a = np.diag(np.sqrt(np.arange(1, nb)), 1)
    return a, a.T


def exact_traces(omega, L, masses, q0, pos_gs, hess_gs, nac, kT, times, nbasis):
    """(C_T(t), k_T(t)) for the initial surface with normal modes (omega (d,), L (D, d), masses (D,), minimum q0) and the final
    surface 1/2 (x - pos_gs)^T hess_gs (x - pos_gs), the coupling T = n1.grad, n1 = -hbar^2 nac / m, at k_B T = ``kT`` (0: the
    ground state), in the product Fock basis of the initial surface with ``nbasis`` = (nb_1, ..., nb_d) functions per mode.
    H_es carries its zero-point energy, as e^{i E0 t} e^{i H_es' t} does in the estimator.  All modes thermal (d = D)."""
    omega, masses = np.asarray(omega, dtype=float), np.asarray(masses, dtype=float)
    d = omega.shape[0]
    eyes = [np.eye(nb) for nb in nbasis]

    def embed(op, k):
        mats = list(eyes)
        mats[k] = op
        out = mats[0]
        for m in mats[1:]:
            out = np.kron(out, m)
        return out
    # everything real: P_k = i c_k R_k with R_k = a^+ - a real, so P_k P_l = -c_k c_l R_k R_l and T = (i / hbar) coef.P is real too
    Q, R, num = [], [], []
    c = np.sqrt(hbar * omega / 2)
    for k, nb in enumerate(nbasis):
        a, ad = _ladder(nb)
        Q.append(embed(np.sqrt(hbar / (2 * omega[k])) * (a + ad), k))
        R.append(embed(ad - a, k))
        num.append(np.diag(embed(ad @ a, k)))
    E_es = sum(hbar * omega[k] * (num[k] + 0.5) for k in range(d))
    dim = E_es.shape[0]
    # final surface in the mass-weighted normal coordinates of the initial one
    Hmw = L.T @ (hess_gs / np.sqrt(np.outer(masses, masses))) @ L
    Qg = L.T @ (np.sqrt(masses) * (np.asarray(pos_gs) - np.asarray(q0)))
    H = np.zeros((dim, dim))
    for k in range(d):
        H -= 0.5 * c[k] ** 2 * R[k] @ R[k]
    dQ = [Q[k] - Qg[k] * np.eye(dim) for k in range(d)]
    for k in range(d):
        for l in range(d):
            H += 0.5 * Hmw[k, l] * dQ[k] @ dQ[l]
    H = 0.5 * (H + H.T)
    E_gs, V = np.linalg.eigh(H)
    # T = n1.grad_x = (i / hbar) n1.p_x, p_x = m^1/2 L P
    n1 = -hbar ** 2 * np.asarray(nac, dtype=float) / masses
    coef = (n1 * np.sqrt(masses)) @ L
    T = sum(-1.0 / hbar * coef[k] * c[k] * R[k] for k in range(d))
    if kT > 0:
        wgt = np.exp(-(E_es - E_es.min()) / kT)
        wgt /= wgt.sum()
    else:
        wgt = np.zeros(dim)
        wgt[np.argmin(E_es)] = 1.0
    VhT, TdV, Vh = V.T @ T, T.T @ V, V.T
    C, K = np.zeros(len(times), dtype=complex), np.zeros(len(times), dtype=complex)
    for i, t in enumerate(times):
        es, gs = wgt * np.exp(1j * E_es * t / hbar), np.exp(-1j * E_gs * t / hbar)
        C[i] = np.sum(es * np.einsum('nj,j,jn->n', V, gs, Vh))
        K[i] = np.sum(es * np.einsum('nj,j,jn->n', TdV, gs, VhT)) / hbar ** 2
    return C, K


def model_2d(omega=(0.9, 1.1), gs_omega=(1.2, 1.0), shift=(0.5, -0.3), kT=1.0):
    """The exactness model: D = 2 harmonic initial surface (non-diagonal Gamma_0, unequal masses); final surface with a rotated,
    frequency-shifted Hessian and a shift; constant coupling vector; k_B T = 1.0 = the mean of hbar omega = (0.9, 1.1).  (The
    frequency shifts and the shift are moderate so that the Fock basis converges at a size a test can double.)"""
    masses = np.array([1.0, 1.7])
    omega = np.array(omega, dtype=float)
    th = 0.35
    L = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    sq = np.sqrt(masses)
    Gamma_0 = (sq[:, None] * (L @ np.diag(omega) @ L.T) * sq[None, :]) / hbar
    q0 = np.array([0.3, -0.2])
    phi = -0.5
    Rg = np.array([[np.cos(phi), -np.sin(phi)], [np.sin(phi), np.cos(phi)]])
    hess_gs = sq[:, None] * (Rg @ np.diag(np.array(gs_omega, dtype=float) ** 2) @ Rg.T) * sq[None, :]
    pos_gs = q0 + np.array(shift, dtype=float)
    return {"masses": masses, "Gamma_0": Gamma_0, "q0": q0, "hess_gs": hess_gs, "pos_gs": pos_gs, "nac": np.array([0.6, -0.4]),
            "kT": float(kT), "E0": 0.5 * hbar * omega.sum(), "omega": omega}


def draw_samples(Gi, G0, masses, q0, kT, n, seed):
    """(ThermalConstants, centres (n, 2 d''), zi (2D, n), probi (n,)) drawn on the host from a generator with ``seed``"""
    from semiclassical_amd import hostmath
    tc = hostmath.ThermalConstants(G0, masses, kT, p0=torch.zeros_like(q0))
    gen = torch.Generator().manual_seed(seed)
    _, _, iLz, detLz, dprime = hostmath.sampling_matrices(Gi, G0)
    D = q0.shape[0]
    xi = torch.randn((n, 2 * dprime), dtype=torch.float64, generator=gen).T
    centres = tc.draw_centres(n, gen)
    a, b = tc.cartesian(centres)
    zi = torch.cat((q0.unsqueeze(0) + a, b), 1).T + torch.einsum('ji,jn->in', iLz, xi)
    probi = detLz / (2 * np.pi) ** D * torch.exp(-0.5 * torch.einsum('in,in->n', xi, xi))
    return tc, centres, zi, probi


def synthetic_dense(D, seed, kT=0.006):
    """A dense harmonic model of D modes in molecular magnitudes: unequal masses, a non-diagonal mass-weighted L on the initial
    surface (frequencies 0.004 ... 0.016), a final surface with another rotation, shifted frequencies and a shift of about one
    width over all modes, a constant coupling vector.  The dict of ``model_2d``."""
    rng = np.random.default_rng(seed)
    masses = 1836.0 * rng.uniform(1.0, 12.0, D)
    sq = np.sqrt(masses)
    L, _ = np.linalg.qr(rng.normal(size=(D, D)))
    omega = np.sort(rng.uniform(0.004, 0.016, D))
    Gamma_0 = sq[:, None] * (L @ np.diag(omega) @ L.T) * sq[None, :] / hbar
    Lg, _ = np.linalg.qr(L + 0.2 * rng.normal(size=(D, D)))
    hess_gs = sq[:, None] * (Lg @ np.diag((omega * rng.uniform(0.85, 1.1, D)) ** 2) @ Lg.T) * sq[None, :]
    Gamma_0, hess_gs = 0.5 * (Gamma_0 + Gamma_0.T), 0.5 * (hess_gs + hess_gs.T)
    q0 = rng.normal(size=D) * 0.1
    shift = (L @ (rng.normal(size=D) / np.sqrt(omega))) / sq / np.sqrt(D)
    return {"masses": masses, "Gamma_0": Gamma_0, "q0": q0, "hess_gs": hess_gs, "pos_gs": q0 + shift,
            "nac": rng.normal(size=D) * 1e-2, "kT": float(kT), "E0": 0.5 * hbar * omega.sum(), "omega": omega}


def model_objects(m, kT, n, seed):
    """(oracle propagator with n host-drawn thermal samples, oracle potential, ThermalConstants, centres) of a model dict"""
    T = lambda x: torch.from_numpy(np.asarray(x, dtype=np.float64)).clone()
    G0, q0, masses = T(m["Gamma_0"]), T(m["q0"]), T(m["masses"])
    D = q0.shape[0]
    tc, centres, zi, probi = draw_samples(G0, G0, masses, q0, kT, n, seed)
    prop = orc.HKOracle(G0, G0)
    prop.set_initial_conditions(q0, torch.zeros_like(q0), G0, zi, probi)
    pot = orc.MolecularHarmonicOracle(m["pos_gs"], 0.0, np.zeros(D), m["hess_gs"], m["masses"], m["nac"])
    return prop, pot, tc, centres
