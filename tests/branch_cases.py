"""Constructions for the branch-tracker tests: hand-made monodromy states whose predecessor determinant is mirrored so that
the sqrt branch rule (reference propagators.py:1006-1066, oracle/sc_oracle.py SignTracker) must flip or must not flip.

CPU only (oracle + torch): tests/test_branch_tracking_host.py checks every premise here without a GPU,
tests/test_branch_tracking_gpu.py drives the engine from the same states."""
import copy

import numpy as np
import torch

from oracle import sc_oracle as orc

MARGIN = 1e-6            # |Re z|, |Im z| >= MARGIN |z|: a 1e-12 difference between kernel and oracle cannot decide a flip
MIN_PER_CATEGORY = 3

# categories of a (predecessor, determinant) pair
FLIP, SAME, PREV_RE_POS, Z_RE_POS = 0, 1, 2, 3


def would_flip(prev, z):
    """the tracker's rule: both real parts negative and the imaginary part changes sign"""
    return (prev.real < 0) & (z.real < 0) & (prev.imag * z.imag < 0)


def mirror(z, gen):
    """predecessors for the determinants z (n,): Re z < 0 -> conj(z)(1+d) (must flip), z(1+d) (must not) or -conj(z)(1+d)
    (Re > 0: must not); Re z > 0 -> -z(1+d) (Re < 0 and opposite Im: only Re z > 0 prevents the flip).  Returns
    (prev, incoming signs +-1, category)"""
    n = z.shape[0]
    u = torch.rand(n, generator=gen, dtype=torch.float64)
    delta = 0.6 * torch.rand(n, generator=gen, dtype=torch.float64) - 0.3
    cat = torch.where(z.real > 0, Z_RE_POS, torch.where(u < 0.5, FLIP, torch.where(u < 0.75, SAME, PREV_RE_POS)))
    prev = torch.where(cat == FLIP, z.conj(), torch.where(cat == SAME, z, torch.where(cat == PREV_RE_POS, -z.conj(), -z)))
    prev = prev * (1.0 + delta)
    sgn = torch.where(torch.rand(n, generator=gen, dtype=torch.float64) < 0.5, -1.0, 1.0).to(torch.float64)
    return prev, sgn, cat


def assert_margin(z, what="z"):
    a = z.abs()
    assert bool(torch.all(z.real.abs() >= MARGIN * a)) and bool(torch.all(z.imag.abs() >= MARGIN * a)), \
        f"{what}: a determinant lies within {MARGIN} |z| of an axis: the flip would be decided by rounding"


def assert_premise(z, prev, cat, minimum=MIN_PER_CATEGORY):
    """every category is populated (flips in both directions of Im), margins hold, and the rule flips exactly FLIP"""
    assert_margin(z)
    assert_margin(prev, "prev")
    counts = {"flip Im -+": int(((cat == FLIP) & (z.imag > 0)).sum()), "flip Im +-": int(((cat == FLIP) & (z.imag < 0)).sum()),
              "no flip": int((cat == SAME).sum()), "prev Re > 0": int((cat == PREV_RE_POS).sum()),
              "z Re > 0": int((cat == Z_RE_POS).sum())}
    assert min(counts.values()) >= minimum, counts
    assert torch.equal(would_flip(prev, z), cat == FLIP)
    return counts


# ---------------------------------------------------------------------------------------------------- models
class Case(object):
    """host inputs of one row: widths, initial conditions, oracle potential, time step, and what builds the engine potential"""

    def __init__(self, kind, D, Gi, q0, p0, oracle_pot, dt, engine_args, wm=None):
        self.kind, self.D, self.Gi, self.q0, self.p0 = kind, D, Gi, q0, p0
        self.oracle_pot, self.dt, self.engine_args, self.wm = oracle_pot, dt, engine_args, wm

    def oracle(self, n, seed):
        ref = orc.WMOracle(self.Gi, self.Gi, *self.wm) if self.wm else orc.HKOracle(self.Gi, self.Gi)
        torch.manual_seed(seed)
        ref.initial_conditions(self.q0, self.p0, self.Gi, ntraj=n)
        return ref

    def engine_potential(self):
        from semiclassical_amd import potentials as P
        if self.kind == "morse":
            omega, chi, nac = self.engine_args
            return P.MorsePotential(omega, chi.clone(), nac)
        if self.kind == "harmonic":
            return P.MolecularHarmonicPotential.from_arrays(*self.engine_args)
        if self.kind == "generic":
            return self.oracle_pot
        raise ValueError(self.kind)


def _rotated(w, rng):
    Q, _ = np.linalg.qr(rng.standard_normal((len(w), len(w))))
    G = (Q * w) @ Q.T
    return torch.from_numpy(0.5 * (G + G.T))


def morse_case(D, diag=True, seed=0, dt=4.0, wm=None, width=1.0):
    """the synthetic AS model (anharmonic, separable): diagonal widths = diag(width omega), else width omega rotated by a
    random basis"""
    from semiclassical_amd.synthetic import anharmonic_as_model
    omega, chi, nac, q0, _ = anharmonic_as_model(D)
    w = width * omega
    G = torch.diag(w) if diag else _rotated(w.numpy(), np.random.default_rng(seed))
    return Case("morse", D, G, q0, 0.0 * q0, orc.MorseOracle(omega, chi.clone(), nac), dt, (omega, chi, nac), wm=wm)


def wm_rerun_case(D=12, zero_modes=6):
    """the model of tests/test_wm_gpu.py::test_wm_weak_fixed_order_pivots_are_rerun_with_pivoting: harmonic separable modes,
    rotated rank-deficient widths, alpha = beta = 0.05"""
    rng = np.random.default_rng(7 + D)
    omega = torch.from_numpy(np.sort(rng.uniform(600, 2500, D)) / 219474.63)
    nac = torch.from_numpy(rng.normal(0, 1e-3, D))
    q0 = torch.from_numpy(rng.normal(0, 1.0, D))
    Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    w = omega.numpy() * rng.uniform(0.7, 1.4, D)
    w[:zero_modes] = 0.0
    G = torch.from_numpy(Q @ np.diag(w) @ Q.T)
    G = 0.5 * (G + G.T)
    chi = torch.zeros(D)
    return Case("morse", D, G, q0, torch.zeros(D), orc.MorseOracle(omega, chi.clone(), nac), 2.0, (omega, chi, nac),
                wm=(0.05, 0.05))


def harmonic_case(D, diag=True, zero_modes=0, seed=0, dt=40.0):
    """a constant dense SPD Hessian in mass-weighted random modes; diagonal or dense (rank-deficient) widths"""
    rng = np.random.default_rng(100 + seed)
    masses = rng.uniform(1800.0, 22000.0, D)
    Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    om = rng.uniform(500, 3000, D) / 219474.63
    sm = np.sqrt(masses)
    hess0 = (Q * om ** 2) @ Q.T * np.outer(sm, sm)
    hess0 = 0.5 * (hess0 + hess0.T)
    pos0, grad0, nac0 = rng.normal(0, 0.1, D), rng.normal(0, 1e-3, D), rng.normal(0, 1e-2, D)
    args = (pos0, np.float64(-0.3), grad0, hess0, masses, nac0)
    w = om * rng.uniform(0.7, 1.4, D)
    if diag:
        G = torch.from_numpy(np.diag(w * masses))
    else:
        w[:zero_modes] = 0.0
        G = _rotated(w, rng) * torch.from_numpy(np.outer(sm, sm))
        G = 0.5 * (G + G.T)
    q0 = torch.from_numpy(pos0 + rng.normal(0, 0.05, D))
    return Case("harmonic", D, G, q0, torch.zeros(D), orc.MolecularHarmonicOracle(*args), dt, args)


class CoupledQuartic(object):
    """V = 1/2 sum w_a^2 r_a^2 + lam (sum r_a r_{a+1})^2 in plain torch: no device descriptor, so the engine evaluates it at the
    stage points and takes the dense path (sc_dense_mono_step); the oracle drives the very same object on the host"""

    def __init__(self, omega, lam, nac):
        self.omega, self.lam, self.nac = omega, lam, nac

    def dimensions(self):
        return len(self.omega)

    def masses(self):
        return torch.ones(len(self.omega), dtype=torch.float64)

    def harmonic_approximation(self, r):
        w2 = (self.omega ** 2).to(r.device).unsqueeze(1)
        d, n = r.shape
        s = torch.sum(r[:-1] * r[1:], dim=0)
        ds = torch.zeros_like(r)
        ds[:-1] += r[1:]
        ds[1:] += r[:-1]
        V = 0.5 * torch.sum(w2 * r * r, dim=0) + self.lam * s * s
        grad = w2 * r + 2.0 * self.lam * s * ds
        hess = 2.0 * self.lam * ds.unsqueeze(1) * ds.unsqueeze(0)
        idx = torch.arange(d, device=r.device)
        hess[idx, idx] += w2.expand(-1, n)
        hess[idx[:-1], idx[1:]] += 2.0 * self.lam * s
        hess[idx[1:], idx[:-1]] += 2.0 * self.lam * s
        return V, grad, hess

    def derivative_coupling_1st(self, r):
        return self.nac.to(r.device).unsqueeze(1).expand(-1, r.shape[1])

    def derivative_coupling_2nd(self, r):
        return torch.zeros_like(r)


def generic_case(D, seed=0, dt=4.0):
    rng = np.random.default_rng(200 + seed)
    omega = torch.from_numpy(np.sort(rng.uniform(500, 3000, D)) / 219474.63)
    pot = CoupledQuartic(omega, 2e-6, torch.from_numpy(rng.normal(0, 1e-3, D)))
    q0 = torch.from_numpy(rng.uniform(-3.0, 3.0, D))
    return Case("generic", D, torch.diag(omega), q0, torch.zeros(D), pot, dt, None)


# ---------------------------------------------------------------------------------------------------- monodromy blocks
def _unit_scales(D, g):
    """per-block scale matrices that make every term of the prefactor matrix O(1): Mqp ~ 1 / gamma, Mpq ~ gamma (g = the
    diagonal of Gamma); without them the i / gamma Mpq term dominates and every determinant has the phase i^D"""
    g = torch.ones(D, dtype=torch.float64) if g is None else torch.as_tensor(g, dtype=torch.float64).abs().clamp_min(1e-12)
    s = torch.sqrt(torch.outer(g, g)).unsqueeze(2)
    return [1.0, 1.0 / s, s, 1.0]


def dense_blocks(D, n, gen, g=None, scale=(1.0, 1.0, 1.0, 1.0), noise=0.3):
    """the blocks of a free rotation by a random angle theta_a per mode (diagonal; prefactor-matrix entry e^(-i theta_a), so the
    phases of the determinants cover the circle) + N(0, noise^2) in every entry, in the units of the widths: diagonally
    dominant, yet the in-block elimination really pivots"""
    theta = (2 * torch.rand(D, n, generator=gen, dtype=torch.float64) - 1) * np.pi
    units = _unit_scales(D, g)
    base = [torch.diag_embed(f(theta).t()).permute(1, 2, 0) for f in (torch.cos, torch.sin, lambda t: -torch.sin(t), torch.cos)]
    return [scale[k] * units[k] * (base[k] + noise * torch.randn(D, D, n, generator=gen, dtype=torch.float64))
            for k in range(4)]


def shifted_blocks(D, n, shift, gen, g=None):
    """every block = a cyclic shift by `shift` columns with random entries: the leading pivots of a fixed or in-block order are
    zero, so the fully pivoted fix-up does the determinant -- and its tracking"""
    pat = torch.roll(torch.eye(D, dtype=torch.float64), shift, dims=1).unsqueeze(2)
    return [u * pat * torch.randn(D, D, n, generator=gen, dtype=torch.float64) for u in _unit_scales(D, g)]


def diagonal_blocks(D, n, gen, g=None):
    """diagonal blocks with random entries (the separable shortcut keeps only diagonals)"""
    out = []
    for u in _unit_scales(D, g):
        b = torch.zeros(D, D, n, dtype=torch.float64)
        torch.diagonal(b, dim1=0, dim2=1)[...] = torch.randn(n, D, generator=gen, dtype=torch.float64)
        out.append(u * b)
    return out


def with_blocks(y, D, blocks):
    y = y.clone()
    for k, blk in enumerate(blocks):
        y[2 * D + k * D * D: 2 * D + (k + 1) * D * D] = blk.reshape(D * D, -1)
    return y


# ---------------------------------------------------------------------------------------------------- oracle side
TRACKED = {"prefactorC": "c2", "detA": "detA", "detM": "detM"}


def keys_of(ref):
    return ("prefactorC", "detA", "detM") if isinstance(ref, orc.WMOracle) else ("prefactorC",)


def oracle_from(ref, y):
    """a copy of `ref` at the state y (trackers untouched)"""
    r = copy.deepcopy(ref)
    r.y = y.clone()
    return r


def determinants_after(ref, y, pot, dt, steps=1):
    """{key: [z after step 1, ..., z after step `steps`]} of the oracle from state y; z depends on the state only"""
    r = oracle_from(ref, y)
    out = {k: [] for k in keys_of(ref)}
    for _ in range(steps):
        r.step(pot, dt)
        for k in out:
            out[k].append(getattr(r, TRACKED[k]).clone())
    return out


def install_predecessor(ref, key, prev, sgn):
    """the tracker state of the oracle: predecessor `prev`, incoming signs `sgn` (and the unsigned prefactor that goes with
    them, which the correlation functions of the current step use)"""
    ref.tracker.state[key] = {"signs": sgn.clone().to(torch.complex128), "previous": prev.clone()}
    if key == "prefactorC":
        ref.c2, ref.c = prev.clone(), torch.sqrt(prev)
    else:
        setattr(ref, TRACKED[key], prev.clone())


def mirrored_setup(ref, y, pot, dt, seed, minimum=MIN_PER_CATEGORY, premise_keys=None):
    """for every tracked key of `ref`: the determinant z of the next step from y, a mirrored predecessor and random incoming
    signs, the premise asserted (category counts only for `premise_keys`, default all; margins for all).
    Returns {key: (z, prev, sgn, cat)}"""
    gen = torch.Generator().manual_seed(seed)
    zs = determinants_after(ref, y, pot, dt)
    out = {}
    for key, (z,) in zs.items():
        prev, sgn, cat = mirror(z, gen)
        assert_premise(z, prev, cat, minimum if premise_keys is None or key in premise_keys else 0)
        out[key] = (z, prev, sgn, cat)
    return out


def oracle_step_from(ref, y, setup, pot, dt, steps=1):
    """the oracle from state y with the mirrored trackers installed, `steps` steps on"""
    r = oracle_from(ref, y)
    for key, (_, prev, sgn, _) in setup.items():
        install_predecessor(r, key, prev, sgn)
    for _ in range(steps):
        r.step(pot, dt)
    return r


# ---------------------------------------------------------------------------------------------------- two-step pair
# off-diagonal noise of the pair rows: small enough that no intermediate in-block pivot is weak (sc_hk_step_multi cannot
# repair those), the rotation angles still spread the phases
PAIR_NOISE = 0.05


def pair_setup(ref, y, pot, dt, seed):
    """sc_hk_step_multi: the predecessor of the FIRST step is mirrored (flip or not), the second step flips or not by itself.
    Returns (z1, z2, prev, sgn, flip1, flip2)"""
    gen = torch.Generator().manual_seed(seed)
    z1, z2 = determinants_after(ref, y, pot, dt, steps=2)["prefactorC"]
    prev, sgn, cat = mirror(z1, gen)
    for z in (z1, z2, prev):
        assert_margin(z)
    flip1, flip2 = would_flip(prev, z1), would_flip(z1, z2)
    return z1, z2, prev, sgn, flip1, flip2


def pair_counts(flip1, flip2):
    return {"intermediate only": int((flip1 & ~flip2).sum()), "final only": int((~flip1 & flip2).sum()),
            "both": int((flip1 & flip2).sum()), "neither": int((~flip1 & ~flip2).sum())}


# ---------------------------------------------------------------------------------------------------- weak last sub-step
def prefactor_matrix(ref):
    """(n, d', d') prefactor matrix of the oracle's current state (oracle/sc_oracle.py HKOracle._prefactor before the det)"""
    Mqq, Mqp, Mpq, Mpp = (X.type(orc.C128) for X in ref.monodromy_matrices())
    mat = 0.5 * (torch.einsum('ai,ijn,jb->abn', ref.sqGt, Mqq, ref.isqGi)
                 + torch.einsum('ai,ijn,jb->abn', ref.isqGt, Mpp, ref.sqGi)
                 - 1j * orc.hbar * torch.einsum('ai,ijn,jb->abn', ref.sqGt, Mqp, ref.sqGi)
                 + 1j / orc.hbar * torch.einsum('ai,ijn,jb->abn', ref.isqGt, Mpq, ref.isqGi))
    return torch.einsum('ia,ijn,jb->abn', ref.U, mat, ref.U).permute(2, 0, 1)


def weak_last_blocks(ref, pot, dt, row, col, seed, outside=0.005):
    """Blocks for which the SECOND of two steps meets a weak in-block pivot in row `row` and the first does not.

    Separable potential, diagonal widths (U = the identity up to signs): row i of every block evolves by one linear map per
    mode, column by column, so the prefactor-matrix entry (i, i) after two steps is a complex linear functional of the four
    initial entries (Mqq, Mqp, Mpq, Mpp)[i, i] alone.  Those are put in the (real, two-dimensional) null space of that
    functional: entry (i, i) is ~1e-16 after the second step and as large as the null space allows after the first (a mode
    with a large omega dt separates the two).  Row i also gets entries of size `outside` in column `col` of another 16-column
    block (the outside candidate that makes the second in-block pivot weak, but not the first), and row `col` O(0.3) entries
    in column i, so that the determinant stays far from zero.  Every other row is diagonal with random entries."""
    D, n = ref.dim, ref.ntraj
    gen = torch.Generator().manual_seed(seed)
    assert torch.allclose(ref.U.real.abs(), torch.eye(D, dtype=torch.float64)), "needs U = identity up to signs"
    blocks = diagonal_blocks(D, n, gen, torch.diagonal(ref.Gamma_i))
    signed = lambda lo, hi: ((lo + (hi - lo) * torch.rand(n, generator=gen, dtype=torch.float64))
                             * torch.where(torch.rand(n, generator=gen, dtype=torch.float64) < 0.5, -1.0, 1.0))
    for b in blocks:
        b[row, col] = signed(outside, 2 * outside)
        b[col, row] = signed(0.3, 0.6)
        b[row, row] = 0.0
    # the functionals: entry (i, i) after one and after two steps for unit initial entries (the probes differ in (i, i) only)
    F1, F2 = torch.zeros(n, 4, dtype=orc.C128), torch.zeros(n, 4, dtype=orc.C128)
    for k in range(4):
        probe = [b.clone() for b in blocks]
        probe[k][row, row] = 1.0
        r = oracle_from(ref, with_blocks(ref.y, D, probe))
        r.step(pot, dt)
        F1[:, k] = prefactor_matrix(r)[:, row, row]
        r.step(pot, dt)
        F2[:, k] = prefactor_matrix(r)[:, row, row]
    real2 = lambda F: torch.stack((F.real, F.imag), dim=1)                 # (n, 2, 4)
    null = torch.linalg.svd(real2(F2))[2][:, 2:, :]                          # (n, 2, 4): orthonormal basis of the null space
    # within the null space, the unit vector with the largest entry (i, i) after the FIRST step
    g = torch.einsum('nrk,njk->nrj', real2(F1), null)                        # (n, 2, 2)
    c = torch.linalg.svd(g)[2][:, 0, :]
    x = torch.einsum('nj,njk->nk', c, null)
    for k in range(4):
        blocks[k][row, row] = x[:, k]
    return blocks


def weak_last_premise(ref, y, pot, dt, row, col):
    """|mat_ii| relative to the row's outside candidate after each of the two steps: (first, second)"""
    r = oracle_from(ref, y)
    ratios = []
    for _ in range(2):
        r.step(pot, dt)
        m = prefactor_matrix(r)
        ratios.append((m[:, row, row].abs() / m[:, row, col].abs()))
    return ratios


# ---------------------------------------------------------------------------------------------------- the one-step rows
def _shift(s):
    return lambda D, n, gen, g: shifted_blocks(D, n, s, gen, g)


def _wm_rerun_blocks(D, n, gen, g):
    """large random momentum blocks (tests/test_wm_gpu.py): the imaginary part of the Filinov matrix dominates its diagonally
    dominant real part, and the fixed pivot order of the WM register kernel meets weak pivots for part of the batch"""
    eye = torch.eye(D, dtype=torch.float64).unsqueeze(2)
    out = [s * ((eye if k in (0, 3) else 0.0) + 0.5 * torch.randn(D, D, n, generator=gen, dtype=torch.float64))
           for k, s in enumerate((1.0, 1.0, 30.0, 30.0))]
    # Mqp, Mpq change sign for half of the batch (about the complex conjugate matrices): determinants on both sides of the axis
    half = torch.where(torch.rand(n, generator=gen, dtype=torch.float64) < 0.5, -1.0, 1.0)
    return [out[0], half * out[1], half * out[2], out[3]]


WM_AB = (0.05, 0.05)

# (test id, route, case, blocks, n, options of the GPU helper)
ONE_STEP = [
    # separable fast path (sc_hk_step_sd) and its 0x200 fix-up pass
    ("fast-D17", "fast", lambda: morse_case(17), dense_blocks, 256, {}),
    ("fast-D33", "fast", lambda: morse_case(33), dense_blocks, 256, {}),
    ("fast-D60", "fast", lambda: morse_case(60), dense_blocks, 256, {}),
    ("fast-fixup-D17", "fast-fixup", lambda: morse_case(17), _shift(8), 256, {}),
    ("fast-fixup-D33", "fast-fixup", lambda: morse_case(33), _shift(11), 256, {}),
    ("fast-fixup-D60", "fast-fixup", lambda: morse_case(60), _shift(20), 256, {}),
    # hk_step_w16_kernel, hk_step_sep16_kernel and its fix-up
    ("w16-D13", "w16", lambda: morse_case(13), dense_blocks, 256, {}),
    ("w16-D16", "w16", lambda: morse_case(16), dense_blocks, 256, {}),
    ("sep16-D5", "sep16", lambda: morse_case(5), dense_blocks, 256, {}),
    ("sep16-D12", "sep16", lambda: morse_case(12), dense_blocks, 256, {}),
    ("sep16-fixup-D5", "sep16-fixup", lambda: morse_case(5), _shift(2), 256, {}),
    ("sep16-fixup-D12", "sep16-fixup", lambda: morse_case(12), _shift(4), 256, {}),
    # hk_step_lin_kernel (constant dense Hessian, D <= 16) and its fix-up launch
    ("lin-D6", "lin", lambda: harmonic_case(6), dense_blocks, 256, {}),
    ("lin-D12-dense-widths", "lin", lambda: harmonic_case(12, diag=False, zero_modes=2), dense_blocks, 256, {}),
    ("lin-fixup-D12", "lin-fixup", lambda: harmonic_case(12), _shift(4), 256, {}),
    # general hk_step_kernel: no flag array, widths that are not diagonal
    ("general-noflags-D5", "general", lambda: morse_case(5), dense_blocks, 256, {"without_flags": True}),
    ("general-noflags-dense-D12", "general", lambda: harmonic_case(12), dense_blocks, 256, {"without_flags": True}),
    ("general-widths-D20", "general", lambda: morse_case(20, diag=False), dense_blocks, 256, {}),
    # separable shortcut (sc_hk_step_diag)
    ("diag-D17", "diag", lambda: morse_case(17), diagonal_blocks, 256, {"exploit_separability": True}),
    ("diag-D51", "diag", lambda: morse_case(51), diagonal_blocks, 256, {"exploit_separability": True}),
    ("diag-D64", "diag", lambda: morse_case(64), diagonal_blocks, 256, {"exploit_separability": True}),
    # normal-mode step (sc_hk_step_modal): one step first, so that the mirrored step starts from blocks in normal modes
    ("modal-D17", "modal", lambda: harmonic_case(17), dense_blocks, 256, {"pre_steps": 1}),
    ("modal-D51", "modal", lambda: harmonic_case(51), dense_blocks, 256, {"pre_steps": 1}),
    ("modal-D64", "modal", lambda: harmonic_case(64), dense_blocks, 128, {"pre_steps": 1}),
    ("modal-D51-dense-widths", "modal", lambda: harmonic_case(51, diag=False, zero_modes=6), dense_blocks, 256, {"pre_steps": 1}),
    # dense path: register prefactor of sc_dense_mono, its weak-pivot fallback, sc_dense_any (D > 96)
    ("dense-mono-D40", "dense-mono", lambda: generic_case(40), dense_blocks, 128, {}),
    ("dense-mono-D70", "dense-mono", lambda: generic_case(70), dense_blocks, 128, {}),
    ("dense-mono-fallback-D40", "dense-mono-fallback", lambda: generic_case(40), _shift(20), 128, {}),
    ("dense-mono-fallback-D70", "dense-mono-fallback", lambda: generic_case(70), _shift(20), 128, {}),
    ("dense-any-D100", "dense-any", lambda: generic_case(100), dense_blocks, 96, {}),
    # Walton-Manolopoulos: prefactorC, detA and detM (wm_small up to D = 16, the global-scratch kernel beyond)
    ("wm-D6", "wm", lambda: morse_case(6, wm=WM_AB), dense_blocks, 256, {}),
    ("wm-D12", "wm", lambda: morse_case(12, wm=WM_AB), dense_blocks, 256, {}),
    ("wm-D20", "wm", lambda: morse_case(20, wm=WM_AB), dense_blocks, 256, {}),
    ("wm-D32", "wm", lambda: morse_case(32, wm=WM_AB), dense_blocks, 128, {}),
    # (the large momentum blocks leave the phases of prefactorC and detM near the real axis: the flips are counted for detA)
    ("wm-rerun-D12", "wm-rerun", wm_rerun_case, _wm_rerun_blocks, 768, {"premise_keys": ("detA",)}),
]

# (test id, case, steps, whole loop in normal modes)
WHOLE_LOOP = [
    ("run-sep16-D5", lambda: morse_case(5), 8, False),
    ("run-lin-D6", lambda: harmonic_case(6), 8, False),
    ("run-modal-D6", lambda: harmonic_case(6, diag=False), 16, True),
]

# the weak last sub-step of sc_hk_step_multi: dimension, row, outside column, trajectories, seed, case
WEAK_LAST = (33, 15, 20, 64, 2, lambda: morse_case(33, dt=20.0, width=4.0))


def one_step_setup(make_case, make_blocks, n, seed=1, pre_steps=0, premise_keys=None, **_):
    """host side of a one-step row: oracle, hand-made state (after `pre_steps` plain steps) and mirrored trackers"""
    case = make_case()
    ref = case.oracle(n, seed)
    gen = torch.Generator().manual_seed(seed)
    y = with_blocks(ref.y, case.D, make_blocks(case.D, n, gen, torch.diagonal(case.Gi)))
    ref.y = y.clone()
    for _ in range(pre_steps):
        ref.step(case.oracle_pot, case.dt)
    return case, ref, y, mirrored_setup(ref, ref.y, case.oracle_pot, case.dt, seed, premise_keys=premise_keys)
