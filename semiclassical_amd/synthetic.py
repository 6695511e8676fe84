"""Synthetic inputs for the BASELINE.json configurations the reference ships no data for.

  anharmonic_as_model(60)      config 2 / 4: 60-mode adiabatic-shift model (the reference only has a 5-mode file)
  sgdml_model(30, 200, 30)     config 5: an sGDML model of the shapes of a 30-atom molecule (the reference only has the
                               17-atom coumarin model)
Deterministic (fixed seeds), NumPy only; used by bench.py, tools/ and the tests.
"""
import numpy as np
import torch

from . import units


def anharmonic_as_model(dim=60):
    """omega, chi, nac, q0, dt of the synthetic `dim`-mode AS model: rng(60); omega = linspace(160, 3300) cm^-1;
    S = U(0, 0.1) x (+-1); nac ~ N(0, 1e-4); chi = 0.02; q0 = sign(S) sqrt(2|S|/omega); dt = 0.005 fs"""
    rng = np.random.default_rng(60)
    omega_cm = np.linspace(160.0, 3300.0, dim)
    S = rng.uniform(0, 0.1, dim) * rng.choice([-1, 1], dim)
    nac = rng.normal(0, 1e-4, dim)
    chi = np.full(dim, 0.02)
    omega = torch.from_numpy(omega_cm / units.hartree_to_wavenumbers)
    S, nac, chi = torch.from_numpy(S), torch.from_numpy(nac), torch.from_numpy(chi)
    q0 = torch.sqrt(2.0 * abs(S) / omega) * torch.sign(S)
    dt = 0.005 / units.autime_to_fs
    return omega, chi, nac, q0, dt


def sgdml_model(n_atoms, n_train, seed):
    """model dict (keys of an sGDML .npz: sig, c, std, z, R_desc (Dd, M), R_d_desc_alpha (M, Dd), perms,
    tril_perms_lin) and the geometry pos (n_atoms, 3) it was built around: atoms on a jittered lattice, training
    descriptors = descriptors of perturbed geometries, coefficients scaled like the coumarin model's"""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(n_atoms ** (1 / 3)))
    grid = np.array([(i, j, k) for i in range(side) for j in range(side) for k in range(side)], dtype=float)[:n_atoms]
    pos = 2.6 * grid + rng.normal(0, 0.15, grid.shape)
    k, l = np.tril_indices(n_atoms, -1)
    desc = lambda p: 1.0 / np.linalg.norm(p[k] - p[l], axis=1)
    R_desc = np.stack([desc(pos + rng.normal(0, 0.08, pos.shape)) for _ in range(n_train)], axis=1)      # (Dd, M)
    alpha = rng.normal(0, 2.0e7, (n_train, len(k))) * R_desc.T ** 2
    model = {"sig": np.int64(40), "c": np.float64(-3.2), "std": np.float64(0.07), "z": np.full(n_atoms, 6),
             "R_desc": R_desc, "R_d_desc_alpha": alpha, "perms": np.arange(n_atoms)[None, :],
             "tril_perms_lin": np.arange(len(k))}
    return model, pos


QFF_COUPLING_FRACTION = 0.02


def qff_model(dim, seed=0, fraction=QFF_COUPLING_FRACTION):
    """Arrays of a synthetic `dim`-mode quartic force field and of the wavepacket that starts on it (the keys of the driver's
    "quartic force field" model file, plus dt): rng(seed); omega = linspace(160, 3300) cm^-1, unit masses, pos0 = 0, grad0 = 0,
    H = diag(omega^2); Morse-like diagonals with chi = 0.02: a_i = sqrt(2 omega_i chi), t_iii = -3 a_i omega_i^2,
    u_iiii = 7 a_i^2 omega_i^2; off-diagonal t_ijk, u_iijj, u_iiij = `fraction` x U(-1, 1) x the geometric mean of the diagonal
    constants of the indices involved (|t_iii t_jjj t_kkk|^(1/3), (u_iiii u_jjjj)^(1/2), (u_iiii^3 u_jjjj)^(1/4)); coupling
    ~ N(0, 1e-4); wavepacket as in the AS model: S = U(0, 0.1) x (+-1), q0 = sign(S) sqrt(2|S|/omega), Gamma_0 = diag(omega);
    dt = 4 a.u.

    fraction = 0.02 was picked on the CPU through the oracle (tests/test_qff_host.py::test_synthetic_model_conditions repeats
    it): at D = 6, 17, 40 and 70 the trajectories of the displaced ground-state wavepacket stay bound over 20 steps (energy guard
    silent), and the anharmonic part of V is more than 1 % of V for the median trajectory."""
    import itertools
    rng = np.random.default_rng(seed)
    omega = np.linspace(160.0, 3300.0, dim) / units.hartree_to_wavenumbers
    a = np.sqrt(2.0 * omega * 0.02)
    t_d, u_d = -3.0 * a * omega ** 2, 7.0 * a ** 2 * omega ** 2
    def sym(x):                                      # exactly symmetric: the permuted copies are added in sorted order
        s = np.sort(np.stack([np.transpose(x, p) for p in itertools.permutations(range(x.ndim))]), axis=0)
        return s[0] + (s[1:] - s[0]).sum(axis=0) / len(s)
    c3 = np.cbrt(np.abs(t_d))
    cubic = sym(fraction * rng.uniform(-1, 1, (dim, dim, dim)) * c3[:, None, None] * c3[None, :, None] * c3[None, None, :])
    iijj = sym(fraction * rng.uniform(-1, 1, (dim, dim)) * np.sqrt(u_d[:, None] * u_d[None, :]))
    iiij = fraction * rng.uniform(-1, 1, (dim, dim)) * (u_d[:, None] ** 3 * u_d[None, :]) ** 0.25
    idx = np.arange(dim)
    cubic[idx, idx, idx] = t_d
    iijj[idx, idx] = u_d
    iiij[idx, idx] = 0.0
    S = rng.uniform(0, 0.1, dim) * rng.choice([-1, 1], dim)
    return {"pos0": np.zeros(dim), "energy0": np.float64(0.0), "grad0": np.zeros(dim), "hess0": np.diag(omega ** 2),
            "cubic": cubic, "quartic_iijj": iijj, "quartic_iiij": iiij, "masses": np.ones(dim),
            "coupling": rng.normal(0, 1e-4, dim), "q0": np.sign(S) * np.sqrt(2.0 * np.abs(S) / omega),
            "Gamma_0": np.diag(omega), "zero_point_energy": np.float64(0.5 * omega.sum()), "dt": 4.0}


def qff_potential(model):
    """QuarticForceFieldPotential of the arrays of qff_model()"""
    from .potentials import QuarticForceFieldPotential
    return QuarticForceFieldPotential.from_arrays(
        model["pos0"], model["energy0"], model["grad0"], model["hess0"], cubic=model.get("cubic"),
        quartic_iijj=model.get("quartic_iijj"), quartic_iiij=model.get("quartic_iiij"), masses=model["masses"],
        nac0=model["coupling"], origin=float(model.get("origin", 0.0)))


class ArrayFchk(object):
    """the three accessors MolecularGDMLPotential / MolecularHarmonicPotential take from an fchk object"""

    def __init__(self, masses, nac, atomic_numbers=None):
        self._masses, self._nac, self._z = np.asarray(masses), np.asarray(nac), atomic_numbers

    def masses(self):
        return self._masses

    def nonadiabatic_coupling(self):
        return self._nac

    def atomic_numbers(self):
        return self._z
