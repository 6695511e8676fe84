"""sGDML potentials of 49 to 170 atoms on the GPU (the multi-kernel route of sc_gdml_eval / sc_gdml_stage):
E, grad and Hessian against the CPU oracle and against extended precision, HK steps and run() through the stage route,
the refusal beyond 170 atoms."""
import numpy as np
import pytest
import torch

from tests import cases

pytestmark = pytest.mark.gpu


def cnp(t):
    return t.detach().cpu().numpy()


class _Fchk(object):
    def __init__(self, model, nac0=None):
        self.model, n = model, len(model["z"])
        self.nac0 = np.zeros(3 * n) if nac0 is None else nac0

    def nonadiabatic_coupling(self):
        return self.nac0

    def masses(self):
        return np.repeat(np.full(len(self.model["z"]), 12.0 * 1822.888), 3)

    def atomic_numbers(self):
        return self.model["z"]


def _model(N, M, seed, perms=1):
    """synthetic model scaled to molecular forces (max |dE/dr| = 0.02), as tests/test_gdml_gpu.py does; perms = 2 adds the
    permutation that swaps atoms 0 and 1 (the training set is expanded to 2 M rows)"""
    from oracle import sc_oracle as orc
    from semiclassical_amd.synthetic import sgdml_model
    model, pos = sgdml_model(N, M, seed)
    if perms == 2:
        pi = np.arange(N)
        pi[[0, 1]] = [1, 0]
        k, l = np.tril_indices(N, -1)
        index = {(a, b): d for d, (a, b) in enumerate(zip(k, l))}
        sigma = np.array([index[(max(pi[a], pi[b]), min(pi[a], pi[b]))] for a, b in zip(k, l)])
        dd = len(k)
        model["perms"] = np.stack([np.arange(N), pi])
        model["tril_perms_lin"] = np.stack([np.arange(dd), sigma + dd]).T.reshape(-1)
    g0 = orc.GDMLOracle(model).forward(torch.from_numpy(pos.reshape(1, -1)))[1]
    model["R_d_desc_alpha"] = model["R_d_desc_alpha"] * (0.02 / float(g0.abs().max()))
    return model, pos


@pytest.mark.parametrize("N,M,perms", [(49, 37, 1), (52, 22, 1), (64, 45, 1), (65, 18, 1), (97, 23, 1), (128, 10, 1),
                                       (170, 7, 1), (56, 9, 2)])
def test_gdml_large_matches_oracle(N, M, perms):
    """49..170 atoms (partial last chunk of training points, partial last Hessian tile where 3N % 16 != 0, a
    permutation-expanded model): E, grad, Hessian against the CPU oracle"""
    from oracle import sc_oracle as orc
    from semiclassical_amd.gdml import MolecularGDMLPotential
    torch.set_default_dtype(torch.float64)
    model, pos = _model(N, M, 200 + N, perms)
    pot = MolecularGDMLPotential(model, _Fchk(model))
    r = torch.from_numpy(pos.reshape(1, -1) + np.random.default_rng(N).normal(0, 0.05, (3, 3 * N)))
    e_ref, g_ref, h_ref = orc.GDMLOracle(model).forward(r)
    v, grad, hess = pot.harmonic_approximation(r.t().contiguous().cuda())
    h = cnp(hess.permute(2, 0, 1))
    dev = (cases.rel_err(cnp(v), e_ref.numpy()), cases.rel_err(cnp(grad.t()), g_ref.numpy()), cases.rel_err(h, h_ref.numpy()))
    print(f"N={N} M={M} perms={perms}: E {dev[0]:.2e}  grad {dev[1]:.2e}  hess {dev[2]:.2e}")
    assert dev[0] < 1e-11 and dev[1] < 1e-11 and dev[2] < 1e-11
    assert np.array_equal(h, h.transpose(0, 2, 1))


def test_gdml_large_batches_of_geometries():
    """more geometries than one batch of the scratch holds: the first and last geometries against the oracle"""
    from oracle import sc_oracle as orc
    from semiclassical_amd.gdml import MolecularGDMLPotential
    from semiclassical_amd._lib import lib
    torch.set_default_dtype(torch.float64)
    N, M = 49, 37
    model, pos = _model(N, M, 7)
    pot = MolecularGDMLPotential(model, _Fchk(model))
    per_geometry = 8 * (2 * 3 * N + 2 + 2 * M + N * (N - 1) // 2 + 9 * N + 2 * M * 3 * N)
    batch = lib.sc_gdml_scratch_bytes(N, M) // per_geometry
    n = batch + 3
    r = torch.from_numpy(pos.reshape(1, -1) + np.random.default_rng(3).normal(0, 0.05, (n, 3 * N)))
    v, grad, hess = pot.harmonic_approximation(r.t().contiguous().cuda())
    pick = [0, 1, batch - 1, batch, n - 1]
    e_ref, g_ref, h_ref = orc.GDMLOracle(model).forward(r[pick])
    dev = (cases.rel_err(cnp(v)[pick], e_ref.numpy()), cases.rel_err(cnp(grad.t())[pick], g_ref.numpy()),
           cases.rel_err(cnp(hess.permute(2, 0, 1))[pick], h_ref.numpy()))
    print(f"{n} geometries, batches of {batch}: E {dev[0]:.2e}  grad {dev[1]:.2e}  hess {dev[2]:.2e}")
    assert dev[0] < 1e-11 and dev[1] < 1e-11 and dev[2] < 1e-11


def test_gdml_large_against_extended_precision():
    """N = 52: the deviation from the extended-precision evaluation is no worse than 3 x the fp64 oracle's own"""
    from oracle import sc_oracle as orc
    from oracle.gdml_truth import forward_longdouble
    from semiclassical_amd.gdml import MolecularGDMLPotential
    torch.set_default_dtype(torch.float64)
    N, M = 52, 13
    model, pos = _model(N, M, 52)
    pot = MolecularGDMLPotential(model, _Fchk(model))
    r = pos.reshape(1, -1) + np.random.default_rng(11).normal(0, 0.05, (2, 3 * N))
    truth = [np.asarray(t, dtype=np.float64) for t in forward_longdouble(model, r)]
    ref = [cnp(t) for t in orc.GDMLOracle(model).forward(torch.from_numpy(r))]
    v, grad, hess = pot.harmonic_approximation(torch.from_numpy(r).t().contiguous().cuda())
    hip = [cnp(v), cnp(grad.t()), cnp(hess.permute(2, 0, 1))]
    for name, a, b, t in zip(("E", "grad", "hess"), hip, ref, truth):
        dh, do = cases.rel_err(a, t), cases.rel_err(b, t)
        print(f"{name}: HIP vs truth {dh:.2e}, oracle vs truth {do:.2e}")
        assert dh <= 3.0 * do + 1e-15, (name, dh, do)


class _PrefactorReference(object):
    """Reference for c2 = det(prefactor matrix) and for the branch sign of its square root, for the first `check` trajectories:
    the determinant, in extended precision (tests/det_cases.py), of the prefactor matrix formed from the ORACLE's monodromy
    blocks, and the rule of the sqrt tracker (reference propagators.py:1045-1047) applied to the sequence of these values,
    starting from c2 = 1 at t = 0.  Not oracle.c2 and the oracle's tracker: torch.det on the host was seen 1e-6 ... 3e-5 away
    from this reference and, in other processes, with the opposite sign at D = 168 and 300, which also flips signs of the
    oracle's tracker; the kernels stay within 2e-13 of the reference."""

    def __init__(self, width, check=2, history=()):
        self.width, self.check, self.history = width, check, []
        self.prev, self.sgn = np.ones(check, dtype=np.complex128), np.ones(check)
        for c2 in history:
            self._track(c2)

    def _track(self, c2):
        flip = (self.prev.real < 0) & (c2.real < 0) & (self.prev.imag * c2.imag < 0)
        self.sgn = np.where(flip, -self.sgn, self.sgn)
        self.prev = c2
        self.history.append(c2)

    def matches(self, prop, oracle, what):
        """advance the reference to the oracle's current blocks and compare the engine's c2 (1e-8, the tolerance of
        test_more_than_64_dimensions_through_the_dense_path) and sign with it"""
        from tests import det_cases as dc
        n = self.check
        mono = np.stack([b.permute(2, 0, 1)[:n].numpy() for b in oracle.monodromy_matrices()], axis=1)
        s = np.full(mono.shape[-1], np.sqrt(self.width))
        want = np.array([dc.det_longdouble(m) for m in dc.prefactor_diag_numpy(mono, s, s)])
        self._track(want.astype(np.complex128))
        err = dc.rel_err(cnp(prop._c2)[:n], want)
        print(f"{what}: c2 vs extended precision {err.max():.2e}, oracle's c2 vs the same "
              f"{dc.rel_err(oracle.c2.numpy()[:n], want).max():.2e}, signs {self.sgn}")
        assert err.max() < 1e-8, (what, err)
        assert np.array_equal(cnp(prop._sgn)[:n], self.sgn), (what, cnp(prop._sgn), self.sgn)


@pytest.mark.parametrize("N,M", [(56, 30), (100, 14)])
def test_gdml_large_hk_steps_and_run_match_oracle(N, M):
    """D = 168 and D = 300: HK steps through sc_gdml_stage x 4 and the any-dimension monodromy kernels, then run() from
    the initial conditions: q, p, S and the four monodromy blocks against the oracle, the prefactor c2 and the sign of its
    square root against an extended-precision determinant of the oracle's blocks (_PrefactorReference).  C(t) and k_ic(t) are NaN in the oracle itself for these widths: its overlap normalisation forms
    det(Gamma_i + Gamma_0) = 80^D, which overflows a double from D = 162 on (and the sampling density underflows to 0 at
    D = 300); the engine has to return NaN in the same places."""
    from oracle import sc_oracle as orc
    from semiclassical_amd.gdml import MolecularGDMLPotential
    from semiclassical_amd import propagators as PR
    torch.set_default_dtype(torch.float64)
    model, pos = _model(N, M, N)
    masses = np.repeat(np.full(N, 12.0 * 1822.888), 3)
    nac0 = np.random.default_rng(1).normal(0, 1e-3, 3 * N)
    pot = MolecularGDMLPotential(model, _Fchk(model, nac0))
    opot = orc.MolecularGDMLOracle(model, masses, nac0, origin=0.0)
    q0 = torch.from_numpy(pos.reshape(-1))
    G = torch.diag(torch.full((3 * N,), 40.0))
    ntraj, dt, E0 = 8, 5.0, 0.01
    oprop = orc.HKOracle(G, G)
    torch.manual_seed(4)
    oprop.initial_conditions(q0, 0.0 * q0, G, ntraj=ntraj)
    prop = PR.HermanKlukPropagator(G, G, device="cuda")
    prop.set_initial_conditions(q0, 0.0 * q0, G, oprop.zi, oprop.probi)
    pre = _PrefactorReference(40.0)
    for _ in range(2):
        oprop.step(opot, dt)
        prop.step(pot, dt)
        pre.matches(prop, oprop, f"D = {3 * N}, step")
    dy = cases.rel_err(cnp(prop.y), oprop.y.numpy())
    print(f"two HK steps at D = {3 * N}: y {dy:.2e}")
    assert dy < 1e-12
    # run() from the initial conditions (correlation functions, then a step, nt times) leaves the same state
    nt = 3
    ref = orc.HKOracle(G, G)
    torch.manual_seed(4)
    ref.initial_conditions(q0, 0.0 * q0, G, ntraj=ntraj)
    rc, rk = orc.run_loop(ref, opot, dt, nt, E0)
    prop = PR.HermanKlukPropagator(G, G, device="cuda")
    prop.set_initial_conditions(q0, 0.0 * q0, G, ref.zi, ref.probi)
    c, k = prop.run(pot, dt, nt, E0)
    dy = cases.rel_err(cnp(prop.y), ref.y.numpy())
    print(f"run() at D = {3 * N}: y after {nt} steps {dy:.2e}")
    assert dy < 1e-12
    # the first two steps of run() are the two steps above (same initial conditions): the branch rule sees the same c2 history
    _PrefactorReference(40.0, history=pre.history).matches(prop, ref, f"D = {3 * N}, run()")
    c, k = np.asarray(c), np.asarray(k)
    assert np.array_equal(np.isnan(c), np.isnan(rc)) and np.array_equal(np.isnan(k), np.isnan(rk))
    np.testing.assert_allclose(c, rc, rtol=1e-8, atol=0.0, equal_nan=True)
    np.testing.assert_allclose(k, rk, rtol=1e-8, atol=0.0, equal_nan=True)


def test_gdml_refuses_171_atoms():
    import ctypes as C
    from semiclassical_amd.gdml import MolecularGDMLPotential
    from semiclassical_amd._lib import lib, sc_gdml_model
    N = 171
    from semiclassical_amd.synthetic import sgdml_model
    model, _ = sgdml_model(N, 2, 1)
    with pytest.raises(ValueError, match="170"):
        MolecularGDMLPotential(model, _Fchk(model))
    dd = N * (N - 1) // 2
    buf = torch.zeros(2 * dd + 16, dtype=torch.float64, device="cuda")
    idx = torch.zeros(dd, dtype=torch.int32, device="cuda")
    p = C.c_void_p(buf.data_ptr())
    m = sc_gdml_model(n_atoms=N, n_desc=dd, n_train=1, xs_train=p, jx_alphas=p, pair_k=C.c_void_p(idx.data_ptr()),
                      pair_l=C.c_void_p(idx.data_ptr()), q=0.05, c=0.0, std=1.0, origin=0.0, inv_mass=p)
    rc = lib.sc_gdml_eval_scratch(C.byref(m), p, p, 1, p, p, p, None)
    assert rc == -2 and "170" in lib.sc_last_error().decode()
