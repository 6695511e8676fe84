"""The normal-mode HK step for constant-Hessian molecules of 17 to 64 modes (sc_hk_step_modal, ABI 18) against the CPU oracle:
random SPD Hessians with dense rank-deficient and diagonal widths, coumarin from its fchk files, changes of basis between
potentials, weak pivots, a full-size batch and the widened sc_mono_similarity."""
import os

import numpy as np
import pytest
import torch

from tests import cases

pytestmark = pytest.mark.gpu

TOL = 1e-9
FCHK = os.path.join(cases.GOLDEN, "fchk")


def _random_case(D, zero_modes, diag, seed, masses=None, om_range=(500, 3000)):
    """random SPD Hessian and widths, the construction of tests/test_hk_gpu.py::test_constant_hessian_register_kernel_vs_oracle"""
    rng = np.random.default_rng(seed)
    masses = rng.uniform(1800.0, 22000.0, D) if masses is None else masses
    Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    om = rng.uniform(*om_range, D) / 219474.63
    sm = np.sqrt(masses)
    hess0 = (Q * om ** 2) @ Q.T * np.outer(sm, sm)
    hess0 = 0.5 * (hess0 + hess0.T)
    pos0, grad0 = rng.normal(0, 0.1, D), rng.normal(0, 1e-3, D)
    nac0 = rng.normal(0, 1e-2, D)
    args = (pos0, np.float64(-0.3), grad0, hess0, masses, nac0)
    w = om * rng.uniform(0.7, 1.4, D)
    if diag:
        G = np.diag(w * masses)
    else:
        w[:zero_modes] = 0.0
        U, _ = np.linalg.qr(rng.standard_normal((D, D)))
        G = (U * w) @ U.T * np.outer(sm, sm)
        G = 0.5 * (G + G.T)
    q0 = torch.from_numpy(pos0 + rng.normal(0, 0.05, D))
    return args, torch.from_numpy(G), q0, torch.zeros(D)


def _pair(G, q0, p0, n, seed=3, wm=None):
    from oracle import sc_oracle as orc
    from semiclassical_amd import propagators as PR
    if wm is None:
        ref, prop = orc.HKOracle(G, G), PR.HermanKlukPropagator(G, G, device="cuda")
    else:
        ref, prop = orc.WMOracle(G, G, *wm), PR.WaltonManolopoulosPropagator(G, G, *wm, device="cuda")
    torch.manual_seed(seed)
    ref.initial_conditions(q0, p0, G, ntraj=n)
    prop.set_initial_conditions(q0, p0, G, ref.zi, ref.probi)
    return ref, prop


def _compare_state(prop, ref, tol=1e-11, signs=True):
    for a, b in zip(prop.current_positions_and_momenta() + prop.monodromy_matrices(),
                    ref.current_positions_and_momenta() + ref.monodromy_matrices()):
        assert cases.rel_err(a.cpu(), b) < tol
    assert cases.rel_err(prop.classical_action().cpu(), ref.classical_action()) < tol
    if signs:
        assert np.array_equal(prop._sgn.cpu().numpy(), ref.tracker.signs("prefactorC").real.numpy())


@pytest.mark.parametrize("diag", [False, True])
@pytest.mark.parametrize("D", [17, 24, 33, 34, 48, 51, 63, 64])
def test_modal_step_random_hessian_vs_oracle(D, diag):
    """run() and ten step() calls on the modal kernel against the oracle's Cartesian RK4"""
    from oracle import sc_oracle as orc
    from semiclassical_amd import potentials as P
    torch.set_default_dtype(torch.float64)
    n, nt, dt = 100, 10, 4.0
    args, G, q0, p0 = _random_case(D, 6, diag, 1000 + 10 * D + diag)
    opot = orc.MolecularHarmonicOracle(*args, origin=-0.3)
    pot = P.MolecularHarmonicPotential.from_arrays(*args, origin=-0.3)
    ref, prop = _pair(G, q0, p0, n)
    assert prop._pre.dprime == (D if diag else D - 6) and bool(prop._pre.diag) == diag
    rc, rk = orc.run_loop(ref, opot, dt, nt, 0.01)
    c, k = prop.run(pot, dt, nt, 0.01)
    assert prop._modal_basis is not None, "run() did not take the normal-mode step"
    assert cases.rel_err(c, rc) < TOL and cases.rel_err(k, rk) < TOL
    _compare_state(prop, ref)
    assert prop._modal_basis is None                       # monodromy_matrices() converted back
    assert abs(prop.mean_energy() - float(ref.eom.en_mean)) < 1e-11 * max(1.0, abs(float(ref.eom.en_mean)))
    # the same ten steps one step() at a time
    _, prop2 = _pair(G, q0, p0, n)
    for _ in range(nt):
        prop2.step(pot, dt)
    assert prop2._modal_basis is not None
    assert cases.rel_err(prop2.autocorrelation(0.01), ref.autocorrelation(0.01)) < TOL
    assert cases.rel_err(prop2.ic_correlation(pot, 0.01), ref.ic_correlation(opot, 0.01)) < TOL
    _compare_state(prop2, ref)


def _coumarin():
    from semiclassical_amd import readers, potentials as P
    from oracle import sc_oracle as orc
    fchk = {}
    for name in ("coumarin_s0", "coumarin_s1"):
        with open(os.path.join(FCHK, name + ".fchk")) as fh:
            fchk[name] = readers.FormattedCheckpointFile(fh)
    s0, s1 = fchk["coumarin_s0"], fchk["coumarin_s1"]
    pot = P.MolecularHarmonicPotential(s1, s1)
    opot = orc.MolecularHarmonicOracle(pot.pos0.numpy(), pot.energy0.numpy(), pot.grad0.numpy(), pot.hess0.numpy(),
                                       pot._masses.numpy(), pot.nac0.numpy())
    centre, widths, _ = s0.vibrational_groundstate()
    return pot, opot, torch.from_numpy(centre), torch.from_numpy(widths)


@pytest.mark.parametrize("wm", [None, (100.0, 100.0)])
def test_coumarin_vs_oracle(wm):
    """coumarin (D = 51, d' = 45): MolecularHarmonicPotential(S1, S1), the wavepacket of the S0 ground state; HK 20 steps of 64
    trajectories, WM 10 steps of 32 (the Cartesian coverage kernel refuses this shape for lack of LDS)"""
    from oracle import sc_oracle as orc
    torch.set_default_dtype(torch.float64)
    pot, opot, q0, G = _coumarin()
    n, nt, dt = (64, 20, 10.0) if wm is None else (32, 10, 10.0)
    ref, prop = _pair(G, q0, torch.zeros_like(q0), n, seed=11, wm=wm)
    assert prop.dim == 51 and prop._pre.dprime == 45
    rc, rk = orc.run_loop(ref, opot, dt, nt)
    c, k = prop.run(pot, dt, nt)
    tol = TOL if wm is None else 1e-8
    assert cases.rel_err(c, rc) < tol and cases.rel_err(k, rk) < tol
    _compare_state(prop, ref, 1e-11 if wm is None else 1e-10)


def test_basis_switches_vs_oracle():
    """y read / written between modal steps, a second Hessian, a separable potential (Cartesian sc_hk_step) and back"""
    from oracle import sc_oracle as orc
    from semiclassical_amd import potentials as P
    torch.set_default_dtype(torch.float64)
    D, n, dt = 24, 64, 200.0
    ones = np.ones(D)
    # unit masses and low frequencies: the separable potential below has the same masses and a similar mean energy, so the
    # energy guard sees no jump when the potentials are swapped
    args1, G, q0, p0 = _random_case(D, 0, False, 501, masses=ones, om_range=(20, 60))
    args2, _, _, _ = _random_case(D, 0, False, 502, masses=ones, om_range=(20, 60))
    args1 = (np.zeros(D), np.float64(0.0), np.zeros(D)) + args1[3:]
    args2 = (np.zeros(D), np.float64(0.0), np.zeros(D)) + args2[3:]
    q0 = torch.from_numpy(np.random.default_rng(5).normal(0, 0.5, D))
    rng = np.random.default_rng(503)
    omega = torch.from_numpy(rng.uniform(20, 60, D) / 219474.63)
    nac = torch.from_numpy(rng.normal(0, 1e-3, D))
    pots = {"h1": (P.MolecularHarmonicPotential.from_arrays(*args1), orc.MolecularHarmonicOracle(*args1)),
            "h2": (P.MolecularHarmonicPotential.from_arrays(*args2), orc.MolecularHarmonicOracle(*args2)),
            "sep": (P.MorsePotential(omega, torch.zeros(D), nac), orc.MorseOracle(omega, torch.zeros(D), nac))}
    ref, prop = _pair(G, q0, p0, n)
    for what in ["h1", "h1", "y", "h1", "h2", "h2", "sep", "h1", "h1"]:
        if what == "y":
            y = prop.y
            assert cases.rel_err(y.cpu(), ref.y) < 1e-11
            prop.y = y
            continue
        prop.step(pots[what][0], dt)
        ref.step(pots[what][1], dt)
        assert (prop._modal_basis is not None) == (what != "sep")
    assert cases.rel_err(prop.autocorrelation(), ref.autocorrelation()) < TOL
    assert cases.rel_err(prop.ic_correlation(pots["h1"][0]), ref.ic_correlation(pots["h1"][1])) < TOL
    assert cases.rel_err(prop._c2.cpu(), ref.c2) < TOL
    _compare_state(prop, ref)


@pytest.mark.parametrize("diag", [False, True])
def test_weak_pivot_vs_oracle(diag):
    """blocks whose prefactor matrix has a zero leading pivot (a cyclic shift with a rank-one correction that zeroes P[0, 0] for the
    propagator's own constants): the prefactor of the modal kernel (mode 1, then one step) equals the oracle's pivoted determinant"""
    from oracle import sc_oracle as orc
    from semiclassical_amd import potentials as P, _lib
    from semiclassical_amd._lib import lib, check, ptr
    torch.set_default_dtype(torch.float64)
    D, n, dt = 40, 48, 2.0
    args, G, q0, p0 = _random_case(D, 0, diag, 77 + diag)
    opot = orc.MolecularHarmonicOracle(*args, origin=-0.3)
    pot = P.MolecularHarmonicPotential.from_arrays(*args, origin=-0.3)
    ref, prop = _pair(G, q0, p0, n)
    # Mqq = Mpp = X, Mqp = Mpq = 0: P = 1/2 (L1 X R1 + L2 X R2).  X = cyclic shift + t a b^T with t chosen so that P[0, 0] = 0
    # for these (dense or diagonal) constants; asserted on the host below
    pre = prop._pre
    if pre.diag:
        L1, L2, R1, R2 = np.diag(pre.st.numpy()), np.diag(1 / pre.st.numpy()), np.diag(1 / pre.si.numpy()), np.diag(pre.si.numpy())
    else:
        L1, L2, R1, R2 = (m.real.numpy() for m in (pre.L1, pre.L2, pre.R1, pre.R2))
    S = np.roll(np.eye(D), 1, axis=0)
    rng = np.random.default_rng(9)
    a, b = rng.standard_normal(D), rng.standard_normal(D)
    P0 = lambda X: 0.5 * (L1 @ X @ R1 + L2 @ X @ R2)
    t = -P0(S)[0, 0] / P0(np.outer(a, b))[0, 0]
    X = S + t * np.outer(a, b)
    assert abs(P0(X)[0, 0]) < 1e-13 * np.abs(P0(X)).max()
    shift = torch.from_numpy(X)
    y = ref.y.clone()
    d = D
    for k, blk in enumerate((shift, torch.zeros(D, D), torch.zeros(D, D), shift)):
        y[2 * d + k * d * d: 2 * d + (k + 1) * d * d] = blk.reshape(-1, 1).expand(-1, n)
    ref.y = y.clone()
    prop.y = y.cuda()
    ref._prefactor()
    desc = prop._potential_descriptor(pot, dt)
    modal = prop._modal_step_constants(pot, desc, dt)
    assert modal is not None
    prop._enter_modal(modal)
    check(lib.sc_hk_step_modal(desc, prop._state, modal["hk"], dt, 1, ptr(modal["phi"]), None, prop._stream()))
    assert cases.rel_err(prop._c2.cpu(), ref.c2) < TOL
    prop.step(pot, dt)
    ref.step(opot, dt)
    assert cases.rel_err(prop._c2.cpu(), ref.c2) < TOL
    _compare_state(prop, ref, signs=False)        # (mode 1 restarted the engine's tracker, the oracle's kept tracking)
    assert _lib.SC_POT_HARMONIC_DENSE == desc.kind


def test_full_size_coumarin():
    """D = 51, n = 1e5, 3 steps: 64 sampled trajectories against the oracle run on their initial points"""
    from oracle import sc_oracle as orc
    from semiclassical_amd import propagators as PR
    torch.set_default_dtype(torch.float64)
    pot, opot, q0, G = _coumarin()
    p0 = torch.zeros_like(q0)
    n, nt, dt = 100_000, 3, 10.0
    prop = PR.HermanKlukPropagator(G, G, device="cuda")
    torch.manual_seed(21)
    zi, probi = prop.draw_initial_conditions(q0, p0, G, n)
    prop.set_initial_conditions(q0, p0, G, zi, probi)
    for _ in range(nt):
        prop.step(pot, dt)
    assert prop._modal_basis is not None
    pick = torch.from_numpy(np.random.default_rng(4).choice(n, 64, replace=False))
    ref = orc.HKOracle(G, G)
    ref.set_initial_conditions(q0, p0, G, zi[:, pick].clone(), probi[pick].clone())
    for _ in range(nt):
        ref.step(opot, dt)
    qp = prop.current_positions_and_momenta()
    for a, b in zip(qp + prop.monodromy_matrices(), ref.current_positions_and_momenta() + ref.monodromy_matrices()):
        assert cases.rel_err(a[..., pick.cuda()].cpu(), b) < 1e-11
    assert cases.rel_err(prop._c2[pick.cuda()].cpu(), ref.c2) < TOL
    assert np.array_equal(prop._sgn[pick.cuda()].cpu().numpy(), ref.tracker.signs("prefactorC").real.numpy())


@pytest.mark.parametrize("D", [17, 33, 64])
def test_mono_similarity_wide(D):
    """sc_mono_similarity for 16 < D <= 64 against a host product"""
    from semiclassical_amd import _lib
    from semiclassical_amd._lib import lib, check, ptr, sc_state
    rng = np.random.default_rng(D)
    n = 37
    mono = torch.from_numpy(rng.standard_normal((n, 4, D, D))).cuda()
    left = torch.from_numpy(rng.standard_normal((4, D, D))).cuda()
    right = torch.from_numpy(rng.standard_normal((4, D, D))).cuda()
    want = np.einsum("pik,npkl,plj->npij", left.cpu().numpy(), mono.cpu().numpy(), right.cpu().numpy())
    st = sc_state(n=n, dim=D, mono_layout=_lib.SC_MONO_ROWMAJOR, mono=ptr(mono))
    check(lib.sc_mono_similarity(st, ptr(left), ptr(right), None))
    torch.cuda.synchronize()
    assert cases.rel_err(mono.cpu().numpy(), want) < 1e-13


def test_run_with_graph_flag_takes_plain_loop():
    """run(use_graph=True) on the modal path gives the numbers of run() and of the oracle"""
    from oracle import sc_oracle as orc
    from semiclassical_amd import potentials as P
    torch.set_default_dtype(torch.float64)
    D, n, nt, dt = 33, 80, 8, 4.0
    args, G, q0, p0 = _random_case(D, 6, False, 4242)
    opot = orc.MolecularHarmonicOracle(*args, origin=-0.3)
    pot = P.MolecularHarmonicPotential.from_arrays(*args, origin=-0.3)
    ref, prop = _pair(G, q0, p0, n)
    _, plain = _pair(G, q0, p0, n)
    rc, rk = orc.run_loop(ref, opot, dt, nt, 0.01)
    c, k = prop.run(pot, dt, nt, 0.01, use_graph=True)
    c2, k2 = plain.run(pot, dt, nt, 0.01)
    assert prop._modal_basis is not None and getattr(prop, "_graph", None) is None
    assert np.array_equal(c, c2) and np.array_equal(k, k2)
    assert cases.rel_err(c, rc) < TOL and cases.rel_err(k, rk) < TOL
    _compare_state(prop, ref)


@pytest.mark.parametrize("name,tol", [("hk_coumarin_harmonic", 1e-9), ("wm_coumarin_harmonic", 1e-8)])
def test_coumarin_matches_reference_golden(name, tol):
    """the reference's own HK / WM run on coumarin (tests/golden/make_golden_harmonic.py) through run() on the modal path"""
    from tests.engine_cases import engine_potential
    from semiclassical_amd import propagators as PR
    torch.set_default_dtype(torch.float64)
    g = cases.load(name)
    Gi, Gt = cases.T(g["Gamma_i"]), cases.T(g["Gamma_t"])
    prop = (PR.WaltonManolopoulosPropagator(Gi, Gt, float(g["alpha"]), float(g["beta"]), device="cuda") if "alpha" in g
            else PR.HermanKlukPropagator(Gi, Gt, device="cuda"))
    prop.set_initial_conditions(cases.T(g["q0"]), cases.T(g["p0"]), cases.T(g["Gamma_0"]), cases.T(g["zi"]), cases.T(g["probi"]))
    pot = engine_potential(g)
    c, k = prop.run(pot, float(g["dt"]), int(g["nt"]), float(g["E0"]))
    assert "alpha" in g or prop._modal_basis is not None
    assert cases.rel_err(c, g["cauto"]) < tol and cases.rel_err(k, g["kic"]) < tol
    assert cases.rel_err(prop._c2.cpu().numpy(), g["c2"][-1]) < tol
    d, nb = prop.dim, g["mono_final"].shape[-1]
    y = prop.y.cpu().numpy()
    assert cases.rel_err(np.vstack((y[:2 * d], y[-1:])), g["qpS_final"]) < 10 * tol
    assert cases.rel_err(y[2 * d:2 * d + 4 * d * d, :nb].reshape(4, d, d, nb), g["mono_final"]) < 10 * tol
    assert np.array_equal(prop._sgn.cpu().numpy(), g["signs_final"].real)
    if "alpha" in g:
        assert np.array_equal(prop._sgnA.cpu().numpy(), g["signsA_final"].real)
        assert np.array_equal(prop._sgnM.cpu().numpy(), g["signsM_final"].real)


def test_coumarin_harmonic_task_matches_reference_driver(tmp_path, monkeypatch):
    """the product driver on a "harmonic" task with the coumarin fchk files (D = 51: the modal step) + the rates task, against the
    npz the reference's driver wrote for the same sampled initial conditions (tests/golden/driver_coumarin_harmonic.npz)"""
    import json
    from semiclassical_amd import driver, propagators as PR
    g = cases.load("driver_coumarin_harmonic")
    assert str(g["outcome"]) == "ok"
    task = json.loads(str(g["task"]))
    out = tmp_path / "correlations.npz"
    task["potential"] = {"type": "harmonic", "ground": os.path.join(FCHK, "coumarin_s0.fchk"),
                         "excited": os.path.join(FCHK, "coumarin_s1.fchk"), "coupling": os.path.join(FCHK, "coumarin_s1.fchk")}
    task["results"] = {"correlations": str(out)}
    count = {"rep": 0}

    def from_golden(self, q0, p0, Gamma_0, ntraj=5000, **kwargs):
        rep = count["rep"]
        count["rep"] += 1
        assert g["zi"][rep].shape[1] == ntraj
        self.set_initial_conditions(q0, p0, Gamma_0, cases.T(g["zi"][rep]), cases.T(g["probi"][rep]))
    monkeypatch.setattr(PR.HermanKlukPropagator, "initial_conditions", from_golden)
    modal_steps = {"n": 0}
    orig = PR.HermanKlukPropagator._enter_modal

    def counting(self, modal):
        modal_steps["n"] += 1
        return orig(self, modal)
    monkeypatch.setattr(PR.HermanKlukPropagator, "_enter_modal", counting)
    driver.run_semiclassical_dynamics(task, device="cuda")
    assert count["rep"] == 2 and modal_steps["n"] > 0
    driver.calculate_rates(dict(json.loads(str(g["rates_task"])), correlations=str(out), rates=str(out)))
    got = dict(np.load(out))
    ref = {k[4:]: v for k, v in g.items() if k.startswith("res_")}
    assert set(got) == set(ref), set(got) ^ set(ref)
    assert str(got["propagator"]) == "HK" and int(got["trajectories"]) == int(ref["trajectories"]) == 32
    assert np.array_equal(got["times"], ref["times"]) and np.array_equal(got["energies"], ref["energies"])
    assert abs(float(got["zero_point_energy"]) - float(ref["zero_point_energy"])) < 1e-12
    assert abs(float(got["adiabatic_gap"]) - float(ref["adiabatic_gap"])) < 1e-10
    for key in ("autocorrelation", "ic_correlation", "ic_rate"):
        assert cases.rel_err(got[key], ref[key]) < 1e-12, key
