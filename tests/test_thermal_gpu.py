"""Thermal ensembles on the device (sc_thermal.hip): the kernels against the host restatement of
tests/thermal_cases.py, the zero-temperature limit against today's path, the clock of the mid states of pairs and visits, the
device sampler, the sums after the kernel, every refusal and the driver key."""
import numpy as np
import pytest
import torch

from oracle import sc_oracle as orc
from tests import cases, thermal_cases as tcs

pytestmark = pytest.mark.gpu
torch.set_default_dtype(torch.float64)

TOL = 1e-9          # x max |.|: the project's tolerance for terms and sums over trajectories against the host


def _golden_case(name, kT, n=None, seed=1):
    """engine and oracle objects of a golden fixture with a thermal ensemble drawn on the host (the fixture's widths, q0, masses,
    potential; fresh samples: the fixture's zi belong to the centre (q0, p0))"""
    from semiclassical_amd import propagators as PR
    from tests.engine_cases import engine_potential
    g = cases.load(name)
    pot, opot = engine_potential(g), cases.oracle_potential(g)
    Gi, Gt, G0, q0 = (cases.T(g[k]) for k in ("Gamma_i", "Gamma_t", "Gamma_0", "q0"))
    masses = opot.masses().to(torch.float64)
    n = int(g["zi"].shape[1]) if n is None else n
    tc, centres, zi, probi = tcs.draw_samples(Gi, G0, masses, q0, kT, n, seed)
    prop = PR.HermanKlukPropagator(Gi, Gt, device="cuda")
    prop.set_thermal_initial_conditions(q0, torch.zeros_like(q0), G0, masses, kT, centres, zi, probi)
    ref = orc.HKOracle(Gi, Gt)
    ref.set_initial_conditions(q0, torch.zeros_like(q0), G0, zi, probi)
    return g, pot, opot, prop, ref, tc, centres


def _synthetic_case(D, n, seed):
    from semiclassical_amd import potentials as P, propagators as PR
    m = tcs.synthetic_dense(D, seed)
    ref, opot, tc, centres = tcs.model_objects(m, m["kT"], n, seed)
    pot = P.MolecularHarmonicPotential.from_arrays(m["pos_gs"], 0.0, np.zeros(D), m["hess_gs"], m["masses"], m["nac"], origin=0.0)
    G0, q0 = cases.T(m["Gamma_0"]), cases.T(m["q0"])
    prop = PR.HermanKlukPropagator(G0, G0, device="cuda")
    prop.set_thermal_initial_conditions(q0, torch.zeros_like(q0), G0, cases.T(m["masses"]), m["kT"], centres, ref.zi, ref.probi)
    return {"dt": 8.0, "E0": m["E0"]}, pot, opot, prop, ref, tc, centres


CASES = {
    "D1": lambda: _golden_case("hk_1d", 0.8, n=67),
    "D5_diag": lambda: _golden_case("hk_as5_chi002", 0.006, n=257),
    "D6_dense": lambda: _synthetic_case(6, 67, 3),
    "D12_methylium": lambda: _golden_case("hk_methylium", 0.004, n=67),
    "D17_dense": lambda: _synthetic_case(17, 67, 4),
    "D65_dense": lambda: _synthetic_case(65, 257, 5),
}


@pytest.mark.parametrize("case", list(CASES))
def test_terms_and_sums_match_restatement(case):
    """per-trajectory terms (autocorrelation_qp, the exported k terms), C and k over four steps, deviation / largest value"""
    g, pot, opot, prop, ref, tc, centres = CASES[case]()
    dt, E0 = float(g["dt"]), float(g["E0"])
    assert tc.diag == (case in ("D1", "D5_diag")) and (tc.dmodes < tc.dim) == (case == "D12_methylium")
    assert torch.equal(prop.thermal_centres.cpu(), centres)
    worst = {}
    for step in range(4):
        cq, kq = tcs.thermal_terms(ref, tc, centres, ref.t, opot)
        phase = np.exp(1j * ref.t * E0)
        C, K = prop.autocorrelation(E0), prop.ic_correlation(pot, E0)
        qp = prop.autocorrelation_qp().cpu()
        got_k = prop._kq.cpu()
        pairs = {"C": (C, complex(cq.sum()) * phase), "k": (K, complex(kq.sum()) * phase),
                 "qp": (qp, cq * ref._mc_weight()), "kq": (got_k, kq)}
        for key, (got, want) in pairs.items():
            scale = float(abs(torch.as_tensor(want)).max())
            dev = float(abs(torch.as_tensor(got) - torch.as_tensor(want)).max()) / scale
            worst[key] = max(worst.get(key, 0.0), dev)
        prop.step(pot, dt)
        ref.step(opot, dt)
    print(f"{case}: D = {tc.dim}, d'' = {tc.dmodes}, n = {prop.ntraj}: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert all(v <= TOL for v in worst.values()), worst


@pytest.mark.parametrize("name", ["hk_as5_chi002", "hk_methylium"])
def test_zero_temperature_is_todays_path(name):
    from semiclassical_amd import hostmath, propagators as PR
    from tests.engine_cases import engine_potential, engine_propagator
    g = cases.load(name)
    pot, prop0 = engine_potential(g), engine_propagator(g)
    nt, dt, E0 = 6, float(g["dt"]), float(g["E0"])
    C0, K0 = prop0.run(pot, dt, nt, E0)
    masses = cases.oracle_potential(g).masses().to(torch.float64)
    tc_modes = hostmath.ThermalConstants(cases.T(g["Gamma_0"]), masses, 0.0).dmodes
    prop = PR.HermanKlukPropagator(cases.T(g["Gamma_i"]), cases.T(g["Gamma_t"]), device="cuda")
    prop.set_thermal_initial_conditions(cases.T(g["q0"]), cases.T(g["p0"]), cases.T(g["Gamma_0"]), masses, 0.0,
                                        torch.zeros((g["zi"].shape[1], 2 * tc_modes)), cases.T(g["zi"]), cases.T(g["probi"]))
    C, K = prop.run(engine_potential(g), dt, nt, E0)
    dc, dk = abs(C - C0).max() / abs(C0).max(), abs(K - K0).max() / abs(K0).max()
    print(f"{name}: T = 0 against the zero-temperature path: C {dc:.1e}, k {dk:.1e}")
    assert dc <= 1e-12 and dk <= 1e-12
    # ... and the way back: initial conditions without a temperature leave the thermal path
    prop.set_initial_conditions(cases.T(g["q0"]), cases.T(g["p0"]), cases.T(g["Gamma_0"]), cases.T(g["zi"]), cases.T(g["probi"]))
    assert prop.thermal_centres is None
    C1, K1 = prop.run(engine_potential(g), dt, nt, E0)
    assert np.array_equal(C1, C0) and np.array_equal(K1, K0)


def test_routes_agree_on_the_state_time():
    """D = 60 (hk_as60 constants, n = 96): run() in pairs, in visits of three, one launch per step, and a step() loop.  The states
    are the same bit for bit; a mid state correlated with the clock of the visit's start would be off by the rotation of a step."""
    nt = 7
    out = {}
    for route in ("pairs", "visits", "single", "steps"):
        g, pot, opot, prop, ref, tc, centres = _golden_case("hk_as60_n96", 0.005)
        dt, E0 = float(g["dt"]), float(g["E0"])
        prop.pair_steps = route in ("pairs", "visits")
        if route == "visits":
            prop.visit_min_bytes = 0
        if route == "steps":
            C, K = np.zeros(nt, dtype=complex), np.zeros(nt, dtype=complex)
            for k in range(nt):
                C[k], K[k] = prop.autocorrelation(E0), prop.ic_correlation(pot, E0)
                prop.step(pot, dt)
        else:
            C, K = prop.run(pot, dt, nt, E0)
        out[route] = (C, K)
    C0, K0 = out["steps"]
    assert abs(C0).min() > 0
    for route in ("pairs", "visits", "single"):
        dc, dk = abs(out[route][0] - C0).max() / abs(C0).max(), abs(out[route][1] - K0).max() / abs(K0).max()
        print(f"{route} against the step() loop: C {dc:.1e}, k {dk:.1e}")
        assert dc <= 1e-13 and dk <= 1e-13
    # the rotation of one step is visible at this tolerance: the test can see a wrong clock
    g, pot, opot, prop, ref, tc, centres = _golden_case("hk_as60_n96", 0.005)
    a = tcs.thermal_terms(ref, tc, centres, 0.0)[0].sum()
    b = tcs.thermal_terms(ref, tc, centres, float(g["dt"]))[0].sum()
    assert abs(a - b) > 1e-6 * abs(a)


def _device_drawn(seed, n, first=0, kT=0.9, **kw):
    from semiclassical_amd import propagators as PR
    omega, masses = torch.tensor([0.5, 1.0, 2.2]), torch.tensor([1.0, 3.0, 0.5])
    G0 = torch.diag(omega * masses)
    prop = PR.HermanKlukPropagator(G0, G0, device="cuda")
    q0 = torch.tensor([0.2, -0.1, 0.4])
    if kT is None:
        prop.initial_conditions(q0, torch.zeros(3), G0, ntraj=n, seed=seed, first_index=first, **kw)
    else:
        prop.thermal_initial_conditions(q0, torch.zeros(3), G0, masses, kT, ntraj=n, seed=seed, first_index=first, **kw)
    return prop, omega, masses, q0


def test_device_sampler():
    n = 2 ** 16
    prop, omega, masses, q0 = _device_drawn(7, n)
    cold, _, _, _ = _device_drawn(7, n, kT=None)
    # the xi are those of sc_sample_initial: the same densities bit for bit, the same displacements from the centre
    assert torch.equal(prop.probi, cold.probi)
    tc = prop._thermal["consts"]
    a, b = tc.cartesian(prop.thermal_centres)
    centre = torch.cat((q0.unsqueeze(0) + a, b), 1).T.to(prop.device)
    z0 = torch.cat((q0, torch.zeros(3))).unsqueeze(1).to(prop.device)
    assert float(abs((prop.zi - centre) - (cold.zi - z0)).max()) <= 1e-13 * float(abs(cold.zi).max())
    # centre variances: hbar nbar / omega and hbar nbar omega, within 4 / sqrt(n) relative
    nbar = 1.0 / np.expm1(omega.numpy() / 0.9)
    want = np.concatenate((nbar / omega.numpy(), nbar * omega.numpy()))
    got = (prop.thermal_centres ** 2).mean(0).cpu().numpy()
    print("centre variances / expected - 1:", np.array2string(got / want - 1.0, precision=4), "bound", 4.0 / np.sqrt(n))
    assert abs(got / want - 1.0).max() <= 4.0 / np.sqrt(n)
    # split invariance over first_index, and another subsequence is another ensemble
    whole, _, _, _ = _device_drawn(3, 100)
    left, _, _, _ = _device_drawn(3, 37)
    right, _, _, _ = _device_drawn(3, 63, first=37)
    for name in ("thermal_centres", "_zi_t", "probi"):
        assert torch.equal(getattr(whole, name), torch.cat((getattr(left, name), getattr(right, name))))
    other, _, _, _ = _device_drawn(3, 100, subsequence=1)
    assert not torch.equal(other.thermal_centres, whole.thermal_centres)
    # a device-drawn ensemble starts normalised: C_T(0) = 1
    assert abs(whole.autocorrelation() - 1.0) < 1e-12


def test_sums_after_the_kernel():
    """standard errors, blocks and the discard mask: the sums of the exported terms, recomputed in torch"""
    from semiclassical_amd import hostmath
    g, pot, opot, prop, ref, tc, centres = _golden_case("hk_as5_chi002", 0.006, n=203)
    dt, E0, dev, n = float(g["dt"]), float(g["E0"]), prop.device, prop.ntraj
    prop.run(pot, dt, 3, E0)
    for masked in (False, True):
        if masked:
            eps = prop.symplectic_deviation()
            prop.discard_nonsymplectic(float(eps.median()))
            assert 0 < prop.kept_count() < n
        slots, moments, blocks = torch.zeros((1, 5), device=dev), torch.zeros((1, 6), device=dev), torch.zeros((1, 4, 4), device=dev)
        prop.run(pot, dt, 1, E0, slots=slots, moments=moments, blocks=blocks)
        prop.synchronize()
        keep = prop.kept.cpu().numpy()
        cq, kq = (np.where(keep, t.cpu().numpy(), 0.0) for t in (prop._cq, prop._kq))
        want_slot = np.array([cq.real.sum(), cq.imag.sum(), kq.real.sum(), kq.imag.sum()])
        want_mom = np.array([(cq.real ** 2).sum(), (cq.imag ** 2).sum(), (cq.real * cq.imag).sum(),
                             (kq.real ** 2).sum(), (kq.imag ** 2).sum(), (kq.real * kq.imag).sum()])
        block = hostmath.error_block(np.arange(n), 4)
        want_blocks = np.array([[x[block == b].sum() for x in (cq.real, cq.imag, kq.real, kq.imag)] for b in range(4)])
        # every sum against the sum of the magnitudes of ITS terms (n eps = 2e-14 of it is the rounding of any order of summation)
        mag = np.array([abs(cq).sum(), abs(cq).sum(), abs(kq).sum(), abs(kq).sum()])
        mag2 = np.repeat([(abs(cq) ** 2).sum(), (abs(kq) ** 2).sum()], 3)
        assert mag.min() > 0
        for got, want, scale in ((slots[0, :4], want_slot, mag), (moments[0], want_mom, mag2), (blocks[0], want_blocks, mag[None, :])):
            assert (abs(got.cpu().numpy() - want) <= 1e-12 * scale).all()
    # standard_errors=True returns the errors of these moments
    g, pot, opot, prop, ref, tc, centres = _golden_case("hk_as5_chi002", 0.006, n=203)
    C, K, sC, sK = prop.run(pot, dt, 2, E0, standard_errors=True)
    _, _, _, _, wC, wK = tcs.run_restatement(ref, opot, tc, centres, dt, 2, E0)
    # (ddof = 1 on both sides; t = 0 has no spread at all for Gamma_i = Gamma_0: compare the second step)
    assert abs(sC[1] - wC[1]) <= 1e-6 * abs(wC[1]) and abs(sK[1] - wK[1]) <= 1e-6 * abs(wK[1])
    sc1, sk1 = prop.standard_errors(E0)
    assert np.isfinite([sc1.real, sk1.real]).all()


def test_refusals():
    from semiclassical_amd import potentials as P, propagators as PR
    from tests.engine_cases import engine_propagator
    g, pot, opot, prop, ref, tc, centres = _golden_case("hk_as5_chi002", 0.006, n=64)
    dt, D = float(g["dt"]), prop.dim
    with pytest.raises(ValueError, match="use_graph"):
        prop.run(pot, dt, 4, use_graph=True)
    ok = np.zeros((2, D))
    with pytest.raises(NotImplementedError, match="thermal"):
        prop.run(pot, dt, 2, targets=(ok, ok))
    with pytest.raises(NotImplementedError, match="thermal"):
        prop.run(pot, dt, 2, operators=(np.ones(1), np.ones((1, D))))
    with pytest.raises(NotImplementedError, match="thermal"):
        prop.cross_correlation(ok, ok)
    with pytest.raises(NotImplementedError, match="thermal"):
        prop.operator_correlation((np.ones(1), np.ones((1, D))))
    with pytest.raises(NotImplementedError, match="thermal"):
        prop.time_average(np.linspace(0.0, 0.1, 4), dt)
    cold = engine_propagator(g)
    acc = cold.time_average(np.linspace(0.0, 0.1, 4), dt)
    with pytest.raises(NotImplementedError, match="thermal"):
        prop.run(pot, dt, 2, time_average=acc)
    for call in (prop.norm, lambda: prop.wavefunction(np.zeros((D, 3))), lambda: prop.reduced_density(0, np.linspace(-1, 1, 5))):
        with pytest.raises(NotImplementedError, match="thermal"):
            call()

    class Varying(P.MorsePotential):
        def derivative_coupling_1st(self, r):
            return super().derivative_coupling_1st(r) * (1.0 + r)
    with pytest.raises(NotImplementedError, match="position-dependent"):
        prop.ic_correlation(Varying(cases.T(g["omega"]), cases.T(g["chi"]), cases.T(g["nac"])))
    assert prop.t == 0.0                                        # none of the refused calls took a step
    # the whole-loop kernel is not refused: D = 5 takes the step loop silently
    C, K = prop.run(pot, dt, 2, float(g["E0"]))
    assert abs(C[0] - 1.0) < 1e-12
    masses = torch.ones(D)
    args = (cases.T(g["q0"]), torch.zeros(D), cases.T(g["Gamma_0"]))
    for bad in (dict(p0=torch.full((D,), 0.1)), dict(temperature=-1.0), dict(masses=torch.ones(D + 1))):
        kw = dict(q0=args[0], p0=args[1], Gamma_0=args[2], masses=masses, temperature=0.006)
        kw.update(bad)
        with pytest.raises(ValueError):
            prop.thermal_initial_conditions(**kw, ntraj=16, seed=1)
    with pytest.raises(ValueError, match="centres"):
        prop.set_thermal_initial_conditions(*args, masses, 0.006, torch.zeros((64, 3)), ref.zi, ref.probi)
    wm = PR.WaltonManolopoulosPropagator(cases.T(g["Gamma_i"]), cases.T(g["Gamma_t"]), 100.0, 100.0, device="cuda")
    with pytest.raises(NotImplementedError):
        wm.thermal_initial_conditions(*args, masses, 0.006, ntraj=16, seed=1)
    with pytest.raises(NotImplementedError):
        wm.set_thermal_initial_conditions(*args, masses, 0.006, centres, ref.zi, ref.probi)


def test_library_bounds():
    """D <= 512 and n <= 64 * 65535: SC_ERR_UNSUPPORTED beyond, before anything is launched"""
    import ctypes as C
    from semiclassical_amd import _lib
    one = torch.zeros(8, device="cuda")
    p = _lib.ptr(one)
    for D, n in ((513, 4), (4, 64 * 65535 + 1)):
        th = _lib.sc_thermal_consts(dim=D, dmodes=D, diag=1, omega=p, map_q=p, map_p=p, q0=p, n1=None, centres=p)
        oc = _lib.sc_overlap_consts(dim=D, diag=1, A=p, B=p, C=p, qk=p, pk=p, fac=1.0)
        st = _lib.sc_state(n=n, dim=D, qp=p, act=p, mono=p, c2=p, sgn=p)
        assert _lib.lib.sc_hk_thermal_initial(th, oc, None, p, n, p, None, None) == -2
        assert _lib.lib.sc_hk_correlate_thermal(st, 0.0, oc, None, th, p, p, None, 1.0, p, None, p, None) == -2
    th = _lib.sc_thermal_consts(dim=4, dmodes=4, diag=1, omega=p, map_q=p, map_p=p, q0=p, n1=None, centres=None)
    assert _lib.lib.sc_hk_thermal_initial(th, oc, None, p, 4, p, None, None) == -1


def test_driver_temperature_key(tmp_path):
    from semiclassical_amd import driver, hostmath, propagators as PR, units
    g = cases.load("hk_as5_chi002")
    model = tmp_path / "AS_model.dat"
    np.savetxt(model, np.vstack((g["omega"] * 219474.63, 0.5 * g["omega"] * g["q0"] ** 2 * np.sign(g["q0"]), g["nac"], np.full(5, 0.02))).T)
    out = tmp_path / "correlations.npz"
    n, nt, kelvin = 300, 4, 1500.0
    task = {"task": "dynamics", "potential": {"type": "anharmonic AS", "model_file": str(model)}, "propagator": "HK",
            "batch_size": n, "num_trajectories": n, "num_steps": nt, "time_step_fs": 0.04, "results": {"correlations": str(out)},
            "manual_seed": 4, "sampling": "host", "temperature": kelvin}
    driver.run_semiclassical_dynamics(task, device="cuda")
    d = np.load(out)
    assert float(d["temperature"]) == kelvin and int(d["trajectories"]) == n
    # the same draw on the host: the xi of initial_conditions, then the centres
    setup = driver.build_problem(task)
    kT = units.kelvin_to_hartree * kelvin
    masses = setup.potential.masses()
    tc = hostmath.ThermalConstants(setup.Gamma_0, masses, kT)
    _, _, iLz, detLz, dprime = hostmath.sampling_matrices(setup.Gamma_0, setup.Gamma_0)
    torch.manual_seed(4)
    zi, probi = PR.HermanKlukPropagator._draw_on_host(torch.zeros(10), iLz, detLz / (2 * np.pi) ** 5, dprime, n)
    centres = tc.draw_centres(n)
    a, b = tc.cartesian(centres)
    zi = zi + torch.cat((setup.q0.unsqueeze(0) + a, b), 1).T
    ref = orc.HKOracle(setup.Gamma_0, setup.Gamma_0)
    ref.set_initial_conditions(setup.q0, setup.p0, setup.Gamma_0, zi, probi)
    opot = orc.MorseOracle(g["omega"], np.full(5, 0.02), g["nac"])
    dt = 0.04 / units.autime_to_fs
    C, K, *_ = tcs.run_restatement(ref, opot, tc, centres, dt, nt, setup.zero_point_energy)
    assert abs(d["autocorrelation"] - C).max() <= TOL * abs(C).max() and abs(d["ic_correlation"] - K).max() <= TOL * abs(K).max()
    # pooling into a file of another temperature, or of none, is refused before any trajectory runs
    more = dict(task, results={"correlations": str(out), "overwrite": False})
    more.pop("manual_seed")
    for other in (dict(more, temperature=300.0), {k: v for k, v in more.items() if k != "temperature"}):
        with pytest.raises(driver.ConfigurationError, match="temperature"):
            driver.run_semiclassical_dynamics(other, device="cuda")
    assert int(np.load(out)["trajectories"]) == n
    driver.run_semiclassical_dynamics(more, device="cuda")
    assert int(np.load(out)["trajectories"]) == 2 * n
    # without the key the file has exactly the keys it had
    plain = tmp_path / "plain.npz"
    cold = {k: v for k, v in task.items() if k != "temperature"}
    cold["results"] = {"correlations": str(plain)}
    driver.run_semiclassical_dynamics(cold, device="cuda")
    assert set(np.load(plain).keys()) == {"propagator", "times", "autocorrelation", "ic_correlation", "adiabatic_gap",
                                          "zero_point_energy", "trajectories"}
    with pytest.raises(driver.ConfigurationError, match="WM"):
        driver.run_semiclassical_dynamics(dict(task, propagator="WM"), device="cuda")
