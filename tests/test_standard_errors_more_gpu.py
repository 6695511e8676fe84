"""Standard errors, continued: the second-moment sums against the CPU oracle's per-trajectory terms on the golden fixtures,
the dense / generic / position-dependent-coupling / pivoted-WM routes, two ranks flushing slots and moments in one
collective, and the driver task key."""
import contextlib
import json
import os

import numpy as np
import pytest
import torch

from tests import cases, engine_cases
from tests.lib_spy import LibSpy

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_default_dtype(torch.float64)


def _six(cq, kq):
    out = []
    for t in (cq, kq):
        out += [torch.sum(t.real * t.real, -1), torch.sum(t.imag * t.imag, -1), torch.sum(t.real * t.imag, -1)]
    return torch.stack(out, -1)


def _rel_cols(a, b):
    """largest deviation of each of the six columns, relative to the column's largest entry"""
    a, b = np.asarray(a), np.asarray(b)
    return np.max(np.abs(a - b), axis=0) / np.maximum(np.max(np.abs(b), axis=0), 1e-300)


@contextlib.contextmanager
def _captured_sums():
    """the argument of the LAST torch.sum inside the block: the per-trajectory terms the oracle sums"""
    real, seen = torch.sum, []

    def spy(x, *a, **k):
        seen.append(x)
        return real(x, *a, **k)
    torch.sum = spy
    try:
        yield seen
    finally:
        torch.sum = real


# ------------------------------------------------------------------------------------------------ exactness against the oracle
ORACLE = [("hk_as5_chi002", 1e-9), ("hk_methylium", 1e-9), ("hk_as33", 1e-9), ("wm_as5_chi002", 1e-8), ("wm_methylium", 1e-8),
          ("hk_coumarin_harmonic", 1e-9)]


@pytest.mark.parametrize("name,tol", ORACLE, ids=[r[0] for r in ORACLE])
def test_moments_match_the_oracle_terms(name, tol):
    """the six sums per step restated in numpy from the oracle's per-trajectory terms (autocorrelation_qp / _mc_weight, and the
    k_ic terms of ic_correlation) on the fixture's initial conditions"""
    g = cases.load(name)
    nt = min(6, int(g["nt"]))
    dt = float(g["dt"])
    ref, opot = cases.oracle_propagator(g), cases.oracle_potential(g)
    want = []
    for _ in range(nt):
        with _captured_sums() as seen:
            ref.autocorrelation(0.0)
        cq = seen[-1]
        with _captured_sums() as seen:
            ref.ic_correlation(opot, 0.0)
        kq = seen[-1]
        want.append(_six(cq.detach().cpu(), kq.detach().cpu()).numpy())
        ref.step(opot, dt)
    prop, pot = engine_cases.engine_propagator(g), engine_cases.engine_potential(g)
    slots = torch.zeros((nt, 5), device=prop.device)
    moments = torch.zeros((nt, 6), device=prop.device)
    prop.run(pot, dt, nt, slots=slots, moments=moments)
    prop.synchronize()
    err = _rel_cols(moments.cpu().numpy(), np.array(want))
    assert np.all(err < tol), err


# ------------------------------------------------------------------------------------------------ further routes
def _generic(D, n, nt, dt=1.0):
    """the coupled quartic of tests/branch_cases.py (no device descriptor: dense, position-dependent Hessian), at a step short
    enough that the energy guard stays quiet over nt steps from its wide initial spread"""
    from tests import branch_cases as B
    case = B.generic_case(D)
    ref = case.oracle(n, 3)

    def make():
        from semiclassical_amd import propagators as PR
        prop = PR.HermanKlukPropagator(case.Gi, case.Gi, device="cuda")
        prop.set_initial_conditions(case.q0, case.p0, case.Gi, ref.zi, ref.probi)
        return prop
    return make, case.engine_potential(), dt, nt


def _varying_couplings(n=150, nt=8):
    from semiclassical_amd import potentials as P, propagators as PR
    from tests.test_generic_potential_gpu import _varying_tau1, _varying_tau2
    rng = np.random.default_rng(33)
    D = 5
    omega = torch.from_numpy(np.sort(rng.uniform(700, 2600, D)) / 219474.63)
    nac = torch.from_numpy(rng.normal(0, 1e-3, D))

    class Eng(P.MorsePotential):
        def derivative_coupling_1st(self, r):
            return _varying_tau1(nac, r)

        def derivative_coupling_2nd(self, r):
            return _varying_tau2(nac, r)
    pot = Eng(omega, torch.full((D,), 0.02), nac)
    G = torch.diag(omega)
    q0 = torch.from_numpy(rng.uniform(-6.0, 6.0, D))
    gen = torch.Generator().manual_seed(4)
    probe = PR.HermanKlukPropagator(G, G, device="cuda")
    zi, probi = probe.draw_initial_conditions(q0, torch.zeros(D), G, n, generator=gen)

    def make():
        prop = PR.HermanKlukPropagator(G, G, device="cuda")
        prop.set_initial_conditions(q0, torch.zeros(D), G, zi, probi)
        return prop
    return make, pot, 1.5, nt


def _wm_pivoted(D=12, zero_modes=6, n=400, nt=3):
    """tests/test_wm_gpu.py::test_wm_weak_fixed_order_pivots_are_rerun_with_pivoting: large random momentum blocks make the fixed
    pivot order of the WM register kernel hand part of the batch to the pivoted re-run"""
    from oracle import sc_oracle as orc
    from semiclassical_amd import potentials as P, propagators as PR
    rng = np.random.default_rng(7 + D)
    omega = torch.from_numpy(np.sort(rng.uniform(600, 2500, D)) / 219474.63)
    nac = torch.from_numpy(rng.normal(0, 1e-3, D))
    q0, p0 = torch.from_numpy(rng.normal(0, 1.0, D)), torch.zeros(D)
    Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    w = omega.numpy() * rng.uniform(0.7, 1.4, D)
    w[:zero_modes] = 0.0
    G = torch.from_numpy(Q @ np.diag(w) @ Q.T)
    G = 0.5 * (G + G.T)
    ref = orc.WMOracle(G, G, 0.05, 0.05)
    torch.manual_seed(3)
    ref.initial_conditions(q0, p0, G, ntraj=n)
    gen = torch.Generator().manual_seed(11)
    y = ref.y.clone()
    eye = torch.eye(D).unsqueeze(2)
    for k, scale in enumerate((1.0, 1.0, 30.0, 30.0)):
        blk = scale * ((eye if k in (0, 3) else 0.0) + 0.5 * torch.randn(D, D, n, generator=gen))
        y[2 * D + k * D * D: 2 * D + (k + 1) * D * D] = blk.reshape(D * D, n)

    def make():
        prop = PR.WaltonManolopoulosPropagator(G, G, 0.05, 0.05, device="cuda")
        prop.set_initial_conditions(q0, p0, G, ref.zi, ref.probi)
        prop.y = y.cuda()
        return prop
    return make, P.MorsePotential(omega, torch.zeros(D), nac), 2.0, nt


def _dense_mono_route(prop, seen, flags):
    assert seen.get("sc_dense_mono_step", 0) > 0 and seen.get("sc_stage_consume", 0) > 0 and 16 < prop.dim <= 96


def _dense_any_route(prop, seen, flags):
    assert seen.get("sc_dense_mono_step", 0) > 0 and prop.dim > 96


def _generic_small_route(prop, seen, flags):
    assert seen.get("sc_stage_consume", 0) > 0 and prop.dim <= 16


def _couplings_route(prop, seen, flags):
    assert prop._nac_generic is not None and seen.get("sc_term_moments", 0) > 0


def _wm_rerun_route(prop, seen, flags):
    assert seen.get("sc_term_moments", 0) > 0 and 0 < max(flags) < prop.ntraj, flags


MORE_ROUTES = [
    ("dense-mono-D40", lambda: _generic(40, 128, 4), _dense_mono_route),
    ("dense-any-D100", lambda: _generic(100, 96, 3), _dense_any_route),
    ("generic-potential-D6", lambda: _generic(6, 128, 8), _generic_small_route),
    ("generic-couplings", _varying_couplings, _couplings_route),
    ("wm-pivoted-rerun", _wm_pivoted, _wm_rerun_route),
]
SPIED = {"sc_dense_mono_step", "sc_stage_consume", "sc_term_moments", "sc_hk_correlate_m"}


@pytest.mark.parametrize("name,build,route", MORE_ROUTES, ids=[r[0] for r in MORE_ROUTES])
def test_moments_on_the_remaining_routes(monkeypatch, name, build, route):
    """run() with moments against run() without (C, k bit for bit) and against the six torch sums of the per-trajectory terms the
    same kernels export step by step (1e-12); the route named is asserted"""
    make, pot, dt, nt = build()
    runs = []
    for with_moments in (True, False):
        prop = make()
        slots = torch.zeros((nt, 5), device=prop.device)
        moments = torch.zeros((nt, 6), device=prop.device) if with_moments else None
        prop.run(pot, dt, nt, slots=slots, moments=moments)
        prop.synchronize()
        runs.append((slots.cpu().numpy(), None if moments is None else moments.cpu().numpy()))
    assert np.array_equal(runs[0][0][:, :4], runs[1][0][:, :4]), "C or k changed with moments on"
    prop = make()
    seen = LibSpy(monkeypatch, SPIED).seen
    rows, flags = [], []
    for _ in range(nt):
        prop.ic_correlation(pot)
        mom = torch.zeros(6, device=prop.device)
        slot = torch.zeros(5, device=prop.device)
        prop._launch_correlate(prop._rows.single(slot, mom))
        want = _six(prop._cq, prop._kq).cpu().numpy()
        assert np.all(_rel_cols(mom.cpu().numpy()[None], want[None]) < 1e-12)
        if hasattr(prop, "_wm_flags"):
            flags.append(int(prop._wm_flags[-1].item()))
        rows.append(want)
        prop.step(pot, dt)
    prop.synchronize()
    monkeypatch.undo()
    route(prop, seen, flags or [0])
    assert np.all(_rel_cols(runs[0][1], np.array(rows)) < 1e-12), _rel_cols(runs[0][1], np.array(rows))


# ------------------------------------------------------------------------------------------------ ranks
@pytest.mark.parametrize("case", ["hk_as5_chi002", "wm_methylium"])
def test_two_ranks_flush_slots_and_moments_in_one_collective(case, tmp_path):
    from semiclassical_amd import distributed as D
    g = cases.load(case)
    nt = 10
    out = str(tmp_path / "moments.npz")
    rc = D.launch_local_ranks([os.path.join(ROOT, "tests", "_rank_moments.py"), case, str(nt), out], 2, timeout=600,
                              extra_env={"SC_DIST_BACKEND": "gloo", "SC_TEST_DEVICE": "0"})
    assert rc == 0, f"a rank process failed (largest exit code {rc})"
    r = np.load(out)
    assert int(r["world"]) == 2 and int(r["collectives"]) == 1
    whole, pot = engine_cases.engine_propagator(g), engine_cases.engine_potential(g)
    slots = torch.zeros((nt, 5), device=whole.device)
    moments = torch.zeros((nt, 6), device=whole.device)
    whole.run(pot, float(g["dt"]), nt, float(g["E0"]), slots=slots, moments=moments)
    whole.synchronize()
    assert np.all(_rel_cols(r["slots"][:, :4], slots.cpu().numpy()[:, :4]) < 1e-12)
    assert np.all(_rel_cols(r["moments"], moments.cpu().numpy()) < 1e-12)


def test_rccl_flush_carries_the_moments():
    """flush_correlations(slots, moments, comm=...) through sc_flush_allreduce: one rank, the sums come back unchanged"""
    from semiclassical_amd import distributed as D
    from semiclassical_amd._lib import lib
    assert lib.sc_comm_available() > 0
    dev = torch.device("cuda", 0)
    comm = D.RcclCommunicator(0, 1, dev)
    try:
        slots = torch.rand((16, 5), device=dev)
        moments = torch.rand((16, 6), device=dev)
        s0, m0 = slots.clone(), moments.clone()
        D.flush_correlations(slots, moments, comm=comm)
        torch.cuda.synchronize(dev)
        assert torch.equal(slots, s0) and torch.equal(moments, m0)
    finally:
        comm.destroy()


# ------------------------------------------------------------------------------------------------ driver
def _as5_task(tmp_path, out, **extra):
    g = cases.load("hk_as5_chi002")
    model = tmp_path / "AS_model.dat"
    rows = np.vstack((g["omega"] * 219474.63, 0.5 * g["omega"] * g["q0"] ** 2 * np.sign(g["q0"]), g["nac"],
                      np.full(5, 0.02))).T
    np.savetxt(model, rows)
    task = {"task": "dynamics", "potential": {"type": "anharmonic AS", "model_file": str(model)},
            "propagator": "HK", "batch_size": 400, "num_trajectories": 1200, "num_steps": 20, "time_step_fs": 0.04,
            "results": {"correlations": str(out)}, "manual_seed": 5}
    task.update(extra)
    return task


TODAY = ["propagator", "times", "autocorrelation", "ic_correlation", "adiabatic_gap", "zero_point_energy", "trajectories"]


def test_driver_task_with_standard_errors_matches_one_pooled_batch(tmp_path):
    """"standard_errors": true, 3 batches of 400 device-sampled trajectories: the file's means, second moments and errors
    against ONE engine run over the union of the same trajectories; without the key the file has today's keys"""
    from semiclassical_amd import driver, hostmath, propagators as PR, units
    out = tmp_path / "with.npz"
    task = _as5_task(tmp_path, out, standard_errors=True)
    driver.run_semiclassical_dynamics(task, device="cuda")
    got = dict(np.load(out))
    assert int(got["trajectories"]) == 1200
    setup = driver.build_problem(task)
    zi, probi = [], []
    for rep in range(3):
        p = driver.make_propagator(task, setup.Gamma_0, "cuda")
        p.initial_conditions(setup.q0, setup.p0, setup.Gamma_0, ntraj=400, ntraj_total=400, seed=5, subsequence=rep, first_index=0)
        zi.append(p.zi.cpu())
        probi.append(p.probi.cpu())
    whole = driver.make_propagator(task, setup.Gamma_0, "cuda")
    whole.set_initial_conditions(setup.q0, setup.p0, setup.Gamma_0, torch.cat(zi, 1), torch.cat(probi))
    dt, nt = task["time_step_fs"] / units.autime_to_fs, task["num_steps"]
    slots = torch.zeros((nt, 5), device=whole.device)
    moments = torch.zeros((nt, 6), device=whole.device)
    whole.run(setup.potential, dt, nt, setup.zero_point_energy, slots=slots, moments=moments)
    whole.synchronize()
    C, k, mC, mk = PR.HermanKlukPropagator.phased_moments(slots, moments, 0.0, dt, setup.zero_point_energy)
    assert cases.rel_err(got["autocorrelation"], C) < 1e-12 and cases.rel_err(got["ic_correlation"], k) < 1e-12
    assert np.all(_rel_cols(got["autocorrelation_second_moment"], 1200 * mC) < 1e-12)
    assert np.all(_rel_cols(got["ic_correlation_second_moment"], 1200 * mk) < 1e-12)
    # the errors are differences N S' - mean'^2: compared where the spread is not lost to cancellation (t > 0)
    sC, sk = hostmath.standard_errors(C, mC, 1200), hostmath.standard_errors(k, mk, 1200)
    assert cases.rel_err(got["autocorrelation_error"][1:], sC[1:]) < 1e-9
    assert cases.rel_err(got["ic_correlation_error"], sk) < 1e-9
    # without the key: today's keys only, and the same means
    plain = tmp_path / "plain.npz"
    driver.run_semiclassical_dynamics(_as5_task(tmp_path, plain), device="cuda")
    d = np.load(plain)
    assert sorted(d.files) == sorted(TODAY)
    assert np.array_equal(d["autocorrelation"], got["autocorrelation"]) and np.array_equal(d["ic_correlation"], got["ic_correlation"])
