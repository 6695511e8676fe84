"""Quartic force field (sc_qff_eval / sc_qff_stage): the kernel through the C-ABI against the np.longdouble
restatement of the folded forms (tests/qff_cases.py), then through the propagators against the CPU oracle driving the class's own
torch code, the golden of the reference's propagator, the generic route, the harmonic surface, run()'s extras, a 1-D spectrum and
the driver."""
import numpy as np
import pytest
import torch

from tests import cases, qff_cases as qc, timeavg_cases as ta
from tests.lib_spy import LibSpy

pytestmark = pytest.mark.gpu
torch.set_default_dtype(torch.float64)


# ------------------------------------------------------------------------------------------- 1. the kernel through the C-ABI

DIMS = (1, 2, 3, 4, 5, 15, 16, 17, 33, 60, 64, 65, 96)


def gpu_eval(pot, r):
    """E [n], grad [n][D], hess [n][D][D] of sc_qff_eval at r [n][D], as numpy (outputs pre-filled with NaN)"""
    from semiclassical_amd._lib import lib, check, ptr
    rt = torch.from_numpy(np.array(r, dtype=np.float64, order="C")).to("cuda")
    n, D = rt.shape
    e, g, h = (torch.full(s, np.nan, device="cuda") for s in ((n,), (n, D), (n, D, D)))
    check(lib.sc_qff_eval(pot._qff_model("cuda"), ptr(rt), n, ptr(e), ptr(g), ptr(h), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return e.cpu().numpy(), g.cpu().numpy(), h.cpu().numpy()


@pytest.mark.parametrize("parts", qc.PARTS)
@pytest.mark.parametrize("D", DIMS)
def test_eval_against_the_long_double_restatement(D, parts):
    """every entry of E, grad, hess within gamma(D) x (sum of the absolute values of its terms) of the np.longdouble evaluation, at
    the tile edges of the n axis; symmetric, repeatable and independent of n, of the index and of the neighbours, bit for bit"""
    from semiclassical_amd._lib import lib
    TB = int(lib.sc_qff_tile())
    nmax = 2 * TB + 2
    c, r, ref, mag = qc.case(D, parts, nmax)
    # the float64 numpy evaluation of the same forms has to meet the bound first (on the CPU)
    host, _ = qc.evaluate(c, r, dtype=np.float64)
    assert all(qc.within_bound(a, b, m, D) <= 1.0 for a, b, m in zip(host, ref, mag))
    pot = qc.potential(c)
    full = gpu_eval(pot, r)
    worst = [qc.within_bound(a, b, m, D) for a, b, m in zip(full, ref, mag)]
    print(f"D={D} {parts}: largest error / bound  E {worst[0]:.3f}  grad {worst[1]:.3f}  hess {worst[2]:.3f}")
    assert all(np.isfinite(a).all() for a in full) and max(worst) <= 1.0, worst
    assert np.array_equal(full[2], full[2].transpose(0, 2, 1))
    again = gpu_eval(pot, r)
    assert all(np.array_equal(a, b) for a, b in zip(full, again))
    for n in (1, TB - 1, TB, TB + 1):
        part = gpu_eval(pot, r[:n])
        assert all(np.array_equal(a, b[:n]) for a, b in zip(part, full)), n
    # the same geometry alone, first and last in a batch
    twice = np.array(r)
    twice[-1] = r[0]
    out = gpu_eval(pot, twice)
    assert all(np.array_equal(a[0], a[-1]) and np.array_equal(a[0], b[0]) for a, b in zip(out, full))
    # a NaN geometry changes no other trajectory
    bad = np.array(r)
    bad[TB // 2] = np.nan
    out = gpu_eval(pot, bad)
    keep = np.arange(nmax) != TB // 2
    assert all(np.array_equal(a[keep], b[keep]) for a, b in zip(out, full)) and np.isnan(out[0][TB // 2])


# ------------------------------------------------------------------------------------------- 2. through the propagators

class Hidden(object):
    """the potential protocol of a QuarticForceFieldPotential and nothing else: takes the generic route (its own torch code)"""

    def __init__(self, pot):
        self._pot = pot
        self.dimensions, self.masses, self.harmonic_approximation = pot.dimensions, pot.masses, pot.harmonic_approximation
        self.derivative_coupling_1st, self.derivative_coupling_2nd = pot.derivative_coupling_1st, pot.derivative_coupling_2nd


def _model_pair(D, n, kind="HK", model=None, cls=None):
    """(model arrays, engine potential, oracle with its initial conditions drawn, engine propagator on the same ones)"""
    from oracle import sc_oracle as orc
    from semiclassical_amd import propagators as PR, synthetic
    m = synthetic.qff_model(D, 0) if model is None else model
    pot = synthetic.qff_potential(m)
    if cls is not None:
        pot.__class__ = cls
    G, q0 = torch.from_numpy(m["Gamma_0"]), torch.from_numpy(m["q0"])
    if kind == "HK":
        ref, prop = orc.HKOracle(G, G), PR.HermanKlukPropagator(G, G, device="cuda")
    else:
        ref, prop = orc.WMOracle(G, G, 80.0, 80.0), PR.WaltonManolopoulosPropagator(G, G, 80.0, 80.0, device="cuda")
    torch.manual_seed(2)
    ref.initial_conditions(q0, 0.0 * q0, G, ntraj=n)
    prop.set_initial_conditions(q0, 0.0 * q0, G, ref.zi, ref.probi)
    return m, pot, ref, prop


def _against_oracle(D, n, nt, kind, monkeypatch, tol=1e-9):
    from oracle import sc_oracle as orc
    m, pot, ref, prop = _model_pair(D, n, kind)
    E0 = float(m["zero_point_energy"])
    rc, rk = orc.run_loop(ref, pot, m["dt"], nt, E0)
    spy = LibSpy(monkeypatch, names=("sc_qff_stage", "sc_stage_point"))
    c, k = prop.run(pot, m["dt"], nt, E0)
    monkeypatch.undo()
    errs = cases.rel_err(c, rc), cases.rel_err(k, rk), cases.rel_err(prop.y.cpu().numpy(), ref.y.numpy())
    print(f"{kind} D={D} n={n} nt={nt}: C {errs[0]:.2e}  k {errs[1]:.2e}  y {errs[2]:.2e}  |C[-1] - C[0]| {abs(rc[-1] - rc[0]):.2e}")
    assert np.abs(rc[-1] - rc[0]) > 1e-3                     # the dynamics is not trivial
    assert max(errs) < tol, errs
    return spy.seen


@pytest.mark.parametrize("kind,D,n,nt", [("HK", 5, 96, 6), ("HK", 17, 96, 6), ("HK", 40, 96, 6), ("WM", 5, 96, 10), ("HK", 70, 24, 3)])
def test_matches_oracle(kind, D, n, nt, monkeypatch):
    seen = _against_oracle(D, n, nt, kind, monkeypatch)
    assert seen == {"sc_qff_stage": 4 * nt}, seen


def test_golden_of_the_reference_propagator():
    """tests/golden/make_golden_qff.py: the reference's own HermanKlukPropagator on this class's torch code"""
    from semiclassical_amd import propagators as PR, synthetic
    g = cases.load("hk_qff6")
    m = synthetic.qff_model(6, int(g["seed"]))
    pot = synthetic.qff_potential(m)
    G, q0 = torch.from_numpy(m["Gamma_0"]), torch.from_numpy(m["q0"])
    prop = PR.HermanKlukPropagator(G, G, device="cuda")
    prop.set_initial_conditions(q0, 0.0 * q0, G, cases.T(g["zi"]), cases.T(g["probi"]))
    c, k = prop.run(pot, float(g["dt"]), int(g["nt"]), float(g["E0"]))
    errs = cases.rel_err(c, g["C"]), cases.rel_err(k, g["k"]), cases.rel_err(prop.y.cpu().numpy(), g["y"])
    print(f"hk_qff6: C {errs[0]:.2e}  k {errs[1]:.2e}  y {errs[2]:.2e}")
    assert max(errs) < 1e-9, errs


def test_routes(monkeypatch):
    """D = 40 takes sc_qff_stage and never the potential's torch code; D = 100, beyond sc_qff_max_dim(), takes the generic route
    (C, k to 1e-8 there, the tolerance of tests/test_generic_potential_gpu.py for the any-dimension kernels beyond D = 96)"""
    from oracle import sc_oracle as orc
    from semiclassical_amd import potentials as P

    class Raising(P.QuarticForceFieldPotential):
        def harmonic_approximation(self, r):
            raise AssertionError("the fused route evaluates the potential in sc_qff_stage")

    m, pot, ref, prop = _model_pair(40, 32, cls=Raising)
    spy = LibSpy(monkeypatch, names=("sc_qff_stage", "sc_stage_point", "sc_dense_mono_step"))
    prop.run(pot, m["dt"], 3, float(m["zero_point_energy"]))
    monkeypatch.undo()
    assert spy.seen == {"sc_qff_stage": 12, "sc_dense_mono_step": 3}, spy.seen
    m, pot, ref, prop = _model_pair(100, 10)
    E0, nt = float(m["zero_point_energy"]), 3
    rc, rk = orc.run_loop(ref, pot, m["dt"], nt, E0)
    spy = LibSpy(monkeypatch, names=("sc_qff_stage", "sc_stage_point"))
    c, k = prop.run(pot, m["dt"], nt, E0)
    monkeypatch.undo()
    assert spy.seen == {"sc_stage_point": 4 * nt}, spy.seen
    errs = cases.rel_err(c, rc), cases.rel_err(k, rk), cases.rel_err(prop.y.cpu().numpy(), ref.y.numpy())
    print(f"D=100, generic route: C {errs[0]:.2e}  k {errs[1]:.2e}  y {errs[2]:.2e}")
    assert errs[0] < 1e-8 and errs[1] < 1e-8 and errs[2] < 1e-9, errs


def test_two_routes_agree(monkeypatch):
    m, pot, _, fused = _model_pair(17, 96)
    _, _, _, generic = _model_pair(17, 96)
    E0, nt = float(m["zero_point_energy"]), 6
    c, k = fused.run(pot, m["dt"], nt, E0)
    spy = LibSpy(monkeypatch, names=("sc_qff_stage", "sc_stage_point"))
    c2, k2 = generic.run(Hidden(pot), m["dt"], nt, E0)
    monkeypatch.undo()
    assert spy.seen == {"sc_stage_point": 4 * nt}, spy.seen
    errs = cases.rel_err(c, c2), cases.rel_err(k, k2), cases.rel_err(fused.y.cpu().numpy(), generic.y.cpu().numpy())
    print(f"D=17, sc_qff_stage against the generic route: C {errs[0]:.2e}  k {errs[1]:.2e}  y {errs[2]:.2e}")
    assert max(errs) < 1e-11, errs


def test_harmonic_limit():
    """no cubic and no quartic constants: the surface of MolecularHarmonicPotential, through run()"""
    from semiclassical_amd import potentials as P, synthetic
    m = dict(synthetic.qff_model(24, 0), cubic=None, quartic_iijj=None, quartic_iiij=None)
    rng = np.random.default_rng(24)
    Q, _ = np.linalg.qr(rng.standard_normal((24, 24)))
    m["hess0"] = qc.symmetrise(Q @ m["hess0"] @ Q.T)            # a dense Hessian
    m["grad0"] = rng.normal(0, 1e-5, 24)
    _, pot, _, prop = _model_pair(24, 96, model=m)
    _, _, _, twin = _model_pair(24, 96, model=m)
    harmonic = P.MolecularHarmonicPotential.from_arrays(m["pos0"], m["energy0"], m["grad0"], m["hess0"], m["masses"], m["coupling"])
    E0, nt = float(m["zero_point_energy"]), 6
    c, k = prop.run(pot, m["dt"], nt, E0)
    c2, k2 = twin.run(harmonic, m["dt"], nt, E0)
    errs = cases.rel_err(c, c2), cases.rel_err(k, k2), cases.rel_err(prop.y.cpu().numpy(), twin.y.cpu().numpy())
    print(f"D=24 harmonic limit: C {errs[0]:.2e}  k {errs[1]:.2e}  y {errs[2]:.2e}")
    assert abs(c2[-1] - c2[0]) > 1e-3 and max(errs) < 1e-9, errs


def test_run_with_every_extra(monkeypatch):
    """run() with a time-average accumulator, operators, targets, blocks and standard errors on the quartic force field: every
    extra output is its stand-alone method's in a step-by-step loop (to 1e-12 of the largest entry, the rule of DESIGN.md sections
    4.13-4.17 for a route without a bit promise), and C, k, y are those of a run() without the extras, bit for bit"""
    from tests.test_cross_gpu import _targets
    from tests.test_opquad_gpu import _operators
    D, n, nt = 17, 96, 5
    m, pot, ref, prop = _model_pair(D, n)
    dt, E0 = m["dt"], float(m["zero_point_energy"])
    g = {"q0": m["q0"], "p0": 0.0 * m["q0"]}
    zi = ref.zi.numpy()
    Q, Pt = _targets(g, zi[:D], zi[D:], 3, np.random.default_rng(nt))
    bra, ket = _operators(prop, np.random.default_rng(nt))
    energies = E0 * (1.0 + 0.5 * np.linspace(-1.0, 1.0, 7))
    acc = prop.time_average(energies, dt, references=(Q[:2], Pt[:2]))
    blocks = torch.zeros((nt, 4, 4), device=prop.device)
    spy = LibSpy(monkeypatch, names=("sc_qff_stage", "sc_hk_cross", "sc_hk_opquad", "sc_hk_ta_terms"))
    C, k, sC, sk, T, sT, X, sX = prop.run(pot, dt, nt, E0, standard_errors=True, blocks=blocks, targets=(Q, Pt), operators=(bra, ket),
                                          time_average=acc)
    monkeypatch.undo()
    assert spy.seen == {"sc_qff_stage": 4 * nt, "sc_hk_cross": nt, "sc_hk_opquad": nt, "sc_hk_ta_terms": nt}, spy.seen
    I, sigma = acc.spectrum(standard_errors=True)
    # without the extras
    _, _, _, twin = _model_pair(D, n)
    C2, k2, sC2, sk2 = twin.run(pot, dt, nt, E0, standard_errors=True)
    assert all(np.array_equal(a, b) for a, b in ((C, C2), (k, k2), (sC, sC2), (sk, sk2)))
    assert torch.equal(prop.y, twin.y) and torch.equal(prop._c2, twin._c2) and torch.equal(prop._sgn, twin._sgn) and prop.t == twin.t
    # step by step
    _, _, _, loop = _model_pair(D, n)
    acc2 = loop.time_average(energies, dt, references=(Q[:2], Pt[:2]))
    want = {"C": [], "T": [], "sT": [], "X": [], "sX": []}
    for _ in range(nt):
        want["C"].append(loop.autocorrelation(E0))
        t_, st_ = loop.cross_correlation(Q, Pt, energy0_es=E0, standard_errors=True)
        x_, sx_ = loop.operator_correlation(bra, ket, energy0_es=E0, standard_errors=True)
        want["T"].append(t_), want["sT"].append(st_), want["X"].append(x_), want["sX"].append(sx_)
        acc2.add()
        loop.step(pot, dt)
    I2, sigma2 = acc2.spectrum(standard_errors=True)
    close = lambda a, b: abs(np.asarray(a) - np.asarray(b)).max() <= 1e-12 * abs(np.asarray(b)).max()
    assert close(C, want["C"]) and close(T, want["T"]) and close(sT, want["sT"]) and close(X, want["X"]) and close(sX, want["sX"])
    assert close(I, I2) and close(sigma, sigma2) and (I > 0).all()
    # the blocks add up to the slot rows of C and k (no dynamical phase in either)
    _, _, _, raw = _model_pair(D, n)
    slots, blocks3 = torch.zeros((nt, 5), device=prop.device), torch.zeros((nt, 4, 4), device=prop.device)
    raw.run(pot, dt, nt, E0, slots=slots, blocks=blocks3)
    raw.synchronize()
    assert torch.equal(blocks, blocks3)
    total, rows = blocks3.sum(1).cpu().numpy(), slots[:, :4].cpu().numpy()
    assert abs(total - rows).max() <= 1e-12 * abs(rows).max()


def test_symplecticity_check_and_discard():
    """the check reads the blocks sc_qff_stage + sc_dense_mono_step wrote: against the host's evaluation of
    the read-back state within its rounding bound; a mark at the median deviation (section 4.11) leaves the state alone, and run()
    under the mask gives what the step-by-step loop gives"""
    from tests import symplectic_ref as R
    D, n, nt = 17, 96, 4
    m, pot, _, prop = _model_pair(D, n)
    _, _, _, plain = _model_pair(D, n)
    _, _, _, loop = _model_pair(D, n)
    dt, E0 = m["dt"], float(m["zero_point_energy"])
    for p in (prop, plain, loop):
        for _ in range(3):
            p.step(pot, dt)
    got = prop.symplectic_deviation(per_block=True).cpu().numpy()
    want, bound = R.deviation_and_bound(R.blocks_from_y(prop.y.cpu().numpy(), D), np.sqrt(np.diag(m["Gamma_0"])))
    assert np.all(np.abs(got - want) <= bound) and want.max() > 0.0
    tol = float(torch.median(prop.symplectic_deviation()))
    eps = prop.discard_nonsymplectic(tol).cpu().numpy()
    loop.discard_nonsymplectic(tol)
    assert 0 < prop.kept_count() == int((eps <= tol).sum()) < n
    C, k = prop.run(pot, dt, nt, E0)
    C2, k2 = plain.run(pot, dt, nt, E0)
    assert torch.equal(prop.y, plain.y) and torch.equal(prop._c2, plain._c2) and torch.equal(prop._sgn, plain._sgn)
    assert not np.array_equal(C, C2)
    want_C = []
    for _ in range(nt):
        want_C.append(loop.autocorrelation(E0))
        loop.step(pot, dt)
    assert abs(C - np.array(want_C)).max() <= 1e-12 * abs(C).max()


# ------------------------------------------------------------------------------------------- 3. physics

def _anharmonic_levels(t=-0.75, u=0.4375, nbasis=80):
    """eigenvalues of p^2/2 + x^2/2 + t x^3/6 + u x^4/24 in `nbasis` harmonic-oscillator functions"""
    a = np.diag(np.sqrt(np.arange(1.0, nbasis + 8)), 1)                     # a few more functions, cut after the powers of x
    x = (a + a.T) / np.sqrt(2.0)
    x2 = x @ x
    H = np.diag(np.arange(nbasis + 8) + 0.5) + t * (x2 @ x) / 6.0 + u * (x2 @ x2) / 24.0
    return np.linalg.eigvalsh(H[:nbasis, :nbasis])


def test_spectrum_of_the_one_dimensional_quartic_oscillator():
    """omega = 1, t = -0.75, u_iiii = 0.4375, Gamma = 1, q0 = 1.0, dt = 0.05, ns = 2000, N = 2048 (tests/timeavg_cases.py's sample,
    seed 3), K = 1, energy grid of spacing dE = 2 pi / (4 ns dt).  The peaks of I next to E1 = 1.44958 and E2 = 2.38852 lie within
    1.5 dE of the exact levels and more than 3 dE from the harmonic 1.5 and 2.5.  On the CPU (oracle + restatement): 1.44093 and
    2.38341, that is 0.55 dE and 0.33 dE from exact, 3.8 dE and 7.4 dE from harmonic."""
    from semiclassical_amd import potentials as P, propagators as PR
    from tests.test_timeavg_gpu import _terms_of, _mc_norm
    dt, ns, N, q0 = 0.05, 2000, 2048, 1.0
    levels = _anharmonic_levels()
    E1, E2 = levels[1], levels[2]
    assert abs(E1 - 1.44958) < 1e-5 and abs(E2 - 2.38852) < 1e-5
    dE = 2.0 * np.pi / (4 * ns * dt)
    energies = np.arange(np.floor((E1 - 0.25) / dE), np.ceil((E2 + 0.25) / dE) + 1) * dE
    one = np.ones(1)
    pot = P.QuarticForceFieldPotential.from_arrays(0.0 * one, 0.0, 0.0 * one, np.eye(1), cubic=-0.75 * np.ones((1, 1, 1)),
                                                   quartic_iijj=0.4375 * np.eye(1), masses=one, nac0=0.0 * one)
    q, p, prob = ta.oscillator_sample(N, q0=q0, seed=3)
    G = torch.eye(1)
    prop = PR.HermanKlukPropagator(G, G, device="cuda")
    prop.set_initial_conditions(q0 * torch.ones(1), torch.zeros(1), G, torch.from_numpy(np.vstack((q, p))), torch.from_numpy(prob))
    acc = prop.time_average(energies, dt)
    Q, Pr = np.array([[q0]]), np.array([[0.0]])
    # the first five steps one by one: I of the window so far against the restatement on the read-back state
    rows = []
    for s in range(5):
        rows.append(_terms_of(prop, Q, Pr))
        acc.add()
        prop.step(pot, dt)
    got = acc.spectrum()
    want, _ = ta.restated_spectrum(np.stack(rows), energies, 0.0, dt, _mc_norm(prop), prob, N)
    assert abs(got - want).max() <= 1e-9 * abs(want).max()
    prop.run(pot, dt, ns - 5, time_average=acc)
    I = acc.spectrum()[0]
    for exact, harmonic in ((E1, 1.5), (E2, 2.5)):
        window = np.flatnonzero(abs(energies - exact) <= 0.25)
        peak = energies[window[np.argmax(I[window])]]
        print(f"level {exact:.5f}: peak of I at {peak:.5f}, {abs(peak - exact) / dE:.2f} dE from exact, "
              f"{abs(peak - harmonic) / dE:.2f} dE from harmonic")
        assert abs(peak - exact) <= 1.5 * dE and abs(peak - harmonic) > 3.0 * dE


# ------------------------------------------------------------------------------------------- 4. the driver

def test_driver_task(tmp_path):
    from semiclassical_amd import driver, propagators as PR, synthetic, units
    m = synthetic.qff_model(6, 0)
    model_file, out = tmp_path / "qff6.npz", tmp_path / "correlations.npz"
    np.savez(model_file, **{k: v for k, v in m.items() if k != "dt"})
    nt, fs = 8, 0.1
    task = {"task": "dynamics", "propagator": "HK", "batch_size": 64, "num_trajectories": 128, "num_steps": nt, "time_step_fs": fs,
            "manual_seed": 0, "potential": {"type": "quartic force field", "model_file": str(model_file)},
            "results": {"correlations": str(out)}}
    setup = driver.build_problem(task)
    assert isinstance(setup.potential, type(synthetic.qff_potential(m))) and np.isnan(setup.adiabatic_gap)
    driver.run_semiclassical_dynamics(task, device="cuda")
    d = dict(np.load(out))
    assert int(d["trajectories"]) == 128
    dt = fs / units.autime_to_fs
    runs = []
    for repetition in range(2):
        prop = PR.HermanKlukPropagator(setup.Gamma_0, setup.Gamma_0, device="cuda")
        prop.initial_conditions(setup.q0, setup.p0, setup.Gamma_0, ntraj=64, ntraj_total=64, seed=0, subsequence=repetition)
        runs.append(prop.run(setup.potential, dt, nt, setup.zero_point_energy)[0])
    want = 0.5 * (runs[0] + runs[1])
    dev = abs(d["autocorrelation"] - want).max() / abs(want).max()
    print(f"driver: stored autocorrelation against single run()s {dev:.2e}")
    assert dev <= 1e-12 and abs(want[-1] - want[0]) > 1e-3
