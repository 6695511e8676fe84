"""Quartic force field on the host: the class's torch code against derivatives of the literally written
Taylor sum, its special cases, the constructor's refusals, minimize(), the ABI, the refusals in front of any launch, the driver's
loader, the golden of the reference's propagator against the oracle, and the conditions the synthetic model promises."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

from tests import cases, qff_cases as qc

torch.set_default_dtype(torch.float64)


def _torch_eval(pot, r):
    """E [n], grad [n][D], hess [n][D][D] of harmonic_approximation at r [n][D], as numpy"""
    V, g, h = pot.harmonic_approximation(torch.from_numpy(np.ascontiguousarray(r.T)))
    return V.numpy(), g.numpy().T, h.numpy().transpose(2, 0, 1)


# ------------------------------------------------------------------------------------------- 1. the surface

@pytest.mark.parametrize("D", [1, 2, 3, 6])
def test_derivatives_of_the_written_out_taylor_sum(D):
    """V, grad, hess of the folded forms against autograd's derivatives of the six sums over the derivative arrays: the factorial
    factors.  Bound: gamma(D) x the sum of the absolute values of the entry's terms; the class's float64 code stays below 0.1 of it
    (measured on the CPU, printed)."""
    c = qc.random_constants(D, 7)
    r = qc.geometries(c, 5, 7)
    pot = qc.potential(c)
    got = _torch_eval(pot, r)
    _, mag = qc.evaluate(c, r)
    f = lambda x: qc.taylor_sum(c, x)
    worst = 0.0
    for b in range(5):
        x = torch.from_numpy(r[b] - c["pos0"])
        want = (f(x).item(), torch.autograd.functional.jacobian(f, x).numpy(), torch.autograd.functional.hessian(f, x).numpy())
        for a, w, m in zip(got, want, mag):
            worst = max(worst, float(np.max(np.abs(a[b] - w) / (qc.gamma(D) * m[b]))))
    print(f"D={D}: largest deviation / bound {worst:.3f}")
    assert worst <= 1.0


def test_long_double_restatement_agrees_with_the_class():
    """the numpy restatement the GPU tests take as their reference is the class's torch code, to the same bound"""
    for D, parts in ((5, "all"), (17, "cubic"), (17, "quartic"), (33, "all")):
        c, r, ref, mag = qc.case(D, parts, 6)
        got = _torch_eval(qc.potential(c), r)
        assert all(qc.within_bound(a, b, m, D) <= 1.0 for a, b, m in zip(got, ref, mag)), (D, parts)


def test_two_mode_identity_with_the_coupled_quartic_potential():
    """t = 0, u_0011 = 4 lam and nothing else: V = 1/2 sum w^2 r^2 + lam (r_0 r_1)^2, the generic potential of
    tests/test_generic_potential_gpu.py"""
    from semiclassical_amd.potentials import QuarticForceFieldPotential
    from tests.test_generic_potential_gpu import CoupledQuarticPotential
    omega, lam = torch.tensor([0.7, 1.3]), 0.37
    masses, nac = torch.ones(2), torch.zeros(2)
    u = np.array([[0.0, 4.0 * lam], [4.0 * lam, 0.0]])
    c = {"pos0": np.zeros(2), "energy0": 0.0, "grad0": np.zeros(2), "hess0": np.diag(omega.numpy() ** 2), "cubic": None,
         "quartic_iijj": u, "quartic_iiij": None}
    pot = QuarticForceFieldPotential.from_arrays(c["pos0"], 0.0, c["grad0"], c["hess0"], cubic=np.zeros((2, 2, 2)), quartic_iijj=u,
                                                 quartic_iiij=np.zeros((2, 2)), masses=masses.numpy(), nac0=nac.numpy())
    r = np.random.default_rng(2).normal(0, 1.5, (9, 2))
    got = _torch_eval(pot, r)
    V, g, h = CoupledQuarticPotential(omega, lam, masses, nac).harmonic_approximation(torch.from_numpy(r.T.copy()))
    want = (V.numpy(), g.numpy().T, h.numpy().transpose(2, 0, 1))
    _, mag = qc.evaluate(c, r)
    assert all(np.all(np.abs(a - b) <= qc.gamma(2) * m) for a, b, m in zip(got, want, mag))


def test_without_anharmonic_constants_it_is_the_harmonic_surface():
    from semiclassical_amd.potentials import MolecularHarmonicPotential
    c = qc.random_constants(7, 3, "none")
    r = qc.geometries(c, 6, 3)
    pot = qc.potential(c, origin=0.25)
    harmonic = MolecularHarmonicPotential.from_arrays(c["pos0"], c["energy0"], c["grad0"], c["hess0"], c["masses"], c["nac0"], origin=0.25)
    for a, b in zip(_torch_eval(pot, r), _torch_eval(harmonic, r)):
        assert np.abs(a - b).max() <= 1e-14 * np.abs(b).max()
    assert pot.total_energy() == harmonic.total_energy() == 0.25 and pot.dimensions() == 7
    rt = torch.from_numpy(r.T.copy())
    assert torch.equal(pot.derivative_coupling_1st(rt), harmonic.derivative_coupling_1st(rt))
    assert torch.equal(pot.derivative_coupling_2nd(rt), harmonic.derivative_coupling_2nd(rt))


def test_constructor_refusals():
    from semiclassical_amd.potentials import QuarticForceFieldPotential as QFF
    c = qc.random_constants(3, 1)
    kw = lambda **over: dict(dict(pos0=c["pos0"], energy0=c["energy0"], grad0=c["grad0"], hess0=c["hess0"], cubic=c["cubic"],
                                  quartic_iijj=c["quartic_iijj"], quartic_iiij=c["quartic_iiij"], masses=c["masses"], nac0=c["nac0"]),
                             **over)
    QFF.from_arrays(**kw())
    def bump(a, idx):
        b = np.array(a)
        b[idx] *= 1.0 + 1e-9
        return b
    for name, shape in (("grad0", (4,)), ("hess0", (3, 4)), ("cubic", (3, 3)), ("quartic_iijj", (2, 2)), ("quartic_iiij", (3,)),
                        ("masses", (2,)), ("nac0", (3, 1))):
        with pytest.raises(ValueError, match=name):
            QFF.from_arrays(**kw(**{name: np.zeros(shape)}))
    for name in ("pos0", "energy0", "grad0", "hess0", "cubic", "quartic_iijj", "quartic_iiij", "masses"):
        bad = np.array(c[name], dtype=float)
        bad[(0,) * bad.ndim] = np.inf
        with pytest.raises(ValueError, match=name):
            QFF.from_arrays(**kw(**{name: bad}))
    for name, idx in (("hess0", (0, 1)), ("cubic", (0, 1, 2)), ("cubic", (0, 0, 1)), ("quartic_iijj", (2, 0))):
        with pytest.raises(ValueError, match=name):
            QFF.from_arrays(**kw(**{name: bump(c[name], idx)}))
    b = np.array(c["quartic_iiij"])
    b[1, 1] = 1e-30
    with pytest.raises(ValueError, match="quartic_iiij"):
        QFF.from_arrays(**kw(quartic_iiij=b))
    # within 1e-12: accepted, and the stored copy is the exact symmetric average
    noise = 1e-14 * np.abs(c["cubic"]).max() * np.random.default_rng(0).normal(size=(3, 3, 3))
    pot = QFF.from_arrays(**kw(cubic=np.array(c["cubic"]) + noise))
    t = pot.cubic.numpy()
    assert all(np.array_equal(t, np.transpose(t, p)) for p in itertools.permutations(range(3)))
    assert np.array_equal(pot.hess0.numpy(), pot.hess0.numpy().T) and np.array_equal(pot.quartic_a.numpy(), pot.quartic_a.numpy().T)


def test_minimize_finds_the_closed_form_minimum():
    """V = g x_0 + 1/2 sum w_i^2 x_i^2 + t/6 x_0^3: the minimum is at x_0 = (-w_0^2 + sqrt(w_0^4 - 2 t g)) / t, x_1 = x_2 = 0"""
    from semiclassical_amd.potentials import QuarticForceFieldPotential as QFF
    w2, g, t = np.array([0.9, 1.7, 2.4]), 0.3, -0.5
    pos0 = np.array([0.4, -1.1, 2.0])
    cubic = np.zeros((3, 3, 3))
    cubic[0, 0, 0] = t
    pot = QFF.from_arrays(pos0, -3.0, np.array([g, 0.0, 0.0]), np.diag(w2), cubic=cubic, masses=np.ones(3), nac0=np.zeros(3))
    x0 = (-w2[0] + np.sqrt(w2[0] ** 2 - 2.0 * t * g)) / t
    emin = -3.0 + g * x0 + 0.5 * w2[0] * x0 ** 2 + t * x0 ** 3 / 6.0
    pot.minimize(torch.from_numpy(pos0 + np.array([0.2, 0.3, -0.2])))
    assert abs(pot.total_energy() - emin) < 1e-12
    V, grad, _ = pot.harmonic_approximation(torch.from_numpy(pos0 + np.array([x0, 0.0, 0.0])).unsqueeze(1))
    assert abs(V.item()) < 1e-12 and grad.abs().max().item() < 1e-12


def test_synthetic_model_conditions():
    """what synthetic.qff_model's docstring says of its coupling fraction, on the oracle itself"""
    from oracle import sc_oracle as orc
    from semiclassical_amd import synthetic
    for D, n in ((6, 64), (17, 48)):
        m = synthetic.qff_model(D, 0)
        pot = synthetic.qff_potential(m)
        G, q0 = torch.from_numpy(m["Gamma_0"]), torch.from_numpy(m["q0"])
        ref = orc.HKOracle(G, G)
        torch.manual_seed(2)
        ref.initial_conditions(q0, 0.0 * q0, G, ntraj=n)
        orc.run_loop(ref, pot, m["dt"], 20, float(m["zero_point_energy"]))       # the energy guard raises if a trajectory leaves
        r = ref.y[:D].real
        V, _, _ = pot.harmonic_approximation(r)
        harmonic = 0.5 * torch.einsum('in,ij,jn->n', r, pot.hess0, r)
        assert ((V - harmonic).abs() / V.abs()).median().item() > 0.01


# ------------------------------------------------------------------------------------------- 2. ABI and refusals

def test_symbols_are_declared_bound_and_exported():
    from semiclassical_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "semiclassical_hip.h")).read()
    for name in ("sc_qff_max_dim", "sc_qff_tile", "sc_qff_scratch_bytes", "sc_qff_eval", "sc_qff_stage"):
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    assert "typedef struct sc_qff_model" in header and _lib.sc_qff_model in _lib.STRUCTS
    assert _lib.lib.sc_struct_size(b"sc_qff_model") == ctypes.sizeof(_lib.sc_qff_model) == 72
    assert int(re.search(r"#define SC_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.ABI_VERSION == _lib.lib.sc_abi_version() == 18
    lib = _lib.lib
    assert lib.sc_qff_max_dim() == 96 and lib.sc_qff_tile() % 16 == 0
    assert lib.sc_qff_scratch_bytes(10, 3) == 8 * (30 + 10 + 30) and lib.sc_qff_scratch_bytes(10, 97) == -1


def test_refusals_in_front_of_any_launch():
    """the arguments are judged before anything is launched: no device is needed (the pointers are never followed)"""
    from semiclassical_amd import _lib
    lib, p = _lib.lib, 4096
    model = lambda **over: _lib.sc_qff_model(**dict(dict(dim=3, pos0=p, grad0=p, hess0=p, cubic=p, quartic_a=p, quartic_b=p,
                                                         energy0=0.0, inv_mass=p), **over))
    ev = lambda m, **kw: lib.sc_qff_eval(m, kw.get("r", p), kw.get("n", 5), kw.get("e", p), kw.get("g", p), kw.get("h", p), None)
    assert ev(None) == -1 and all(ev(model(), **{k: None}) == -1 for k in "regh")
    assert all(ev(model(**{k: None})) == -1 for k in ("pos0", "grad0", "hess0"))
    assert ev(model(dim=0)) == -2 and ev(model(dim=97)) == -2 and "96" in lib.sc_last_error().decode()
    assert ev(model(), n=64 * 65535 + 1) == -2 and str(64 * 65535) in lib.sc_last_error().decode()
    assert ev(model(), n=0) == 0 and ev(model(dim=96), n=0) == 0
    state = lambda n=5, dim=3: _lib.sc_state(n=n, dim=dim, mono_layout=0, qp=p, act=p, mono=p, c2=p, sgn=p, work=None, flags=None)
    dense = _lib.sc_dense_scratch(hess=p, kprev=p, ksum=p, ssum=p)
    st = lambda m, **kw: lib.sc_qff_stage(m, kw.get("scratch", p), kw.get("state", state()), kw.get("dense", dense), 0.1,
                                          kw.get("stage", 0), p, None)
    assert st(None) == -1 and st(model(), scratch=None) == -1 and st(model(), state=None) == -1 and st(model(), dense=None) == -1
    assert st(model(inv_mass=None)) == -1 and st(model(), stage=4) == -1 and st(model(), stage=-1) == -1
    assert st(model(dim=0), state=state(dim=0)) == -2 and st(model(dim=97), state=state(dim=97)) == -2
    assert st(model(), state=state(n=64 * 65535 + 1)) == -2 and st(model(), state=state(dim=4)) == -1
    assert st(model(), state=state(n=0)) == 0


# ------------------------------------------------------------------------------------------- 3. the driver's loader

def test_driver_loader(tmp_path):
    from semiclassical_amd import driver, potentials, synthetic
    m = synthetic.qff_model(4, 1)
    arrays = {k: v for k, v in m.items() if k != "dt"}
    path = tmp_path / "qff4.npz"
    task = {"potential": {"type": "quartic force field", "model_file": str(path)}}
    np.savez(path, **arrays, origin=0.125, p0=0.1 * m["q0"], adiabatic_gap=0.07)
    setup = driver.build_problem(task)
    pot = setup.potential
    assert isinstance(pot, potentials.QuarticForceFieldPotential) and pot.total_energy() == 0.125
    for a, b in ((pot.pos0, m["pos0"]), (pot.hess0, m["hess0"]), (pot.cubic, m["cubic"]), (pot.masses(), m["masses"]),
                 (pot.nac0, m["coupling"]), (setup.q0, m["q0"]), (setup.p0, 0.1 * m["q0"]), (setup.Gamma_0, m["Gamma_0"])):
        assert np.array_equal(a.numpy(), b)
    assert setup.zero_point_energy == float(m["zero_point_energy"]) and setup.adiabatic_gap == 0.07
    r = torch.from_numpy(m["q0"]).unsqueeze(1)
    assert torch.equal(pot.harmonic_approximation(r)[0], synthetic.qff_potential(dict(m, origin=0.125)).harmonic_approximation(r)[0])
    # the optional arrays left out
    np.savez(path, **{k: v for k, v in arrays.items() if k not in ("cubic", "quartic_iijj", "quartic_iiij")})
    setup = driver.build_problem(task)
    assert setup.potential.cubic is None and setup.potential.quartic_a is None and np.isnan(setup.adiabatic_gap)
    assert float(setup.p0.abs().max()) == 0.0 and setup.potential.total_energy() == 0.0
    # missing or mis-shaped arrays: refused before any trajectory runs
    for key in ("pos0", "hess0", "masses", "coupling", "q0", "Gamma_0", "zero_point_energy"):
        np.savez(path, **{k: v for k, v in arrays.items() if k != key})
        with pytest.raises(driver.ConfigurationError, match=key):
            driver.build_problem(task)
    for key, bad in (("q0", np.zeros(5)), ("Gamma_0", np.zeros((4, 3))), ("cubic", np.zeros((4, 4))), ("grad0", np.zeros(3))):
        np.savez(path, **dict(arrays, **{key: bad}))
        with pytest.raises(driver.ConfigurationError, match=key):
            driver.build_problem(task)
    with pytest.raises(driver.ConfigurationError):
        driver.build_problem({"potential": {"type": "quartic force field", "model_file": str(tmp_path / "none.npz")}})


# ------------------------------------------------------------------------------------------- 4. golden

def test_oracle_matches_the_golden_of_the_reference_propagator():
    from oracle import sc_oracle as orc
    from semiclassical_amd import synthetic
    g = cases.load("hk_qff6")
    m = synthetic.qff_model(6, int(g["seed"]))
    pot = synthetic.qff_potential(m)
    G, q0 = torch.from_numpy(m["Gamma_0"]), torch.from_numpy(m["q0"])
    assert float(g["dt"]) == m["dt"] and float(g["E0"]) == float(m["zero_point_energy"])
    ref = orc.HKOracle(G, G)
    ref.set_initial_conditions(q0, 0.0 * q0, G, cases.T(g["zi"]), cases.T(g["probi"]))
    c, k = orc.run_loop(ref, pot, float(g["dt"]), int(g["nt"]), float(g["E0"]))
    errs = cases.rel_err(c, g["C"]), cases.rel_err(k, g["k"]), cases.rel_err(ref.y.numpy(), g["y"])
    print(f"hk_qff6: oracle against the reference  C {errs[0]:.2e}  k {errs[1]:.2e}  y {errs[2]:.2e}")
    assert max(errs) < 1e-12 and g["zi"].shape == (12, 64) and abs(g["C"][-1] - g["C"][0]) > 1e-3
