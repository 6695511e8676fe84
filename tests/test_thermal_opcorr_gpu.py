"""HermanKlukPropagator.thermal_operator_correlation / run(thermal_operators=...) (sc_hk_opcorr_thermal)
against the numpy restatement of tests/thermal_opcorr_cases.py: the tile, chunk and band edges through the C-ABI, the engine on the
thermal models, the zero-temperature limit, the clock of the mid states of pairs and visits, the discard mask, the closed form at
t = 0, every refusal and the driver key."""
import numpy as np
import pytest
import torch

from oracle import sc_oracle as orc
from tests import cases, thermal_cases as tcs, thermal_opcorr_cases as toc
from tests.lib_spy import LibSpy as _Spy
from tests.test_opcorr_gpu import _operators
from tests.test_opcorr_host import restated_rows
from tests.test_thermal_gpu import CASES, _golden_case

pytestmark = pytest.mark.gpu
torch.set_default_dtype(torch.float64)

TOL = 1e-9          # x max |X|: the project's tolerance for a sum over trajectories against the host


# ------------------------------------------------------------------------------------------- 1. tile edges through the C-ABI

def _dev(a):
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view(np.float64).reshape(a.shape + (2,)) if np.iscomplexobj(a) else a.astype(np.float64))
    return t.contiguous().to("cuda")


class _ThermalOpcorr(object):
    """sc_hk_opcorr_thermal / sc_hk_opcorr_thermal_initial on synthetic operands: qp, zi (n, 2 D), centres (n, 2 d''), omega (d'',),
    cq (n,), built once per (n, D, d'')"""

    def __init__(self, rng, n, D, dm):
        from semiclassical_amd import _lib
        self.lib, self.n, self.D, self.dm = _lib, n, D, dm
        s, sm = 1.0 / np.sqrt(D), 1.0 / np.sqrt(dm)
        self.qp = np.hstack((rng.normal(0.0, 0.6 * s, (n, D)), rng.normal(0.0, 0.9 * s, (n, D))))
        self.zi = np.hstack((rng.normal(0.0, 0.6 * s, (n, D)), rng.normal(0.0, 0.9 * s, (n, D))))
        self.centres = np.hstack((rng.normal(0.0, 0.7 * sm, (n, dm)), rng.normal(0.0, 0.8 * sm, (n, dm))))
        self.omega = rng.uniform(0.5, 2.0, dm)
        self.cq = (rng.normal(size=n) + 1j * rng.normal(size=n)) / n
        self.stream = torch.cuda.current_stream().cuda_stream
        self.omega_d = _dev(self.omega)

    def operands(self, rng, M):
        """(u, w (M, D), ut, wt (M, d''), kappa (M,) complex) of one side"""
        return (rng.normal(size=(M, self.D)), rng.normal(size=(M, self.D)), rng.normal(size=(M, self.dm)), rng.normal(size=(M, self.dm)),
                rng.normal(size=M) + 1j * rng.normal(size=M))

    def rotated(self, t, centres=None):
        c = self.centres if centres is None else centres
        Q, P, w = c[:, :self.dm], c[:, self.dm:], self.omega[None, :]
        return Q * np.cos(w * t) + P / w * np.sin(w * t), P * np.cos(w * t) - w * Q * np.sin(w * t)

    def affine(self, z, side, t):
        u, w, ut, wt, kap = side
        Qt, Pt = self.rotated(t)
        return kap[None, :] + z[:, :self.D] @ u.T + Qt @ ut.T + 1j * (z[:, self.D:] @ w.T + Pt @ wt.T)

    def initial(self, ket):
        lib, ptr = self.lib.lib, self.lib.ptr
        M = ket[0].shape[0]
        g = torch.full((self.n, M, 2), np.nan, device="cuda")
        bufs = [_dev(a) for a in (self.zi, self.centres) + tuple(ket)]
        self.lib.check(lib.sc_hk_opcorr_thermal_initial(ptr(bufs[0]), ptr(bufs[1]), self.n, self.D, self.dm, ptr(bufs[2]), ptr(bufs[3]),
                                                        ptr(bufs[4]), ptr(bufs[5]), ptr(bufs[6]), M, ptr(g), self.stream))
        torch.cuda.synchronize()
        return torch.view_as_complex(g).cpu().numpy()

    def __call__(self, bra, g, t, kept=None, qp=None, cq=None, centres=None):
        lib, ptr = self.lib.lib, self.lib.ptr
        M = bra[0].shape[0]
        bufs = [_dev(a) for a in (self.qp if qp is None else qp, self.cq if cq is None else cq,
                                  self.centres if centres is None else centres) + tuple(bra) + (g,)]
        state = self.lib.sc_state(n=self.n, dim=self.D, mono_layout=0, qp=bufs[0].data_ptr(), act=None, mono=None, c2=None, sgn=None,
                                  work=None, flags=None)
        # map_q, map_p, q0 and n1 are not read: NULL
        th = self.lib.sc_thermal_consts(dim=self.D, dmodes=self.dm, diag=0, omega=ptr(self.omega_d), map_q=None, map_p=None, q0=None,
                                        n1=None, centres=ptr(bufs[2]))
        part = torch.full((int(lib.sc_hk_opcorr_thermal_rows(self.n, M)) * M * 5,), np.nan, device="cuda")
        out = torch.full((1, M, 5), np.nan, device="cuda")
        mask = None if kept is None else torch.from_numpy(np.asarray(kept, dtype=np.uint8)).to("cuda")
        self.lib.check(lib.sc_hk_opcorr_thermal(state, float(t), th, ptr(bufs[1]), ptr(bufs[3]), ptr(bufs[4]), ptr(bufs[5]), ptr(bufs[6]),
                                                ptr(bufs[7]), ptr(bufs[8]), M, ptr(mask), ptr(part), ptr(out), None, self.stream))
        torch.cuda.synchronize()
        return out.cpu().numpy()[0]


SIZES_N = (1, 63, 64, 65, 130)
SIZES_M = (1, 3, 64, 65)
TIMES = (0.0, 0.9)          # omega in 0.5 ... 2: omega t of order 1


@pytest.mark.parametrize("D", [1, 15, 16, 17, 33])
def test_tile_edges_through_the_c_abi(D):
    rng = np.random.default_rng(2000 + D)
    worst = worst_g = 0.0
    for dm in sorted({d for d in (1, 15, 16, 17, D) if d <= D}):
        for n in SIZES_N:
            call = _ThermalOpcorr(rng, n, D, dm)
            masks = [None, np.arange(n) >= 64, np.arange(n) == n // 2]      # none; the first 64-band discarded; a single one kept
            for M in SIZES_M:
                bra, ket = call.operands(rng, M), call.operands(rng, M)
                g = call.initial(ket)
                want_g = call.affine(call.zi, ket, 0.0)
                dev_g = abs(g - want_g).max() / abs(want_g).max()
                assert g.shape == (n, M) and dev_g <= 1e-12, (n, M, dm, dev_g)
                worst_g = max(worst_g, dev_g)
                for t in TIMES:
                    x = call.affine(call.qp, bra, t) * g * call.cq[:, None]
                    for kept in masks:
                        got = call(bra, g, t, kept)
                        want = restated_rows(x, kept)
                        assert got.shape == want.shape == (M, 5) and np.isfinite(got).all()
                        scale = abs(want).max(axis=1)                # every row against its largest entry
                        dev = abs(got - want).max(axis=1)
                        assert (dev <= TOL * scale).all(), (n, M, dm, t, kept is not None, dev.max(), scale)
                        worst = max(worst, (dev[scale > 0] / scale[scale > 0]).max() if (scale > 0).any() else 0.0)
                        if kept is not None and not kept.any():
                            assert not got.any()                     # nobody kept: exact zeros
                    assert np.array_equal(call(bra, g, t, kept), got)                # two calls, the same bits
                # a non-finite cq, g, state or centre of a discarded trajectory never reaches the sums: each alone, and all together
                if n > 1:
                    kept, t = np.arange(n) > 0, TIMES[1]
                    clean = call(bra, g, t, kept)
                    qp, cq, cen, gd = call.qp.copy(), call.cq.copy(), call.centres.copy(), g.copy()
                    qp[0], cq[0], cen[0], gd[0] = np.nan, np.inf, np.nan, np.nan
                    for dirty in (dict(qp=qp), dict(cq=cq), dict(centres=cen), dict(qp=qp, cq=cq, centres=cen)):
                        assert np.array_equal(call(bra, g, t, kept, **dirty), clean), (n, M, dm, sorted(dirty))
                    assert np.array_equal(call(bra, gd, t, kept, qp=qp, cq=cq, centres=cen), clean), (n, M, dm, "all")
    print(f"D={D}: largest deviation of a row {worst:.2e} of its largest entry; of g {worst_g:.2e}")


def test_c_abi_refusals():
    from semiclassical_amd import _lib
    lib, ptr = _lib.lib, _lib.ptr
    buf = torch.zeros(256, device="cuda")
    b = ptr(buf)
    state = _lib.sc_state(n=5, dim=3, mono_layout=0, qp=buf.data_ptr(), act=None, mono=None, c2=None, sgn=None, work=None, flags=None)
    consts = lambda **kw: _lib.sc_thermal_consts(dim=kw.get("dim", 3), dmodes=kw.get("dm", 2), diag=0, omega=kw.get("omega", b), map_q=None,
                                                 map_p=None, q0=None, n1=None, centres=kw.get("centres", b))
    args = lambda **kw: [kw.get("st", state), 0.0, kw.get("th", consts()), b, b, b, b, b, b, b, kw.get("M", 1), None, b, kw.get("out", b),
                         None, None]
    call = lib.sc_hk_opcorr_thermal
    assert call(*args(M=0)) == -1 and call(*args(out=None)) == -1 and call(*args(th=None)) == -1
    assert call(*args(th=consts(omega=None))) == -1 and call(*args(th=consts(centres=None))) == -1 and call(*args(th=consts(dim=4))) == -1
    assert call(*args(M=65536)) == -2 and b"65535" in lib.sc_last_error()
    assert call(*args(th=consts(dm=0))) == -2 and call(*args(th=consts(dm=4))) == -2 and b"d''" in lib.sc_last_error()
    big = _lib.sc_state.from_buffer_copy(state)
    big.dim = 513
    assert call(*args(st=big, th=consts(dim=513))) == -2 and b"512" in lib.sc_last_error()
    many = _lib.sc_state.from_buffer_copy(state)
    many.n = 64 * 65535 + 1
    assert call(*args(st=many)) == -2 and str(64 * 65535).encode() in lib.sc_last_error()
    init = lambda **kw: [kw.get("zi", b), kw.get("cen", b), kw.get("n", 5), kw.get("D", 3), kw.get("dm", 2), b, b, b, b, b, kw.get("M", 1),
                         b, None]
    first = lib.sc_hk_opcorr_thermal_initial
    assert first(*init(M=0)) == -1 and first(*init(zi=None)) == -1 and first(*init(cen=None)) == -1
    assert first(*init(M=65536)) == -2 and first(*init(D=513, dm=3)) == -2 and first(*init(n=64 * 65535 + 1)) == -2
    assert first(*init(dm=0)) == -2 and first(*init(dm=4)) == -2
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------- 2. engine vs restatement

class _ReadBack(object):
    """what tests/thermal_opcorr_cases.py reads of an oracle propagator, from the engine's state read back"""

    def __init__(self, prop):
        self.q0, self.Gamma_i, self.Gamma_t, self.Gamma_0 = prop._q0h, prop._Gi, prop._Gt, prop._G0h
        self._initial = tuple(t.cpu().clone() for t in prop.initial_positions_and_momenta())
        self._current = tuple(t.cpu().clone() for t in prop.current_positions_and_momenta())
        self.cq = (prop.autocorrelation_qp() / (prop._mc_norm() * prop.probi)).cpu().numpy()
        self.tc, self.centres, self.t = prop._thermal["consts"], prop.thermal_centres.cpu(), prop.t

    def initial_positions_and_momenta(self):
        return self._initial

    def current_positions_and_momenta(self):
        return self._current

    def terms(self, bra, ket, t=None):
        """x (n, M) = f g cq with the exported cq and the direct matrix elements at the clock t (default: the engine's)"""
        f, g = toc.thermal_factors(self, self.tc, self.centres, self.t if t is None else t, bra, ket)
        return f * g * self.cq[:, None]


@pytest.mark.parametrize("case", list(CASES))
def test_engine_matches_restatement(case):
    """measured on the MI355X (deviation / max |X|): see DESIGN.md section 4.20"""
    g, pot, opot, prop, ref, tc, centres = CASES[case]()
    dt, E0 = float(g["dt"]), float(g["E0"])
    for _ in range(3):
        prop.step(pot, dt)
    bra, ket = _operators(prop, 5, np.random.default_rng(len(case)))
    before = [t.clone() for t in (prop._qp, prop._act, prop._mono, prop._c2, prop._sgn)]
    X, sigma = prop.thermal_operator_correlation(bra, ket, energy0_es=E0, standard_errors=True)
    assert X.shape == sigma.shape == (6,) and X.dtype == np.complex128
    assert np.array_equal(prop.thermal_operator_correlation(bra, ket, energy0_es=E0), X)          # the same bits in every call
    x = _ReadBack(prop).terms(bra, ket)
    want, want_sigma = toc.estimate(x, np.exp(1j * prop.t * E0))
    scale = abs(want).max()
    auto = prop.autocorrelation(E0)
    dev_sigma = max((abs(sigma.real - want_sigma.real) / want_sigma.real).max(), (abs(sigma.imag - want_sigma.imag) / want_sigma.imag).max())
    print(f"{case}: D = {tc.dim}, d'' = {tc.dmodes}, n = {prop.ntraj}: deviation {abs(X - want).max() / scale:.2e} of max |X| = {scale:.3e}; "
          f"|X_(1,1) - C_auto| {abs(X[5] - auto):.2e}; sigma {dev_sigma:.2e} relative")
    assert scale > 0 and abs(X - want).max() <= TOL * scale
    assert abs(X[5] - auto) <= 1e-12                              # the (1, 1) pair is the autocorrelation function
    assert dev_sigma <= 1e-9
    # nothing changed: the state, and the step that follows
    assert all(torch.equal(a, b) for a, b in zip(before, (prop._qp, prop._act, prop._mono, prop._c2, prop._sgn)))
    twin = CASES[case]()
    for _ in range(4):
        twin[3].step(twin[1], dt)
    prop.step(pot, dt)
    assert torch.equal(prop.y, twin[3].y) and torch.equal(prop._c2, twin[3]._c2) and torch.equal(prop._sgn, twin[3]._sgn)


@pytest.mark.parametrize("name", ["hk_as5_chi002", "hk_methylium"])
def test_zero_temperature_is_operator_correlation(name):
    from semiclassical_amd import hostmath, propagators as PR
    from tests.engine_cases import engine_potential, engine_propagator
    g = cases.load(name)
    pot, cold = engine_potential(g), engine_propagator(g)
    dt, E0 = float(g["dt"]), float(g["E0"])
    masses = cases.oracle_potential(g).masses().to(torch.float64)
    dm = hostmath.ThermalConstants(cases.T(g["Gamma_0"]), masses, 0.0).dmodes
    prop = PR.HermanKlukPropagator(cases.T(g["Gamma_i"]), cases.T(g["Gamma_t"]), device="cuda")
    prop.set_thermal_initial_conditions(cases.T(g["q0"]), cases.T(g["p0"]), cases.T(g["Gamma_0"]), masses, 0.0,
                                        torch.zeros((g["zi"].shape[1], 2 * dm)), cases.T(g["zi"]), cases.T(g["probi"]))
    pot2 = engine_potential(g)
    bra, ket = _operators(cold, 4, np.random.default_rng(5))
    worst = 0.0
    for _ in range(4):
        X0 = cold.operator_correlation(bra, ket, energy0_es=E0)
        X = prop.thermal_operator_correlation(bra, ket, energy0_es=E0)
        worst = max(worst, abs(X - X0).max() / abs(X0).max())
        cold.step(pot, dt)
        prop.step(pot2, dt)
    print(f"{name}: k_B T = 0 against operator_correlation(): {worst:.1e} of max |X|")
    assert worst <= 1e-12


# ------------------------------------------------------------------------------------------- 3. the clock of every state

def test_routes_agree_on_the_state_time(monkeypatch):
    """D = 60 (hk_as60 constants, n = 96): run(thermal_operators=...) in pairs, in visits of three and one launch per step against
    thermal_operator_correlation() in a step() loop; C, k, errors, blocks and the final state are the bits of the same run()
    without the keyword.  A mid state whose bra centres were rotated to another state's time would be off by the rotation of a step:
    the restatement one dt off is asserted to differ by more than 1e3 times the bound."""
    nt, kT = 7, 0.005
    g, pot, _, loop, _, _, _ = _golden_case("hk_as60_n96", kT)
    dt, E0 = float(g["dt"]), float(g["E0"])
    bra, ket = _operators(loop, 3, np.random.default_rng(nt))
    want, want_sigma = [], []
    for k in range(nt):
        if k == 2:
            rb = _ReadBack(loop)
            here, off = (toc.estimate(rb.terms(bra, ket, t))[0] for t in (loop.t, loop.t + dt))
        x, s = loop.thermal_operator_correlation(bra, ket, energy0_es=E0, standard_errors=True)
        want.append(x)
        want_sigma.append(s)
        loop.step(pot, dt)
    want, want_sigma = np.array(want), np.array(want_sigma)
    scale = abs(want).max()
    bound = 1e-13 * scale
    assert abs(here * np.exp(1j * 2 * dt * E0) - want[2]).max() <= TOL * scale
    print(f"the restatement one dt off differs by {abs(off - here).max() / scale:.2e} of max |X|")
    assert abs(off - here).max() > 1e3 * bound
    for route, attrs, entry in (("pairs", {"visit_min_bytes": 0, "visit_steps": 2}, "sc_hk_step_multi"),
                                ("visits", {"visit_min_bytes": 0, "visit_steps": 3}, "sc_hk_step_visit"),
                                ("single", {"pair_steps": False}, "sc_hk_step")):
        out, state = [], []
        for with_ops in (True, False):
            g, pot, _, prop, _, _, _ = _golden_case("hk_as60_n96", kT)
            for key, value in attrs.items():
                setattr(prop, key, value)
            blocks = torch.zeros((nt, 4, 4), device=prop.device)
            spy = _Spy(monkeypatch)
            out.append(prop.run(pot, dt, nt, E0, standard_errors=True, blocks=blocks,
                                **({"thermal_operators": (bra, ket)} if with_ops else {})))
            monkeypatch.undo()
            state.append((blocks, prop.y, prop._c2, prop._sgn, prop.t))
            assert spy.seen.get(entry, 0) > 0 and spy.seen.get("sc_hk_opcorr_thermal", 0) == (nt if with_ops else 0), (route, spy.seen)
            assert spy.seen.get("sc_hk_correlate_thermal", 0) == nt
        (C, k, sC, sk, X, sX), plain = out
        assert len(plain) == 4 and all(np.array_equal(a, b) for a, b in zip((C, k, sC, sk), plain))
        assert all(torch.equal(a, b) for a, b in zip(state[0][:4], state[1][:4])) and state[0][4] == state[1][4]
        dev = abs(X - want).max()
        print(f"{route}: run() against the step() loop {dev / scale:.1e} of max |X| = {scale:.3e}")
        assert X.shape == (nt, 4) and dev <= bound and abs(sX - want_sigma).max() <= 1e-9 * abs(want_sigma).max()
        assert abs(X[:, 3] - C).max() <= 1e-12                   # the last pair is (1, 1)
    # slots= given: the raw rows in the caller's buffer give the same numbers
    g, pot, _, raw, _, _, _ = _golden_case("hk_as60_n96", kT)
    raw.pair_steps = False
    slots, buf = torch.zeros((nt, 5), device=raw.device), torch.full((nt + 1, 4, 5), np.nan, device=raw.device)
    assert raw.run(pot, dt, nt, E0, slots=slots, thermal_operators=(bra, ket), thermal_opcorr=buf) is None
    raw.synchronize()
    X4, sX4 = raw.finalize_cross(buf[:nt], 0.0, dt, E0, raw._ntraj_norm)
    assert np.array_equal(X4, X) and np.array_equal(sX4, sX) and torch.isnan(buf[nt]).all()


# ------------------------------------------------------------------------------------------- 4. discard mask, closed form

def test_after_discard_nonsymplectic():
    g, pot, _, prop, _, _, _ = _golden_case("hk_as5_chi002", 0.006, n=203)
    dt, E0 = float(g["dt"]), float(g["E0"])
    for _ in range(6):
        prop.step(pot, dt)
    prop.discard_nonsymplectic(float(prop.symplectic_deviation().median()))
    kept, n = prop.kept.cpu().numpy(), prop.ntraj
    assert 0 < kept.sum() < n
    bra, ket = _operators(prop, 5, np.random.default_rng(8))
    X = prop.thermal_operator_correlation(bra, ket, energy0_es=E0)
    x = _ReadBack(prop).terms(bra, ket)                          # cq carries the unchanged N; the restatement selects
    want = x[kept.astype(bool)].sum(0) * np.exp(1j * prop.t * E0)
    scale = abs(want).max()
    assert abs(x.sum(0) - x[kept.astype(bool)].sum(0)).max() > 1e-3 * scale      # the mask matters
    print(f"masked, kept {int(kept.sum())} of {n}: deviation {abs(X - want).max() / scale:.2e} of max |X|")
    assert abs(X - want).max() <= TOL * scale and abs(X[5] - prop.autocorrelation(E0)) <= 1e-12
    out = prop.run(pot, dt, 2, E0, thermal_operators=(bra, ket))
    assert len(out) == 3 and abs(out[2][0] - want).max() <= TOL * scale and abs(out[2][:, 5] - out[0]).max() <= 1e-12


def test_standard_errors_cover_the_closed_form():
    """t = 0 on the 2-D exactness model as a dense engine case (the samples of tests/test_thermal_opcorr_host.py): the three
    non-trivial pairs within 5 sigma of the closed form"""
    from semiclassical_amd import propagators as PR
    m = tcs.model_2d()
    ref, _, tc, centres = tcs.model_objects(m, m["kT"], 20000, 7)
    G0, q0 = cases.T(m["Gamma_0"]), cases.T(m["q0"])
    prop = PR.HermanKlukPropagator(G0, G0, device="cuda")
    prop.set_thermal_initial_conditions(q0, torch.zeros_like(q0), G0, cases.T(m["masses"]), m["kT"], centres, ref.zi, ref.probi)
    bra, ket = toc.exactness_pairs()
    X, sigma = prop.thermal_operator_correlation(bra, ket, energy0_es=m["E0"], standard_errors=True)
    closed = toc.closed_form_t0(bra, ket, m["q0"], tc)
    d = X - closed
    for a in range(4):
        print(f"pair {a}: X {X[a]:.6f}  closed form {closed[a]:.6f}  sigma {sigma[a]:.2e}")
    floor = 1e-12 * abs(closed)
    assert (abs(d.real) <= 5.0 * sigma.real + floor).all() and (abs(d.imag) <= 5.0 * sigma.imag + floor).all()
    assert (sigma.real[1:] > 1e-4).all() and (sigma.real <= 0.01).all()         # error bars that mean something


# ------------------------------------------------------------------------------------------- 5. refusals

def test_refusals():
    from semiclassical_amd import propagators as PR
    from tests.engine_cases import engine_potential, engine_propagator
    g, pot, _, prop, ref, tc, centres = _golden_case("hk_as5_chi002", 0.006, n=64)
    D, dt = prop.dim, float(g["dt"])
    ok = (np.ones(2), np.ones((2, D)))
    bad_m = np.ones((2, D))
    bad_m[1, 2] = np.inf
    for ops in ((np.ones(2), np.ones((2, D + 1))), (np.ones(3), np.ones((2, D))), (np.ones(2), np.ones(D)), (np.ones(0), np.ones((0, D))),
                (np.ones(2), bad_m), (np.full(2, np.nan), np.ones((2, D)))):
        with pytest.raises(ValueError):
            prop.thermal_operator_correlation(ops)
        with pytest.raises(ValueError):
            prop.thermal_operator_correlation(ok, ops)
        with pytest.raises(ValueError):
            prop.run(pot, dt, 2, thermal_operators=ops)
        with pytest.raises(ValueError):
            prop.run(pot, dt, 2, thermal_operators=(ok, ops))
    with pytest.raises(ValueError):
        prop.thermal_operator_correlation(ok, (np.ones(3), np.ones((3, D))))       # another number of operators on the ket side
    K = np.zeros((2, D, D))
    K[0, 0, 0] = 1.0
    for kw in (dict(bra=ok + (K,)), dict(bra=ok, ket=ok + (K,))):
        with pytest.raises(NotImplementedError, match="quadratic"):
            prop.thermal_operator_correlation(**kw)
    with pytest.raises(NotImplementedError, match="quadratic"):
        prop.run(pot, dt, 2, thermal_operators=ok + (K,))
    prop.thermal_operator_correlation(ok + (np.zeros((2, D, D)),))              # a K of zeros is no K
    with pytest.raises(ValueError, match="use_graph"):
        prop.run(pot, dt, 4, thermal_operators=ok, use_graph=True)
    slots = torch.zeros((2, 5), device=prop.device)
    with pytest.raises(ValueError, match="thermal_opcorr"):
        prop.run(pot, dt, 2, slots=slots, thermal_operators=ok)
    for buf in (torch.zeros((2, 2, 4), device=prop.device), torch.zeros((1, 2, 5), device=prop.device),
                torch.zeros((2, 3, 5), device=prop.device), torch.zeros((2, 2, 5)), torch.zeros((2, 2, 5), device=prop.device, dtype=torch.float32)):
        with pytest.raises(ValueError, match="thermal_opcorr"):
            prop.run(pot, dt, 2, slots=slots, thermal_operators=ok, thermal_opcorr=buf)
    with pytest.raises(ValueError, match="thermal_operators"):
        prop.run(pot, dt, 2, thermal_opcorr=torch.zeros((2, 2, 5), device=prop.device))
    # the zero-temperature names stay refused on a thermal ensemble, and name the way
    with pytest.raises(NotImplementedError, match="thermal_operator_correlation"):
        prop.operator_correlation(ok)
    with pytest.raises(NotImplementedError, match="thermal"):
        prop.run(pot, dt, 2, operators=ok)
    assert prop.t == 0.0                                        # none of the refused calls took a step
    # without a thermal ensemble
    cold, cold_pot = engine_propagator(g), engine_potential(g)
    with pytest.raises(ValueError, match="operator_correlation"):
        cold.thermal_operator_correlation(ok)
    with pytest.raises(ValueError, match="operator_correlation"):
        cold.run(cold_pot, dt, 2, thermal_operators=ok)
    assert cold.t == 0.0
    # a vector outside the range of the singular widths of methylium
    gm, potm, _, meth, _, _, _ = _golden_case("hk_methylium", 0.004, n=64)
    e, V = np.linalg.eigh(meth._Gt.numpy() + meth._G0h.numpy())
    null = V[:, abs(e) <= 1e-8][:, :1].T
    with pytest.raises(ValueError, match="range"):
        meth.thermal_operator_correlation((np.zeros(1), null))
    with pytest.raises(ValueError, match="range"):
        meth.run(potm, float(gm["dt"]), 2, thermal_operators=((np.ones(1), np.zeros((1, meth.dim))), (np.zeros(1), null)))
    wm = PR.WaltonManolopoulosPropagator(cases.T(g["Gamma_i"]), cases.T(g["Gamma_t"]), 100.0, 100.0, device="cuda")
    with pytest.raises(NotImplementedError):
        wm.thermal_operator_correlation(ok)


# ------------------------------------------------------------------------------------------- 6. driver

def test_driver_key_with_a_temperature(tmp_path):
    """the task of test_thermal_gpu.py::test_driver_temperature_key plus an operator file"""
    from semiclassical_amd import driver, hostmath, propagators as PR, units
    g = cases.load("hk_as5_chi002")
    model, ofile, out = tmp_path / "AS_model.dat", tmp_path / "operators.npz", tmp_path / "correlations.npz"
    np.savetxt(model, np.vstack((g["omega"] * 219474.63, 0.5 * g["omega"] * g["q0"] ** 2 * np.sign(g["q0"]), g["nac"], np.full(5, 0.02))).T)
    rng = np.random.default_rng(21)
    bra = (np.array([1.0, 0.3]), np.vstack((np.zeros(5), rng.normal(size=5))))
    ket = (np.array([1.0, -0.2]), np.vstack((np.zeros(5), rng.normal(size=5))))
    np.savez(ofile, bra_c=bra[0], bra_m=bra[1], ket_c=ket[0], ket_m=ket[1])
    n, nt, kelvin = 300, 4, 1500.0
    task = {"task": "dynamics", "potential": {"type": "anharmonic AS", "model_file": str(model)}, "propagator": "HK",
            "batch_size": n, "num_trajectories": n, "num_steps": nt, "time_step_fs": 0.04, "results": {"correlations": str(out)},
            "manual_seed": 4, "sampling": "host", "temperature": kelvin, "standard_errors": True, "operator_correlation": str(ofile)}
    driver.run_semiclassical_dynamics(task, device="cuda")
    d = dict(np.load(out))
    assert float(d["temperature"]) == kelvin and int(d["trajectories"]) == n
    assert np.array_equal(d["operator_bra_m"], bra[1]) and np.array_equal(d["operator_ket_c"], ket[0])
    X = d["operator_correlation"]
    assert X.shape == (nt, 2) and d["operator_correlation_error"].shape == (nt, 2)
    assert abs(X[:, 0] - d["autocorrelation"]).max() <= 1e-9
    # the same draw on the host (the xi of initial_conditions, then the centres) through the restatement
    setup = driver.build_problem(task)
    tc = hostmath.ThermalConstants(setup.Gamma_0, setup.potential.masses(), units.kelvin_to_hartree * kelvin)
    _, _, iLz, detLz, dprime = hostmath.sampling_matrices(setup.Gamma_0, setup.Gamma_0)
    torch.manual_seed(4)
    zi, probi = PR.HermanKlukPropagator._draw_on_host(torch.zeros(10), iLz, detLz / (2 * np.pi) ** 5, dprime, n)
    centres = tc.draw_centres(n)
    a, b = tc.cartesian(centres)
    zi = zi + torch.cat((setup.q0.unsqueeze(0) + a, b), 1).T
    ref = orc.HKOracle(setup.Gamma_0, setup.Gamma_0)
    ref.set_initial_conditions(setup.q0, setup.p0, setup.Gamma_0, zi, probi)
    opot = orc.MorseOracle(g["omega"], np.full(5, 0.02), g["nac"])
    want, _ = toc.run_restatement(ref, opot, tc, centres, 0.04 / units.autime_to_fs, nt, bra, ket, setup.zero_point_energy)[False]
    print(f"driver: second pair against the restatement {abs(X[:, 1] - want[:, 1]).max() / abs(want[:, 1]).max():.2e}")
    assert abs(X[:, 1] - want[:, 1]).max() <= 1e-9 * abs(want[:, 1]).max()
    # other operators with overwrite: false: refused before anything runs, the file as it was
    again = dict(task, results={"correlations": str(out), "overwrite": False})
    again.pop("manual_seed")
    np.savez(ofile, bra_c=bra[0], bra_m=bra[1])
    with pytest.raises(driver.ConfigurationError, match="operators"):
        driver.run_semiclassical_dynamics(again, device="cuda")
    after = dict(np.load(out))
    # (byte for byte: the anharmonic AS model has no adiabatic gap, the file holds a NaN there)
    assert set(after) == set(d) and all(after[k].dtype == d[k].dtype and after[k].tobytes() == d[k].tobytes() for k in d)
    # quadratic operators with a temperature
    np.savez(ofile, bra_c=bra[0], bra_m=bra[1], bra_k=np.tile(np.eye(5), (2, 1, 1)))
    with pytest.raises(driver.ConfigurationError, match="bra_k"):
        driver.run_semiclassical_dynamics(dict(task, results={"correlations": str(tmp_path / "quad.npz")}), device="cuda")
    # a second batch pools
    np.savez(ofile, bra_c=bra[0], bra_m=bra[1], ket_c=ket[0], ket_m=ket[1])
    driver.run_semiclassical_dynamics(again, device="cuda")
    pooled = np.load(out)
    assert int(pooled["trajectories"]) == 2 * n and abs(pooled["operator_correlation"][:, 0] - pooled["autocorrelation"]).max() <= 1e-9
    # without "operator_correlation" the thermal file has exactly the keys it has today
    plain = tmp_path / "plain.npz"
    bare = {k: v for k, v in task.items() if k not in ("operator_correlation", "standard_errors")}
    bare["results"] = {"correlations": str(plain)}
    driver.run_semiclassical_dynamics(bare, device="cuda")
    assert set(np.load(plain).keys()) == {"propagator", "times", "autocorrelation", "ic_correlation", "adiabatic_gap",
                                          "zero_point_energy", "trajectories", "temperature"}
