"""HermanKlukPropagator.thermal_quadratic_correlation / run(thermal_quadratic=...) (sc_hk_opquad_thermal)
against the numpy restatement of tests/thermal_opquad_cases.py: the tile, chunk, band and column edges through the C-ABI, the engine
on the thermal models, the clock of the mid states of pairs and visits, the dispatch on K, the discard mask, the closed form at
t = 0, the zero-temperature limit and every refusal."""
import numpy as np
import pytest
import torch

from tests import cases, thermal_cases as tcs, thermal_opquad_cases as tqc
from tests.lib_spy import LibSpy as _Spy
from tests.test_opcorr_host import restated_rows
from tests.test_opquad_gpu import _operators as _ranked_operators
from tests.test_thermal_gpu import CASES, _golden_case
from tests.test_thermal_opcorr_gpu import _ReadBack, _dev
from tests.thermal_opcorr_cases import estimate

pytestmark = pytest.mark.gpu
torch.set_default_dtype(torch.float64)

TOL = 1e-9          # x max |X|: the project's tolerance for a sum over trajectories against the host


# ------------------------------------------------------------------------------------------- 1. tile edges through the C-ABI

class _ThermalOpquad(object):
    """sc_hk_opquad_thermal / sc_hk_opquad_thermal_initial on synthetic operands: qp, zi (n, 2 D), centres (n, 2 d''), omega (d'',),
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

    def operands(self, rng, M, R, unit=False):
        """(u, w (M, 1 + R, D), ut, wt (M, 1 + R, d''), kappa (M, 1 + R) complex, lam (M, 1 + R)) of one side; ``unit``: lam = 1"""
        shape = (M, 1 + R)
        return (rng.normal(size=shape + (self.D,)), rng.normal(size=shape + (self.D,)), rng.normal(size=shape + (self.dm,)),
                rng.normal(size=shape + (self.dm,)), rng.normal(size=shape) + 1j * rng.normal(size=shape),
                np.ones(shape) if unit else rng.normal(size=shape))

    def rotated(self, t, centres=None):
        c = self.centres if centres is None else centres
        Q, P, w = c[:, :self.dm], c[:, self.dm:], self.omega[None, :]
        return Q * np.cos(w * t) + P / w * np.sin(w * t), P * np.cos(w * t) - w * Q * np.sin(w * t)

    def value(self, z, side, t, centres=None):
        """sum over the columns of lam z^p: (n, M)"""
        u, w, ut, wt, kap, lam = side
        Qt, Pt = self.rotated(t, centres)
        zc = (kap[None] + np.einsum('acd,nd->nac', u, z[:, :self.D]) + np.einsum('acd,nd->nac', ut, Qt)
              + 1j * (np.einsum('acd,nd->nac', w, z[:, self.D:]) + np.einsum('acd,nd->nac', wt, Pt)))
        return lam[None, :, 0] * zc[:, :, 0] + (lam[None, :, 1:] * zc[:, :, 1:] ** 2).sum(2)

    def initial(self, ket):
        lib, ptr = self.lib.lib, self.lib.ptr
        M, RB = ket[5].shape[0], ket[5].shape[1] - 1
        g = torch.full((self.n, M, 2), np.nan, device="cuda")
        bufs = [_dev(a) for a in (self.zi, self.centres) + tuple(ket)]
        self.lib.check(lib.sc_hk_opquad_thermal_initial(ptr(bufs[0]), ptr(bufs[1]), self.n, self.D, self.dm, *map(ptr, bufs[2:]), M, RB,
                                                        ptr(g), self.stream))
        torch.cuda.synchronize()
        return torch.view_as_complex(g).cpu().numpy()

    def __call__(self, bra, g, t, kept=None, qp=None, cq=None, centres=None, cursor=None, rows=1, entry="quad"):
        """the rows of sc_hk_opquad_thermal; ``entry``: "linear" = sc_hk_opcorr_thermal, "cold" = sc_hk_opquad on the same operands"""
        lib, ptr = self.lib.lib, self.lib.ptr
        M, RA = bra[5].shape[0], bra[5].shape[1] - 1
        d_qp, d_cq, d_cen = (_dev(a) for a in (self.qp if qp is None else qp, self.cq if cq is None else cq,
                                               self.centres if centres is None else centres))
        b, d_g = [_dev(a) for a in bra], _dev(g)
        state = self.lib.sc_state(n=self.n, dim=self.D, mono_layout=0, qp=d_qp.data_ptr(), act=None, mono=None, c2=None, sgn=None,
                                  work=None, flags=None)
        # map_q, map_p, q0 and n1 are not read: NULL
        th = self.lib.sc_thermal_consts(dim=self.D, dmodes=self.dm, diag=0, omega=ptr(self.omega_d), map_q=None, map_p=None, q0=None,
                                        n1=None, centres=ptr(d_cen))
        part = torch.full((int(lib.sc_hk_opquad_thermal_rows(self.n, M)) * M * 5,), np.nan, device="cuda")
        out = torch.full((rows, M, 5), np.nan, device="cuda")
        mask = None if kept is None else torch.from_numpy(np.asarray(kept, dtype=np.uint8)).to("cuda")
        cur = None if cursor is None else torch.tensor([cursor], dtype=torch.int64, device="cuda")
        tail = (M, ptr(mask), ptr(part), ptr(out), ptr(cur), self.stream)
        if entry == "linear":
            self.lib.check(lib.sc_hk_opcorr_thermal(state, float(t), th, ptr(d_cq), *map(ptr, b[:5]), ptr(d_g), *tail))
        elif entry == "cold":
            self.lib.check(lib.sc_hk_opquad(state, ptr(d_cq), ptr(b[0]), ptr(b[1]), ptr(b[4]), ptr(b[5]), ptr(d_g), M, RA, *tail[1:]))
        else:
            self.lib.check(lib.sc_hk_opquad_thermal(state, float(t), th, ptr(d_cq), *map(ptr, b), ptr(d_g), M, RA, *tail[1:]))
        torch.cuda.synchronize()
        if cur is not None:
            assert int(cur.item()) == cursor                     # read, not advanced
        return out.cpu().numpy()


SIZES_N = (1, 63, 64, 65, 130)
SHAPES_MR = ((1, 0), (1, 1), (3, 2), (1, 63), (1, 64), (1, 130), (2, 31), (2, 32), (65, 1))
RANKS_KET = (0, 3)
TIMES = (0.0, 0.9)          # omega in 0.5 ... 2: omega t of order 1
DIMS = (1, 16, 17, 33)


def _schedule(D):
    """(n, M, RA, RB, d'') of one D: not the full product -- every shape with two of the n, both ket ranks and two of the d'', the
    offsets moving with D so that over the four D every value of a list meets at least two values of every other; the wide case
    (1, 130) with d'' = 17 where D allows it"""
    dms = sorted({d for d in (1, 15, 16, 17, D) if d <= D})
    off = DIMS.index(D)
    for idx, (M, RA) in enumerate(SHAPES_MR):
        for j in (0, 1):
            dm = dms[(idx + j * (1 + off)) % len(dms)]
            if (M, RA) == (1, 130) and j == 0 and 17 in dms:
                dm = 17
            yield SIZES_N[(idx + 2 * j + off) % 5], M, RA, RANKS_KET[(idx + j) % 2], dm


def test_the_schedule_covers_the_lists():
    seen = [(n, (M, RA), RB, D, dm) for D in DIMS for n, M, RA, RB, dm in _schedule(D)]
    for i in range(5):
        for j in range(5):
            if i != j:
                for v in {s[i] for s in seen}:
                    # (d'' <= D: D = 1 has the one d'' = 1, and d'' = 33 the one D = 33)
                    need = 1 if (i, j, v) in ((3, 4, 1), (4, 3, 33)) else 2
                    assert len({s[j] for s in seen if s[i] == v}) >= need, (i, j, v)
    assert {s[1] for s in seen} == set(SHAPES_MR) and {s[0] for s in seen} == set(SIZES_N) and {s[2] for s in seen} == set(RANKS_KET)
    assert {1, 15, 16, 17, 33} <= {s[4] for s in seen} and any(s[1] == (1, 130) and s[4] == 17 for s in seen)


@pytest.mark.parametrize("D", DIMS)
def test_tile_edges_through_the_c_abi(D):
    rng = np.random.default_rng(3000 + D)
    worst = worst_g = worst_lin = worst_cold = 0.0
    for n, M, RA, RB, dm in _schedule(D):
        call = _ThermalOpquad(rng, n, D, dm)
        masks = [None, np.arange(n) >= 64, np.arange(n) == n // 2]      # none; the first 64-band discarded; a single one kept
        bra, ket = call.operands(rng, M, RA, unit=RA == 0), call.operands(rng, M, RB, unit=RB == 0)
        g = call.initial(ket)
        want_g = call.value(call.zi, ket, 0.0)
        dev_g = abs(g - want_g).max() / abs(want_g).max()
        assert g.shape == (n, M) and dev_g <= 1e-12, (n, M, RB, dm, dev_g)
        worst_g = max(worst_g, dev_g)
        for t in TIMES:
            x = call.value(call.qp, bra, t) * g * call.cq[:, None]
            for kept in masks:
                got = call(bra, g, t, kept)[0]
                want = restated_rows(x, kept)
                assert got.shape == want.shape == (M, 5) and np.isfinite(got).all()
                scale = abs(want).max(axis=1)                # every row against its largest entry
                dev = abs(got - want).max(axis=1)
                assert (dev <= TOL * scale).all(), (n, M, RA, RB, dm, t, kept is not None, dev.max(), scale)
                worst = max(worst, (dev[scale > 0] / scale[scale > 0]).max() if (scale > 0).any() else 0.0)
                if kept is not None and not kept.any():
                    assert not got.any()                     # nobody kept: exact zeros
                if RA == 0 and RB == 0:
                    # no squared column: the rows of sc_hk_opcorr_thermal on the same operands
                    lin = call(bra, g, t, kept, entry="linear")[0]
                    dev_lin = abs(got - lin).max(axis=1)
                    assert (dev_lin <= 1e-13 * abs(lin).max(axis=1)).all(), (n, M, dm, dev_lin.max())
                    worst_lin = max(worst_lin, (dev_lin[scale > 0] / abs(lin).max(axis=1)[scale > 0]).max() if (scale > 0).any() else 0.0)
            assert np.array_equal(call(bra, g, t, kept)[0], got)                # two calls, the same bits
        # all centres zero and ut = wt = 0: the rows of sc_hk_opquad on the same operands
        t = TIMES[1]
        still = bra[:2] + (np.zeros_like(bra[2]), np.zeros_like(bra[3])) + bra[4:]
        nowhere = np.zeros_like(call.centres)
        cold = call(still, g, t, masks[1], centres=nowhere, entry="cold")[0]
        dev_cold = abs(call(still, g, t, masks[1], centres=nowhere)[0] - cold).max(axis=1)
        assert (dev_cold <= 1e-13 * abs(cold).max(axis=1)).all(), (n, M, RA, dm, dev_cold.max())
        if abs(cold).max() > 0:
            worst_cold = max(worst_cold, (dev_cold / np.maximum(abs(cold).max(axis=1), 1e-300)).max())
        # a non-finite cq, g, state or centre of a discarded trajectory never reaches the sums: each alone, and all together
        if n > 1:
            kept = np.arange(n) > 0
            clean = call(bra, g, t, kept)[0]
            qp, cq, cen, gd = call.qp.copy(), call.cq.copy(), call.centres.copy(), g.copy()
            qp[0], cq[0], cen[0], gd[0] = np.nan, np.inf, np.nan, np.nan
            for dirty in (dict(qp=qp), dict(cq=cq), dict(centres=cen)):
                assert np.array_equal(call(bra, g, t, kept, **dirty)[0], clean), (n, M, RA, dm, sorted(dirty))
            assert np.array_equal(call(bra, gd, t, kept)[0], clean), (n, M, RA, dm, "g")
            assert np.array_equal(call(bra, gd, t, kept, qp=qp, cq=cq, centres=cen)[0], clean), (n, M, RA, dm, "all")
    # with a cursor the row goes to out[*cursor]
    got = call(bra, g, t, None, cursor=2, rows=3)
    assert np.isnan(got[:2]).all() and np.array_equal(got[2], call(bra, g, t)[0])
    print(f"D={D}: largest deviation of a row {worst:.2e} of its largest entry; of g {worst_g:.2e}; R = 0 against sc_hk_opcorr_thermal "
          f"{worst_lin:.2e}; no centres against sc_hk_opquad {worst_cold:.2e}")


def test_c_abi_refusals():
    from semiclassical_amd import _lib
    lib, ptr = _lib.lib, _lib.ptr
    buf = torch.zeros(4096, device="cuda")
    b = ptr(buf)
    state = _lib.sc_state(n=5, dim=3, mono_layout=0, qp=buf.data_ptr(), act=None, mono=None, c2=None, sgn=None, work=None, flags=None)
    consts = lambda **kw: _lib.sc_thermal_consts(dim=kw.get("dim", 3), dmodes=kw.get("dm", 2), diag=0, omega=kw.get("omega", b), map_q=None,
                                                 map_p=None, q0=None, n1=None, centres=kw.get("centres", b))
    args = lambda **kw: [kw.get("st", state), 0.0, kw.get("th", consts()), kw.get("cq", b), b, b, b, kw.get("wt", b), b, kw.get("lam", b), b,
                         kw.get("M", 1), kw.get("R", 0), None, b, kw.get("out", b), None, None]
    call = lib.sc_hk_opquad_thermal
    assert call(*args()) == 0
    assert all(call(*args(**{null: None})) == -1 for null in ("cq", "wt", "lam", "out", "th"))
    assert call(*args(M=0)) == -1 and call(*args(R=-1)) == -1
    assert call(*args(th=consts(omega=None))) == -1 and call(*args(th=consts(centres=None))) == -1 and call(*args(th=consts(dim=4))) == -1
    assert call(*args(R=513)) == -2 and b"512" in lib.sc_last_error()
    assert call(*args(M=65536)) == -2 and b"65535" in lib.sc_last_error()
    assert call(*args(M=65535, R=256)) == -2 and b"16777216" in lib.sc_last_error()       # 65535 x 257 >= 2^24
    assert call(*args(th=consts(dm=0))) == -2 and call(*args(th=consts(dm=4))) == -2 and b"d''" in lib.sc_last_error()
    big = _lib.sc_state.from_buffer_copy(state)
    big.dim = 513
    assert call(*args(st=big, th=consts(dim=513))) == -2 and b"512" in lib.sc_last_error()
    many = _lib.sc_state.from_buffer_copy(state)
    many.n = 64 * 65535 + 1
    assert call(*args(st=many)) == -2 and str(64 * 65535).encode() in lib.sc_last_error()
    init = lambda **kw: [kw.get("zi", b), kw.get("cen", b), kw.get("n", 5), kw.get("D", 3), kw.get("dm", 2), b, b, b, b, b, kw.get("lam", b),
                         kw.get("M", 1), kw.get("R", 0), kw.get("g", b), None]
    first = lib.sc_hk_opquad_thermal_initial
    assert first(*init()) == 0
    assert all(first(*init(**{null: None})) == -1 for null in ("zi", "cen", "lam", "g"))
    assert first(*init(M=0)) == -1 and first(*init(R=-1)) == -1
    assert first(*init(R=513)) == -2 and first(*init(D=513, dm=3)) == -2 and first(*init(M=65535, R=256)) == -2
    assert first(*init(n=64 * 65535 + 1)) == -2 and first(*init(dm=0)) == -2 and first(*init(dm=4)) == -2
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------- 2. engine vs restatement

def _terms(prop, bra, ket, t=None):
    """x (n, M) = f g cq with the exported cq and the direct matrix elements at the clock t (default: the engine's)"""
    rb = _ReadBack(prop)
    f, g = tqc.thermal_factors(rb, rb.tc, rb.centres, rb.t if t is None else t, bra, ket)
    return f * g * rb.cq[:, None]


def _operators(prop, rng):
    """the four pairs of tests/test_opquad_gpu.py (bra K of ranks 1, 2, D, 0, ket K of ranks 0, 1, D, 2, projected onto the range of
    their side) and then (1, 1)"""
    D = prop.dim
    one = (np.ones(1), np.zeros((1, D)), np.zeros((1, D, D)))
    return tuple(tuple(np.concatenate((a, b)) for a, b in zip(side, one)) for side in _ranked_operators(prop, rng))


@pytest.mark.parametrize("case", list(CASES))
def test_engine_matches_restatement(case):
    """measured on the MI355X (deviation / max |X|): see DESIGN.md section 4.22"""
    g, pot, opot, prop, ref, tc, centres = CASES[case]()
    dt, E0 = float(g["dt"]), float(g["E0"])
    for _ in range(3):
        prop.step(pot, dt)
    bra, ket = _operators(prop, np.random.default_rng(len(case)))
    before = [t.clone() for t in (prop._qp, prop._act, prop._mono, prop._c2, prop._sgn)]
    X, sigma = prop.thermal_quadratic_correlation(bra, ket, energy0_es=E0, standard_errors=True)
    assert X.shape == sigma.shape == (5,) and X.dtype == np.complex128
    assert np.array_equal(prop.thermal_quadratic_correlation(bra, ket, energy0_es=E0), X)          # the same bits in every call
    assert 0 < prop._thermal_opquad["RA"] <= tc.dim and 0 < prop._thermal_opquad["RB"] <= tc.dim
    want, want_sigma = estimate(_terms(prop, bra, ket), np.exp(1j * prop.t * E0))
    scale = abs(want).max()
    auto = prop.autocorrelation(E0)
    dev_sigma = max((abs(sigma.real - want_sigma.real) / want_sigma.real).max(), (abs(sigma.imag - want_sigma.imag) / want_sigma.imag).max())
    print(f"{case}: D = {tc.dim}, d'' = {tc.dmodes}, n = {prop.ntraj}, R = {prop._thermal_opquad['RA']}: deviation "
          f"{abs(X - want).max() / scale:.2e} of max |X| = {scale:.3e}; |X_(1,1) - C_auto| {abs(X[4] - auto):.2e}; sigma {dev_sigma:.2e} relative")
    assert scale > 0 and abs(X - want).max() <= TOL * scale
    assert abs(X[4] - auto) <= 1e-12                              # the (1, 1) pair is the autocorrelation function
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
    bra, ket = _operators(cold, np.random.default_rng(5))
    worst = 0.0
    for _ in range(4):
        X0 = cold.operator_correlation(bra, ket, energy0_es=E0)
        X = prop.thermal_quadratic_correlation(bra, ket, energy0_es=E0)
        worst = max(worst, abs(X - X0).max() / abs(X0).max())
        cold.step(pot, dt)
        prop.step(pot2, dt)
    print(f"{name}: k_B T = 0 against operator_correlation() with K: {worst:.1e} of max |X|")
    assert worst <= 1e-12


# ------------------------------------------------------------------------------------------- 3. the clock of every state

def test_routes_agree_on_the_state_time(monkeypatch):
    """D = 60 (hk_as60 constants, n = 96): run(thermal_quadratic=...) in pairs, in visits of three and one launch per step against
    thermal_quadratic_correlation() in a step() loop: the same bits; C, k, errors, blocks and the final state are the bits of the same
    run() without the keyword.  A mid state whose bra centres were rotated to another state's time would be off by the rotation of
    a step: the restatement one dt off is asserted to differ by more than 1e3 times the bound 1e-9 max |X|."""
    nt, kT = 7, 0.005
    g, pot, _, loop, _, _, _ = _golden_case("hk_as60_n96", kT)
    dt, E0 = float(g["dt"]), float(g["E0"])
    bra, ket = _operators(loop, np.random.default_rng(nt))
    want, want_sigma = [], []
    for k in range(nt):
        if k == 2:
            here, off = (estimate(_terms(loop, bra, ket, t))[0] for t in (loop.t, loop.t + dt))
        x, s = loop.thermal_quadratic_correlation(bra, ket, energy0_es=E0, standard_errors=True)
        want.append(x)
        want_sigma.append(s)
        loop.step(pot, dt)
    want, want_sigma = np.array(want), np.array(want_sigma)
    scale = abs(want).max()
    assert abs(here * np.exp(1j * 2 * dt * E0) - want[2]).max() <= TOL * scale
    print(f"the restatement one dt off differs by {abs(off - here).max() / scale:.2e} of max |X|: "
          f"{abs(off - here).max() / (TOL * scale):.1e} times the bound")
    assert abs(off - here).max() > 1e3 * TOL * scale
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
                                **({"thermal_quadratic": (bra, ket)} if with_ops else {})))
            monkeypatch.undo()
            state.append((blocks, prop.y, prop._c2, prop._sgn, prop.t))
            assert spy.seen.get(entry, 0) > 0 and spy.seen.get("sc_hk_opquad_thermal", 0) == (nt if with_ops else 0), (route, spy.seen)
            assert spy.seen.get("sc_hk_correlate_thermal", 0) == nt and "sc_hk_opcorr_thermal" not in spy.seen
        (C, k, sC, sk, X, sX), plain = out
        assert len(plain) == 4 and all(np.array_equal(a, b) for a, b in zip((C, k, sC, sk), plain))
        assert all(torch.equal(a, b) for a, b in zip(state[0][:4], state[1][:4])) and state[0][4] == state[1][4]
        print(f"{route}: run() against the step() loop {abs(X - want).max() / scale:.1e} of max |X| = {scale:.3e}")
        assert X.shape == (nt, 5) and np.array_equal(X, want) and np.array_equal(sX, want_sigma)
        assert abs(X[:, 4] - C).max() <= 1e-12                   # the last pair is (1, 1)
    # slots= given: the raw rows in the caller's buffer give the same numbers
    g, pot, _, raw, _, _, _ = _golden_case("hk_as60_n96", kT)
    raw.pair_steps = False
    slots, buf = torch.zeros((nt, 5), device=raw.device), torch.full((nt + 1, 5, 5), np.nan, device=raw.device)
    assert raw.run(pot, dt, nt, E0, slots=slots, thermal_quadratic=(bra, ket), thermal_opquad=buf) is None
    raw.synchronize()
    X4, sX4 = raw.finalize_cross(buf[:nt], 0.0, dt, E0, raw._ntraj_norm)
    assert np.array_equal(X4, X) and np.array_equal(sX4, sX) and torch.isnan(buf[nt]).all()


# ------------------------------------------------------------------------------------------- 4. dispatch, discard mask, closed form

def test_a_zero_K_takes_the_linear_path(monkeypatch):
    g, pot, _, prop, _, _, _ = _golden_case("hk_as5_chi002", 0.006, n=130)
    dt, E0, D = float(g["dt"]), float(g["E0"]), prop.dim
    prop.step(pot, dt)
    rng = np.random.default_rng(3)
    bra, ket = (rng.normal(size=3), rng.normal(size=(3, D))), (rng.normal(size=3), rng.normal(size=(3, D)))
    want = prop.thermal_operator_correlation(bra, ket, energy0_es=E0, standard_errors=True)
    for with_K in ((bra + (np.zeros((3, D, D)),), ket + (None,)), (bra, ket), (bra + (None,), ket + (np.zeros((3, D, D)),))):
        prop._thermal_opquad = None
        spy = _Spy(monkeypatch)
        got = prop.thermal_quadratic_correlation(*with_K, energy0_es=E0, standard_errors=True)
        monkeypatch.undo()
        assert spy.seen.get("sc_hk_opcorr_thermal", 0) == 1 and spy.seen.get("sc_hk_opcorr_thermal_initial", 0) == 1
        assert "sc_hk_opquad_thermal" not in spy.seen and "sc_hk_opquad_thermal_initial" not in spy.seen
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
    g, pot, _, a, _, _, _ = _golden_case("hk_as5_chi002", 0.006, n=130)
    g, pot2, _, b, _, _, _ = _golden_case("hk_as5_chi002", 0.006, n=130)
    spy = _Spy(monkeypatch)
    out = a.run(pot, dt, 3, E0, thermal_quadratic=(bra + (np.zeros((3, D, D)),), ket))
    monkeypatch.undo()
    assert spy.seen.get("sc_hk_opcorr_thermal", 0) == 3 and "sc_hk_opquad_thermal" not in spy.seen
    assert all(np.array_equal(x, y) for x, y in zip(out, b.run(pot2, dt, 3, E0, thermal_operators=(bra, ket))))
    # cached per bytes of (c, m, K) until the initial conditions change
    K = np.zeros((3, D, D))
    K[:, 0, 0] = 1.0
    a.thermal_quadratic_correlation(bra + (K,), ket)
    hit = a._thermal_opquad
    a.thermal_quadratic_correlation(bra + (K.copy(),), ket)
    assert a._thermal_opquad is hit and "RA" in hit
    a.thermal_quadratic_correlation(bra + (2.0 * K,), ket)
    assert a._thermal_opquad is not hit


def test_after_discard_nonsymplectic():
    g, pot, _, prop, _, _, _ = _golden_case("hk_as5_chi002", 0.006, n=203)
    dt, E0 = float(g["dt"]), float(g["E0"])
    for _ in range(6):
        prop.step(pot, dt)
    prop.discard_nonsymplectic(float(prop.symplectic_deviation().median()))
    kept, n = prop.kept.cpu().numpy(), prop.ntraj
    assert 0 < kept.sum() < n
    bra, ket = _operators(prop, np.random.default_rng(8))
    X = prop.thermal_quadratic_correlation(bra, ket, energy0_es=E0)
    x = _terms(prop, bra, ket)                                   # cq carries the unchanged N; the restatement selects
    want = x[kept.astype(bool)].sum(0) * np.exp(1j * prop.t * E0)
    scale = abs(want).max()
    assert abs(x.sum(0) - x[kept.astype(bool)].sum(0)).max() > 1e-3 * scale      # the mask matters
    print(f"masked, kept {int(kept.sum())} of {n}: deviation {abs(X - want).max() / scale:.2e} of max |X|")
    assert abs(X - want).max() <= TOL * scale and abs(X[4] - prop.autocorrelation(E0)) <= 1e-12
    out = prop.run(pot, dt, 2, E0, thermal_quadratic=(bra, ket))
    assert len(out) == 3 and abs(out[2][0] - want).max() <= TOL * scale and abs(out[2][:, 4] - out[0]).max() <= 1e-12


def test_standard_errors_cover_the_closed_form():
    """t = 0 on the 2-D exactness model as a dense engine case (the samples of tests/test_thermal_opquad_host.py): the four pairs
    within 5 sigma of the closed form"""
    from semiclassical_amd import propagators as PR
    m = tcs.model_2d()
    ref, _, tc, centres = tcs.model_objects(m, m["kT"], 20000, 7)
    G0, q0 = cases.T(m["Gamma_0"]), cases.T(m["q0"])
    prop = PR.HermanKlukPropagator(G0, G0, device="cuda")
    prop.set_thermal_initial_conditions(q0, torch.zeros_like(q0), G0, cases.T(m["masses"]), m["kT"], centres, ref.zi, ref.probi)
    bra, ket = tqc.exactness_pairs()
    X, sigma = prop.thermal_quadratic_correlation(bra, ket, energy0_es=m["E0"], standard_errors=True)
    closed = tqc.closed_form_t0(bra, ket, m["q0"], tc)
    d = X - closed
    for a in range(4):
        print(f"pair {a}: X {X[a]:.6f}  closed form {closed[a]:.6f}  sigma {sigma[a]:.2e}")
    floor = 1e-12 * abs(closed)
    assert (abs(d.real) <= 5.0 * sigma.real + floor).all() and (abs(d.imag) <= 5.0 * sigma.imag + floor).all()
    assert (sigma.real > 1e-4).all() and (sigma.real <= 0.03).all()             # error bars that mean something


# ------------------------------------------------------------------------------------------- 5. refusals

def test_refusals():
    from semiclassical_amd import propagators as PR
    from tests.engine_cases import engine_potential, engine_propagator
    g, pot, _, prop, ref, tc, centres = _golden_case("hk_as5_chi002", 0.006, n=64)
    D, dt = prop.dim, float(g["dt"])
    c, m, K = np.ones(2), np.ones((2, D)), np.array([np.eye(D)] * 2)
    ok = (c, m, K)
    bad_m, skew, broken = m.copy(), K.copy(), K.copy()
    bad_m[1, 2], skew[1, 0, 1], broken[0, 1, 1] = np.inf, 1e-6, np.inf
    for ops in ((c, np.ones((2, D + 1)), K), (np.ones(3), m, K), (c, np.ones(D), K), (np.ones(0), np.ones((0, D)), np.ones((0, D, D))),
                (c, bad_m, K), (np.full(2, np.nan), m, K), (c, m, skew), (c, m, broken), (c, m, K[:, 0]), (c, m, np.concatenate((K, K[:1]))),
                (c, m, K[:1]), (c, m, K[:, :, :-1])):
        with pytest.raises(ValueError):
            prop.thermal_quadratic_correlation(ops)
        with pytest.raises(ValueError):
            prop.thermal_quadratic_correlation(ok, ops)
        with pytest.raises(ValueError):
            prop.run(pot, dt, 2, thermal_quadratic=ops)
        with pytest.raises(ValueError):
            prop.run(pot, dt, 2, thermal_quadratic=(ok, ops))
    with pytest.raises(ValueError, match="symmetric"):
        prop.thermal_quadratic_correlation((c, m, skew))
    with pytest.raises(ValueError):
        prop.thermal_quadratic_correlation(ok, (np.ones(3), np.ones((3, D))))        # another number of operators on the ket side
    with pytest.raises(ValueError, match="use_graph"):
        prop.run(pot, dt, 4, thermal_quadratic=ok, use_graph=True)
    with pytest.raises(ValueError, match="thermal_operators"):
        prop.run(pot, dt, 2, thermal_quadratic=ok, thermal_operators=(c, m))           # one set of thermal operators per call
    slots = torch.zeros((2, 5), device=prop.device)
    with pytest.raises(ValueError, match="thermal_opquad"):
        prop.run(pot, dt, 2, slots=slots, thermal_quadratic=ok)
    for buf in (torch.zeros((2, 2, 4), device=prop.device), torch.zeros((1, 2, 5), device=prop.device),
                torch.zeros((2, 3, 5), device=prop.device), torch.zeros((2, 2, 5)), torch.zeros((2, 2, 5), device=prop.device, dtype=torch.float32)):
        with pytest.raises(ValueError, match="thermal_opquad"):
            prop.run(pot, dt, 2, slots=slots, thermal_quadratic=ok, thermal_opquad=buf)
    with pytest.raises(ValueError, match="thermal_quadratic"):
        prop.run(pot, dt, 2, thermal_opquad=torch.zeros((2, 2, 5), device=prop.device))
    # the existing refusals keep their types and name the way
    with pytest.raises(NotImplementedError, match="thermal_quadratic_correlation"):
        prop.thermal_operator_correlation(ok)
    with pytest.raises(NotImplementedError, match="thermal_quadratic_correlation"):
        prop.operator_correlation(ok)
    assert prop.t == 0.0                                        # none of the refused calls took a step
    # without a thermal ensemble
    cold, cold_pot = engine_propagator(g), engine_potential(g)
    with pytest.raises(ValueError, match="operator_correlation"):
        cold.thermal_quadratic_correlation(ok)
    with pytest.raises(ValueError, match="operator_correlation"):
        cold.run(cold_pot, dt, 2, thermal_quadratic=ok)
    assert cold.t == 0.0
    # a vector or a kept eigenvector outside the range of the singular widths of methylium
    gm, potm, _, meth, _, _, _ = _golden_case("hk_methylium", 0.004, n=64)
    e, V = np.linalg.eigh(meth._Gt.numpy() + meth._G0h.numpy())
    null = V[:, abs(e) <= 1e-8][:, :1].T
    inside = (np.ones(1), np.zeros((1, meth.dim)))
    with pytest.raises(ValueError, match="range"):
        meth.thermal_quadratic_correlation((np.zeros(1), null, np.zeros((1, meth.dim, meth.dim))))
    with pytest.raises(ValueError, match="range"):
        meth.thermal_quadratic_correlation(inside + (np.einsum('ai,aj->aij', null, null),))
    with pytest.raises(ValueError, match="range"):
        meth.run(potm, float(gm["dt"]), 2, thermal_quadratic=(inside, inside + (np.einsum('ai,aj->aij', null, null),)))
    wm = PR.WaltonManolopoulosPropagator(cases.T(g["Gamma_i"]), cases.T(g["Gamma_t"]), 100.0, 100.0, device="cuda")
    with pytest.raises(NotImplementedError):
        wm.thermal_quadratic_correlation(ok)
