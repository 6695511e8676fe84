"""HermanKlukPropagator.operator_correlation / run(operators=...) (sc_hk_opcorr) against the numpy
restatement of the definition (tests/test_opcorr_host.py): the engine on the golden cases, the bra side against quadrature of the
wavefunction, the tile edges through the C-ABI, every route of run(), the discard mask, the standard errors and the driver key."""
import os

import numpy as np
import pytest
import torch

from tests import cases
from tests.lib_spy import LibSpy as _Spy
from tests.test_cross_host import gaussian
from tests.test_opcorr_host import (bra_factors, closed_form_t0, ket_factors, project, restated_opcorr, restated_rows, t0_operator_pairs,
                                    within_five_sigma)

pytestmark = pytest.mark.gpu
torch.set_default_dtype(torch.float64)

TOL = 1e-9          # x max |X|: the project's tolerance for a sum over trajectories against the host


def _prepared(name, select=None, **attrs):
    from tests.engine_cases import engine_potential, engine_propagator
    g = cases.load(name)
    pot, prop = engine_potential(g), engine_propagator(g, select=select)
    for key, value in attrs.items():
        setattr(prop, key, value)
    return g, pot, prop


def _read_back(prop):
    """what the restatement takes, read back from the engine as numpy: the current (Q, P), the initial (q, p), the per-trajectory
    C_auto terms cq (the Monte-Carlo weight inside) and the three widths, q0, p0"""
    Q, P = (t.cpu().numpy().copy() for t in prop.current_positions_and_momenta())
    q, p = (t.cpu().numpy().copy() for t in prop.initial_positions_and_momenta())
    cq = (prop.autocorrelation_qp() / (prop._mc_norm() * prop.probi)).cpu().numpy()
    return dict(Q=Q, P=P, q=q, p=p, cq=cq, Gi=prop._Gi.numpy(), Gt=prop._Gt.numpy(), G0=prop._G0h.numpy(), q0=prop._q0h.numpy(),
                p0=prop._p0h.numpy())


def _restated(bra, ket, s, kept=None):
    return restated_opcorr(bra, ket, s["Q"], s["P"], s["q"], s["p"], s["cq"], s["Gi"], s["Gt"], s["G0"], s["q0"], s["p0"], kept)


def _operators(prop, M, rng):
    """M random pairs (every m projected onto the range of its side's widths: the identity for regular ones) and then (1, 1)"""
    D = prop.dim
    Gi, Gt, G0 = prop._Gi.numpy(), prop._Gt.numpy(), prop._G0h.numpy()
    mA = np.vstack((project(rng.normal(size=(M, D)), G0, Gt), np.zeros((1, D))))
    mB = np.vstack((project(rng.normal(size=(M, D)), Gi, G0), np.zeros((1, D))))
    return (np.append(rng.normal(size=M), 1.0), mA), (np.append(rng.normal(size=M), 1.0), mB)


# ------------------------------------------------------------------------------------------- 1. engine vs restatement

ENGINE_CASES = ["hk_1d", "hk_as5_chi002", "hk_as33", "hk_as60_n96", "hk_methylium", "hk_coumarin_harmonic"]


@pytest.mark.parametrize("name", ENGINE_CASES)
def test_engine_matches_restatement(name):
    """measured on the MI355X (deviation / max |X|): see DESIGN.md section 4.14"""
    select = slice(0, 45) if name == "hk_as33" else None
    g, pot, prop = _prepared(name, select=select)
    for _ in range(3):
        prop.step(pot, float(g["dt"]))
    bra, ket = _operators(prop, 5, np.random.default_rng(len(name)))
    E0 = float(g["E0"])
    before = [t.clone() for t in (prop._qp, prop._act, prop._mono, prop._c2, prop._sgn)]      # (not prop.y: it may change the layout)
    X, sigma = prop.operator_correlation(bra, ket, energy0_es=E0, standard_errors=True)
    assert X.shape == sigma.shape == (6,) and X.dtype == np.complex128
    assert np.array_equal(prop.operator_correlation(bra, ket, energy0_es=E0), X)          # the same bits in every call
    rows = _restated(bra, ket, _read_back(prop))
    want = (rows[:, 0] + 1j * rows[:, 1]) * np.exp(1j * prop.t * E0)
    scale = abs(want).max()
    print(f"{name}: |X_a| {np.array2string(abs(want), precision=3)}, deviation {abs(X - want).max() / scale:.2e} of the largest")
    assert scale > 0 and abs(X - want).max() <= TOL * scale
    # the (1, 1) pair is the autocorrelation function
    auto = prop.autocorrelation(E0)
    print(f"{name}: |X_(1,1) - C_auto| {abs(X[5] - auto):.2e}")
    assert abs(X[5] - auto) <= TOL * scale
    # ket=None: the operators of the bra on both sides
    if np.array_equal(g["Gamma_i"], g["Gamma_t"]):                 # (singular widths: the bra's m lie in the ket's range as well)
        same = prop.operator_correlation(bra, energy0_es=E0)
        rows2 = _restated(bra, bra, _read_back(prop))
        want2 = (rows2[:, 0] + 1j * rows2[:, 1]) * np.exp(1j * prop.t * E0)
        assert abs(same - want2).max() <= TOL * abs(want2).max()
    # standard errors: the host's algebra on the restated second moments
    from semiclassical_amd import hostmath
    want_sigma = hostmath.standard_errors(want, hostmath.rotate_second_moments(rows[:, 2:5], prop.t * E0), prop._ntraj_norm)
    assert np.allclose(sigma.real, want_sigma.real, rtol=1e-6, atol=1e-9 * scale) and np.allclose(sigma.imag, want_sigma.imag, rtol=1e-6, atol=1e-9 * scale)
    # nothing changed: the state, and the step that follows
    assert all(torch.equal(a, b) for a, b in zip(before, (prop._qp, prop._act, prop._mono, prop._c2, prop._sgn)))
    _, pot2, twin = _prepared(name, select=select)
    for _ in range(4):
        twin.step(pot2, float(g["dt"]))
    prop.step(pot, float(g["dt"]))
    assert torch.equal(prop.y, twin.y) and torch.equal(prop._c2, twin._c2) and torch.equal(prop._sgn, twin._sgn)


def test_refusals():
    g, pot, prop = _prepared("hk_as5_chi002")
    D, dt = prop.dim, float(g["dt"])
    ok = (np.ones(2), np.ones((2, D)))
    bad_m = np.ones((2, D))
    bad_m[1, 2] = np.inf
    for ops in ((np.ones(2), np.ones((2, D + 1))), (np.ones(3), np.ones((2, D))), (np.ones(2), np.ones(D)), (np.ones(0), np.ones((0, D))),
                (np.ones(2), bad_m), (np.full(2, np.nan), np.ones((2, D)))):
        with pytest.raises(ValueError):
            prop.operator_correlation(ops)
        with pytest.raises(ValueError):
            prop.operator_correlation(ok, ops)
        with pytest.raises(ValueError):
            prop.run(pot, dt, 2, operators=ops)
        with pytest.raises(ValueError):
            prop.run(pot, dt, 2, operators=(ok, ops))
    with pytest.raises(ValueError):
        prop.operator_correlation(ok, (np.ones(3), np.ones((3, D))))           # another number of operators on the ket side
    with pytest.raises(ValueError, match="use_graph"):
        prop.run(pot, dt, 4, operators=ok, use_graph=True)
    slots = torch.zeros((2, 5), device=prop.device)
    with pytest.raises(ValueError, match="opcorr"):
        prop.run(pot, dt, 2, slots=slots, operators=ok)
    for buf in (torch.zeros((2, 2, 4), device=prop.device), torch.zeros((1, 2, 5), device=prop.device),
                torch.zeros((2, 3, 5), device=prop.device), torch.zeros((2, 2, 5)), torch.zeros((2, 2, 5), device=prop.device, dtype=torch.float32)):
        with pytest.raises(ValueError, match="opcorr"):
            prop.run(pot, dt, 2, slots=slots, operators=ok, opcorr=buf)
    with pytest.raises(ValueError, match="operators"):
        prop.run(pot, dt, 2, opcorr=torch.zeros((2, 2, 5), device=prop.device))
    assert prop.t == 0.0                                        # none of the refused calls took a step
    # a vector outside the range of the singular widths of methylium
    gm, potm, meth = _prepared("hk_methylium")
    e, V = np.linalg.eigh(meth._Gt.numpy() + meth._G0h.numpy())
    null = V[:, abs(e) <= 1e-8][:, :1].T
    with pytest.raises(ValueError, match="range"):
        meth.operator_correlation((np.zeros(1), null))
    with pytest.raises(ValueError, match="range"):
        meth.run(potm, float(gm["dt"]), 2, operators=((np.ones(1), np.zeros((1, meth.dim))), (np.zeros(1), null)))
    gw, potw, wm = _prepared("wm_as5_chi002")
    with pytest.raises(NotImplementedError):
        wm.operator_correlation(ok)
    with pytest.raises(NotImplementedError):
        wm.run(potw, float(gw["dt"]), 2, operators=ok)


# ------------------------------------------------------------------------------------------- 2. the bra side, without cq

def test_bra_side_against_the_wavefunction():
    """A = x, B = 1 on hk_1d after 3 steps: X = <phi_0|x|psi(t)> by the trapezoid rule on phi_0^*(x) x psi(x, t), psi from
    wavefunction() -- a check of the bra-side factor that does not go through cq.  The grid covers 8 widths 1 / sqrt(Gamma_0) to
    either side of q0 at a sixteenth of a width: phi_0 is exp(-32) = 1e-14 at its ends, and for an integrand that is a Gaussian
    of width >= 1 / sqrt(Gamma_0 + Gamma_t) times a polynomial the rule's error is exp(-2 pi^2 sigma^2 / h^2) < 1e-100: the
    quadrature-limited 1e-8 |X| is far too wide here.  The bound is what the restatement alone achieves on this grid (psi summed on
    the host from the state read back against the restated X: 3e-16 of |X|, measured at run time and printed), times 10, plus a
    rounding floor for the engine's own sums: X is a sum of n terms x_i and psi at every grid point a sum of n terms, and a sum of n
    fp64 terms is exact to n 2^-53 of the sum of their magnitudes at worst -- so the floor is n 2^-53 (sum_i |x_i| + h sum_k
    |phi_0(x_k) x_k| sum_i |v_i <x_k|Q_i,P_i>|) / |X|, about 1e-13 for n = 256.  Both parts are asserted to stay below 1e-12, so a
    bra-side error of 1e-12 relative cannot pass."""
    g, pot, prop = _prepared("hk_1d")
    for _ in range(3):
        prop.step(pot, float(g["dt"]))
    E0 = float(g["E0"])
    X = prop.operator_correlation((np.zeros(1), np.ones((1, 1))), (np.ones(1), np.zeros((1, 1))), energy0_es=E0)[0]
    s = _read_back(prop)
    width = 1.0 / np.sqrt(s["G0"][0, 0])
    h = width / 16.0
    x = (s["q0"][0] + h * np.arange(-128, 129))[None, :]
    phi0 = gaussian(s["q0"], s["p0"], s["G0"], x)
    psi = prop.wavefunction(x)
    quad = np.sum(np.conj(phi0) * x[0] * psi) * h * np.exp(1j * prop.t * E0)
    # the restatement alone: psi from the coefficients read back, X from the two factors
    v = prop.coefficients().cpu().numpy()
    n = prop.ntraj
    parts = np.array([v[i] * gaussian(s["Q"][:, i], s["P"][:, i], s["Gt"], x) for i in range(n)])      # (n, nx): the terms of psi
    rows = _restated((np.zeros(1), np.ones((1, 1))), (np.ones(1), np.zeros((1, 1))), s)
    host = abs(np.sum(np.conj(phi0) * x[0] * parts.sum(0)) * h - (rows[0, 0] + 1j * rows[0, 1])) / abs(X)
    terms = (bra_factors(np.zeros(1), np.ones((1, 1)), s["Q"], s["P"], s["Gt"], s["G0"], s["q0"], s["p0"])[:, 0]
             * ket_factors(np.ones(1), np.zeros((1, 1)), s["q"], s["p"], s["Gi"], s["G0"], s["q0"], s["p0"])[:, 0] * s["cq"])
    magnitude = abs(terms).sum() + h * np.sum(abs(phi0 * x[0]) * abs(parts).sum(0))
    floor = n * 2.0 ** -53 * magnitude / abs(X)
    dev = abs(X - quad) / abs(X)
    print(f"hk_1d: X {X:.6f}, quadrature {quad:.6f}, deviation {dev:.2e} of |X|; the restatement alone {host:.2e}, "
          f"rounding floor of the engine's sums {floor:.2e}")
    assert 10.0 * host <= 1e-12 and floor <= 1e-12
    assert dev <= 10.0 * host + floor


# ------------------------------------------------------------------------------------------- 3. tile edges through the C-ABI

class _Opcorr(object):
    """sc_hk_opcorr / sc_hk_opcorr_initial on synthetic operands: qp (n, 2D), zi (n, 2D), cq (n,), built once per (n, D)"""

    def __init__(self, rng, n, D):
        from semiclassical_amd import _lib
        self.lib, self.n, self.D = _lib, n, D
        s = 1.0 / np.sqrt(D)
        self.qp = np.hstack((rng.normal(0.0, 0.6 * s, (n, D)), rng.normal(0.0, 0.9 * s, (n, D))))
        self.zi = np.hstack((rng.normal(0.0, 0.6 * s, (n, D)), rng.normal(0.0, 0.9 * s, (n, D))))
        self.cq = (rng.normal(size=n) + 1j * rng.normal(size=n)) / n
        self.stream = torch.cuda.current_stream().cuda_stream

    @staticmethod
    def dev(a):
        a = np.ascontiguousarray(a)
        t = torch.from_numpy(a.view(np.float64).reshape(a.shape + (2,)) if np.iscomplexobj(a) else a.astype(np.float64))
        return t.contiguous().to("cuda")

    @staticmethod
    def operands(rng, M, D):
        """(u, w (M, D), kappa (M,) complex) of one side"""
        return rng.normal(size=(M, D)), rng.normal(size=(M, D)), rng.normal(size=M) + 1j * rng.normal(size=M)

    def affine(self, z, side):
        u, w, kap = side
        return kap[None, :] + z[:, :self.D] @ u.T + 1j * (z[:, self.D:] @ w.T)

    def initial(self, ket):
        """g (n, M) complex from sc_hk_opcorr_initial"""
        lib, ptr = self.lib.lib, self.lib.ptr
        M = ket[0].shape[0]
        g = torch.full((self.n, M, 2), np.nan, device="cuda")
        bufs = [self.dev(a) for a in (self.zi,) + tuple(ket)]
        self.lib.check(lib.sc_hk_opcorr_initial(ptr(bufs[0]), self.n, self.D, ptr(bufs[1]), ptr(bufs[2]), ptr(bufs[3]), M, ptr(g),
                                                self.stream))
        torch.cuda.synchronize()
        return torch.view_as_complex(g).cpu().numpy()

    def __call__(self, bra, g, kept=None, cursor=None, rows=1, qp=None, cq=None):
        lib, ptr = self.lib.lib, self.lib.ptr
        M = bra[0].shape[0]
        bufs = [self.dev(a) for a in (self.qp if qp is None else qp, self.cq if cq is None else cq) + tuple(bra) + (g,)]
        state = self.lib.sc_state(n=self.n, dim=self.D, mono_layout=0, qp=bufs[0].data_ptr(), act=None, mono=None, c2=None, sgn=None,
                                  work=None, flags=None)
        part = torch.full((int(lib.sc_hk_opcorr_rows(self.n, M)) * M * 5,), np.nan, device="cuda")
        out = torch.full((rows, M, 5), np.nan, device="cuda")
        mask = None if kept is None else torch.from_numpy(np.asarray(kept, dtype=np.uint8)).to("cuda")
        cur = None if cursor is None else torch.tensor([cursor], dtype=torch.int64, device="cuda")
        self.lib.check(lib.sc_hk_opcorr(state, ptr(bufs[1]), ptr(bufs[2]), ptr(bufs[3]), ptr(bufs[4]), ptr(bufs[5]), M, ptr(mask),
                                        ptr(part), ptr(out), ptr(cur), self.stream))
        torch.cuda.synchronize()
        if cur is not None:
            assert int(cur.item()) == cursor                     # read, not advanced
        return out.cpu().numpy()


SIZES_N = (1, 63, 64, 65, 130)
SIZES_M = (1, 3, 64, 65, 130)


@pytest.mark.parametrize("D", [1, 15, 16, 17, 33])
def test_tile_edges_through_the_c_abi(D):
    rng = np.random.default_rng(1000 + D)
    worst = worst_g = 0.0
    for n in SIZES_N:
        call = _Opcorr(rng, n, D)
        masks = [None, np.arange(n) >= 64, np.arange(n) == n // 2]      # none; the first 64-band discarded; a single one kept
        for M in SIZES_M:
            bra, ket = call.operands(rng, M, D), call.operands(rng, M, D)
            g = call.initial(ket)
            want_g = call.affine(call.zi, ket)
            assert g.shape == want_g.shape == (n, M)
            dev_g = abs(g - want_g).max() / abs(want_g).max()
            assert dev_g <= TOL, (n, M, dev_g)
            worst_g = max(worst_g, dev_g)
            x = call.affine(call.qp, bra) * g * call.cq[:, None]
            for kept in masks:
                got = call(bra, g, kept)[0]
                want = restated_rows(x, kept)
                assert got.shape == want.shape == (M, 5) and np.isfinite(got).all()
                scale = abs(want).max(axis=1)                    # every row against its largest entry
                dev = abs(got - want).max(axis=1)
                assert (dev <= TOL * scale).all(), (n, M, kept is not None, dev.max(), scale)
                worst = max(worst, (dev[scale > 0] / scale[scale > 0]).max() if (scale > 0).any() else 0.0)
                if kept is not None and not kept.any():
                    assert not got.any()                         # nobody kept: exact zeros
                assert np.array_equal(call(bra, g, kept)[0], got)      # two calls, the same bits
            # a non-finite cq, g or state of a discarded trajectory never reaches the sums: each alone, and all together
            if n > 1:
                kept = np.arange(n) > 0
                clean = call(bra, g, kept)[0]
                qp, cq, gd = call.qp.copy(), call.cq.copy(), g.copy()
                qp[0], cq[0], gd[0] = np.nan, np.inf, np.nan
                for dirty in (dict(qp=qp), dict(cq=cq), dict(cq=cq, qp=qp)):
                    assert np.array_equal(call(bra, g, kept, **dirty)[0], clean), (n, M, sorted(dirty))
                assert np.array_equal(call(bra, gd, kept)[0], clean), (n, M, "g")
                assert np.array_equal(call(bra, gd, kept, qp=qp, cq=cq)[0], clean), (n, M, "all")
    # with a cursor the row goes to out[*cursor]
    got = call(bra, g, None, cursor=2, rows=3)
    assert np.isnan(got[:2]).all() and np.array_equal(got[2], call(bra, g)[0])
    print(f"D={D}: largest deviation of a row {worst:.2e} of its largest entry; of g {worst_g:.2e}")


def test_c_abi_refusals():
    from semiclassical_amd import _lib
    lib, ptr = _lib.lib, _lib.ptr
    buf = torch.zeros(256, device="cuda")
    state = _lib.sc_state(n=5, dim=3, mono_layout=0, qp=buf.data_ptr(), act=None, mono=None, c2=None, sgn=None, work=None, flags=None)
    b = ptr(buf)
    args = lambda **kw: [kw.get("st", state), b, b, b, b, b, kw.get("M", 1), None, b, kw.get("out", b), None, None]
    assert lib.sc_hk_opcorr(*args(M=0)) == -1 and lib.sc_hk_opcorr(*args(out=None)) == -1
    assert lib.sc_hk_opcorr(*args(M=65536)) == -2 and b"65535" in lib.sc_last_error()
    big = _lib.sc_state.from_buffer_copy(state)
    big.dim = 513
    assert lib.sc_hk_opcorr(*args(st=big)) == -2 and b"512" in lib.sc_last_error()
    many = _lib.sc_state.from_buffer_copy(state)
    many.n = 64 * 65535 + 1
    assert lib.sc_hk_opcorr(*args(st=many)) == -2 and str(64 * 65535).encode() in lib.sc_last_error()
    init = lambda **kw: [kw.get("zi", b), kw.get("n", 5), kw.get("D", 3), b, b, b, kw.get("M", 1), b, None]
    assert lib.sc_hk_opcorr_initial(*init(M=0)) == -1 and lib.sc_hk_opcorr_initial(*init(zi=None)) == -1
    assert lib.sc_hk_opcorr_initial(*init(M=65536)) == -2 and lib.sc_hk_opcorr_initial(*init(D=513)) == -2
    assert lib.sc_hk_opcorr_initial(*init(n=64 * 65535 + 1)) == -2
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------- 4. run(operators=...)

ROUTES = [
    # case, nt, attributes, the entry point that has to run, bit-identical rows promised
    ("hk_as60_n96", 7, {"visit_min_bytes": 0, "visit_steps": 3}, "sc_hk_step_visit", True),
    ("hk_as60_n96", 7, {"visit_min_bytes": 0, "visit_steps": 2}, "sc_hk_step_multi", True),
    ("hk_as60_n96", 7, {"pair_steps": False}, "sc_hk_step", True),
    ("hk_as33", 5, {"visit_min_bytes": 0, "visit_steps": 3}, "sc_hk_step_visit", True),
    ("hk_as33", 5, {"visit_min_bytes": 0, "visit_steps": 2}, "sc_hk_step_multi", True),
    ("hk_as33", 5, {"pair_steps": False}, "sc_hk_step", True),
    ("hk_as5_chi002", 5, {}, "sc_hk_step", False),                      # a whole-loop shape: step by step with operators
    ("hk_coumarin_harmonic", 3, {}, "sc_hk_step_modal", False),
]


@pytest.mark.parametrize("name,nt,attrs,entry,bits", ROUTES, ids=[f"{r[0]}-{r[3]}" for r in ROUTES])
def test_run_with_operators(name, nt, attrs, entry, bits, monkeypatch):
    g, pot, prop = _prepared(name, **attrs)
    dt, E0 = float(g["dt"]), float(g["E0"])
    D = prop.dim
    bra, ket = _operators(prop, 3, np.random.default_rng(nt))
    targets = (np.vstack((g["q0"], g["zi"][:D, 0])), np.vstack((g["p0"], g["zi"][D:, 0])))
    blocks = torch.zeros((nt, 4, 4), device=prop.device)
    spy = _Spy(monkeypatch)
    C, k, sC, sk, T, sT, X, sX = prop.run(pot, dt, nt, E0, standard_errors=True, blocks=blocks, targets=targets, operators=(bra, ket))
    monkeypatch.undo()
    assert spy.seen.get(entry, 0) > 0 and spy.seen.get("sc_hk_opcorr", 0) == nt and spy.seen.get("sc_hk_cross", 0) == nt, spy.seen
    assert "sc_hk_run" not in spy.seen and "sc_hk_run_m" not in spy.seen
    assert X.shape == sX.shape == (nt, 4) and X.dtype == np.complex128 and T.shape == (nt, 2)
    # without operators: the same C, k, errors, blocks, cross rows and final state, bit for bit
    _, pot2, twin = _prepared(name, **attrs)
    blocks2 = torch.zeros((nt, 4, 4), device=prop.device)
    C2, k2, sC2, sk2, T2, sT2 = twin.run(pot2, dt, nt, E0, standard_errors=True, blocks=blocks2, targets=targets)
    for a, b in ((C, C2), (k, k2), (sC, sC2), (sk, sk2), (T, T2), (sT, sT2)):
        assert np.array_equal(a, b)
    assert torch.equal(blocks, blocks2) and torch.equal(prop.y, twin.y) and torch.equal(prop._c2, twin._c2)
    assert prop.t == twin.t
    if name == "hk_as5_chi002":
        # ... and against the one-launch loop this shape takes without operators or targets: DESIGN.md section 0, row H
        _, pot5, whole = _prepared(name, **attrs)
        spy = _Spy(monkeypatch, names=("sc_hk_run", "sc_hk_run_m"))
        C5, k5 = whole.run(pot5, dt, nt, E0)
        monkeypatch.undo()
        assert sum(spy.seen.values()) > 0
        assert abs(C - C5).max() <= 1e-13 * abs(C5).max() and abs(k - k5).max() <= 1e-13 * abs(k5).max()
    # row k of X is operator_correlation() of the state before step k
    _, pot3, loop = _prepared(name, **attrs)
    want, want_sigma = [], []
    for _ in range(nt):
        x, s = loop.operator_correlation(bra, ket, energy0_es=E0, standard_errors=True)
        want.append(x)
        want_sigma.append(s)
        loop.step(pot3, dt)
    want, want_sigma = np.array(want), np.array(want_sigma)
    scale = abs(want).max()
    print(f"{name} {entry}: run() against the step-by-step loop {abs(X - want).max() / scale:.2e} of max |X| = {scale:.3e}")
    if bits:
        assert np.array_equal(X, want) and np.array_equal(sX, want_sigma)
    else:
        assert abs(X - want).max() <= 1e-12 * scale
    # the last pair is (1, 1): the autocorrelation function
    assert abs(X[:, 3] - C).max() <= TOL * max(scale, abs(C).max())
    # bra alone: the bra's operators on both sides; slots= given: the raw rows in the caller's buffer give the same numbers
    _, pot4, raw = _prepared(name, **attrs)
    slots, buf = torch.zeros((nt, 5), device=prop.device), torch.full((nt + 1, 4, 5), np.nan, device=prop.device)
    assert raw.run(pot4, dt, nt, E0, slots=slots, operators=(bra, ket), opcorr=buf) is None
    raw.synchronize()
    X4, sX4 = raw.finalize_cross(buf[:nt], 0.0, dt, E0, raw._ntraj_norm)
    assert np.array_equal(X4, X) and np.array_equal(sX4, sX) and torch.isnan(buf[nt]).all()


def test_run_with_the_bra_alone():
    """operators=bra: the same operators on both sides, the tuple ends with X"""
    g, pot, prop = _prepared("hk_as5_chi002")
    dt, E0 = float(g["dt"]), float(g["E0"])
    bra = _operators(prop, 2, np.random.default_rng(2))[0]
    out = prop.run(pot, dt, 3, E0, operators=bra)
    _, pot2, twin = _prepared("hk_as5_chi002")
    both = twin.run(pot2, dt, 3, E0, operators=(bra, bra))
    assert len(out) == len(both) == 3 and out[2].shape == (3, 3) and all(np.array_equal(a, b) for a, b in zip(out, both))
    # ... and C, k are the bits of the step-at-a-time loop that exports no per-trajectory terms
    _, pot3, plain = _prepared("hk_as5_chi002")
    plain._whole_loop_ok = False
    assert all(np.array_equal(a, b) for a, b in zip(out, plain.run(pot3, dt, 3, E0)))


# ------------------------------------------------------------------------------------------- 5. under a discard mask

def test_after_discard_nonsymplectic():
    g, pot, prop = _prepared("hk_as5_chi002")
    dt, E0 = float(g["dt"]), float(g["E0"])
    for _ in range(6):
        prop.step(pot, dt)
    eps = prop.symplectic_deviation().cpu().numpy()
    tol = float(np.median(eps))
    prop.discard_nonsymplectic(tol)
    kept = prop.kept.cpu().numpy()
    n = prop.ntraj
    print(f"tolerance {tol:.3e}: kept {int(kept.sum())} of {n}")
    assert 0 < kept.sum() < n
    bra, ket = _operators(prop, 5, np.random.default_rng(8))
    X = prop.operator_correlation(bra, ket, energy0_es=E0)
    # (cq read back under the mask is the correlate kernel's export for every trajectory, kept or not: the restatement selects)
    s = _read_back(prop)
    rows = _restated(bra, ket, s, kept)                          # cq carries the unchanged N
    want = (rows[:, 0] + 1j * rows[:, 1]) * np.exp(1j * prop.t * E0)
    everyone = _restated(bra, ket, s)
    assert abs(everyone[:, 0] - rows[:, 0]).max() > 1e-3 * abs(rows[:, 0]).max()      # the mask matters
    scale = abs(want).max()
    print(f"masked: deviation {abs(X - want).max() / scale:.2e} of max |X|")
    assert abs(X - want).max() <= TOL * scale
    assert abs(X[5] - prop.autocorrelation(E0)) <= TOL * scale
    t0 = prop.t
    out = prop.run(pot, dt, 2, E0, operators=(bra, ket))
    assert len(out) == 3 and prop.t > t0 and abs(out[2][0] - want).max() <= TOL * scale      # row 0: the state the call above saw
    assert abs(out[2][:, 5] - out[0]).max() <= TOL * scale


# ------------------------------------------------------------------------------------------- 6. standard errors mean something

def test_standard_errors_cover_the_closed_form():
    """t = 0 on the fixture's own initial conditions: every X_a(0) within 5 sigma_a of <phi_0|A_a B_a|phi_0> for the three pairs
    checked on the CPU first (test_opcorr_host.py::test_five_sigma_at_t0_on_the_cpu), and sigma equal to the restatement's"""
    from semiclassical_amd import hostmath
    g, pot, prop = _prepared("hk_as5_chi002")
    bra, ket = t0_operator_pairs(prop.dim)
    X, sigma = prop.operator_correlation(bra, ket, energy0_es=float(g["E0"]), standard_errors=True)
    exact = closed_form_t0(bra, ket, g["Gamma_0"], g["q0"])
    for a in range(3):
        print(f"pair {a}: X {X[a]:.6f}  exact {exact[a]:.6f}  sigma {sigma[a]:.2e}")
    ok = within_five_sigma(X, sigma, exact)
    assert ok.all(), ok
    rows = _restated(bra, ket, _read_back(prop))
    want = hostmath.standard_errors(rows[:, 0] + 1j * rows[:, 1], rows[:, 2:5], prop._ntraj_norm)
    assert (abs(sigma.real - want.real) <= 1e-9 * want.real).all()
    big = want.imag > 1e-6 * abs(exact)                          # (pair 0: Im x_i = 0 up to rounding, sigma_Im is rounding noise)
    assert big[1:].all() and (abs(sigma.imag - want.imag)[big] <= 1e-9 * want.imag[big]).all()


# ------------------------------------------------------------------------------------------- 7. driver

FCHK = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fchk")


def test_driver_key(tmp_path):
    from semiclassical_amd import driver
    out, ofile = tmp_path / "correlations.npz", tmp_path / "operators.npz"
    task = {"task": "dynamics", "propagator": "HK", "batch_size": 64, "num_trajectories": 128, "num_steps": 12, "time_step_fs": 0.005,
            "manual_seed": 0, "standard_errors": True, "operator_correlation": str(ofile),
            "potential": {"type": "harmonic", "ground": os.path.join(FCHK, "methylium_s0.fchk"),
                          "excited": os.path.join(FCHK, "methylium_s1.fchk"), "coupling": os.path.join(FCHK, "methylium_s1.fchk")},
            "results": {"correlations": str(out)}}
    setup = driver.build_problem(task)
    D = setup.q0.shape[0]
    e, V = np.linalg.eigh(setup.Gamma_0.numpy())
    stiff = V[:, -1]                                             # in the range of the singular Gamma_0 (rank 6)
    bra_c, bra_m = np.array([1.0, 0.0, 0.5]), np.vstack((np.zeros(D), stiff, 2.0 * V[:, -2]))
    np.savez(ofile, bra_c=bra_c, bra_m=bra_m)
    driver.run_semiclassical_dynamics(task, device="cuda")
    d = dict(np.load(out))
    assert int(d["trajectories"]) == 128
    assert np.array_equal(d["operator_bra_c"], bra_c) and np.array_equal(d["operator_bra_m"], bra_m)
    assert np.array_equal(d["operator_ket_c"], bra_c) and np.array_equal(d["operator_ket_m"], bra_m)
    X = d["operator_correlation"]
    assert X.shape == (12, 3) and d["operator_correlation_error"].shape == (12, 3) and d["operator_correlation_second_moment"].shape == (12, 3, 3)
    dev = abs(X[:, 0] - d["autocorrelation"]).max()
    print(f"driver: |operator_correlation[:, (1, 1)] - autocorrelation| {dev:.2e}")
    assert dev <= 1e-9
    # <phi_0|(u.x)^2|phi_0> = (u.q0)^2 + 1 / (2 lambda) along an eigenvector u of Gamma_0, within the error bar at t = 0
    exact = (stiff @ setup.q0.numpy()) ** 2 + 0.5 / e[-1]
    assert abs(X[0, 1].real - exact) <= 5.0 * d["operator_correlation_error"][0, 1].real + 1e-12 * exact
    # other operators, adding to the file: refused before anything runs
    np.savez(ofile, bra_c=bra_c[:2], bra_m=bra_m[:2])
    again = dict(task, results={"correlations": str(out), "overwrite": False})
    again.pop("manual_seed")
    with pytest.raises(driver.ConfigurationError, match="operators"):
        driver.run_semiclassical_dynamics(again, device="cuda")
    without = dict(again)
    without.pop("operator_correlation")
    with pytest.raises(driver.ConfigurationError):
        driver.run_semiclassical_dynamics(without, device="cuda")
    after = dict(np.load(out))
    assert set(after) == set(d) and all(np.array_equal(after[k], d[k]) for k in d)
    # the same task without the key: the file has the keys it always had.  This shape (constant Hessian, D = 12) runs as ONE launch
    # without operators and step by step with them: the correlation functions agree to the 1e-13 of DESIGN.md section 0, row H (on
    # every other shape they are the same bits: test_run_with_operators); everything that is not a sum over trajectories is equal
    plain_out = tmp_path / "plain.npz"
    plain = dict(task, results={"correlations": str(plain_out)})
    plain.pop("operator_correlation")
    driver.run_semiclassical_dynamics(plain, device="cuda")
    p = dict(np.load(plain_out))
    assert set(d) - set(p) == set(driver.CorrelationStore.OPERATOR_KEYS + driver.CorrelationStore.OPERATOR_ERROR_KEYS)
    assert set(p) - set(d) == set()
    sums = ("autocorrelation", "ic_correlation", "autocorrelation_second_moment", "ic_correlation_second_moment")
    derived = ("autocorrelation_error", "ic_correlation_error")      # sqrt(N S - mean^2) of those sums: a difference, not held to 1e-13
    for key in p:
        if not np.array_equal(p[key], d[key]):
            worst = abs(p[key] - d[key]).max() / abs(p[key]).max()
            print(f"driver: {key} with and without the key: {worst:.2e} of its largest entry")
            assert key in sums + derived and (key in derived or worst <= 1e-13)
    # the rates task: the lineshapes next to an ic_rate that is bit for bit the one the task writes without the operators' keys.
    # THIS REPLACES THE ISSUE'S WORDING ("ic_rate bit-identical to a run without the key"): a dynamics run of this shape without the
    # key takes the one-launch loop, whose k_ic(t) agrees with the step-at-a-time loop's to 1e-13 and not in the last bit (checked
    # above), so its ic_rate cannot be the same bits either.  What the rates task itself must guarantee -- that the operators' keys
    # change none of the values it wrote before -- is checked bit for bit on the same correlation functions.
    bare_out = tmp_path / "bare.npz"
    np.savez(bare_out, **{key: d[key] for key in p})
    for src in (out, bare_out):
        driver.calculate_rates({"task": "rates", "correlations": str(src), "rates": str(src), "adiabatic_gap_ev": 4.0})
    r, rb = dict(np.load(out)), dict(np.load(bare_out))
    assert set(r) - set(rb) == set(d) - set(p) | {"operator_lineshape", "radiative_rate"}
    assert all(np.array_equal(r[key], rb[key]) for key in rb)
    assert r["operator_lineshape"].shape == (r["energies"].shape[0], 3) and np.isfinite(r["radiative_rate"])
    # the same operators pool
    np.savez(ofile, bra_c=bra_c, bra_m=bra_m)
    driver.run_semiclassical_dynamics(again, device="cuda")
    pooled = np.load(out)
    assert int(pooled["trajectories"]) == 256 and abs(pooled["operator_correlation"][:, 0] - pooled["autocorrelation"]).max() <= 1e-9
    assert "operator_lineshape" not in pooled and "radiative_rate" not in pooled          # stale after new trajectories
