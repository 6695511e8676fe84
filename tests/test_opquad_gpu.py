"""HermanKlukPropagator.operator_correlation / run(operators=...) with QUADRATIC operators (sc_hk_opquad)
against the numpy restatement of the definition (tests/test_opquad_host.py, the direct formula without an eigendecomposition): the
engine on the golden cases, the bra side against quadrature of the wavefunction, the tile edges and the refusals through the C-ABI,
every route of run(), the discard mask, the standard errors and the driver key."""
import numpy as np
import pytest
import torch

from tests.lib_spy import LibSpy as _Spy
from tests.test_cross_host import gaussian
from tests.test_opcorr_gpu import FCHK, ROUTES, TOL, _prepared, _read_back
from tests.test_opcorr_host import project, restated_rows
from tests.test_opquad_host import (bra_factors, closed_form_t0, ket_factors, random_symmetric, restated_opquad, t0_operator_pairs,
                                    within_five_sigma)

pytestmark = pytest.mark.gpu
torch.set_default_dtype(torch.float64)


def _restated(bra, ket, s, kept=None):
    return restated_opquad(bra, ket, s["Q"], s["P"], s["q"], s["p"], s["cq"], s["Gi"], s["Gt"], s["G0"], s["q0"], s["p0"], kept)


BRA_RANKS, KET_RANKS = (1, 2, None, 0), (0, 1, None, 2)      # None: D


def _operators(prop, rng, scale=1.0):
    """M = 4 random pairs (c, m, K): K random symmetric of the ranks above (at most D), m and K projected onto the range of their
    side's widths (the identity for regular ones)"""
    D = prop.dim
    Gi, Gt, G0 = prop._Gi.numpy(), prop._Gt.numpy(), prop._G0h.numpy()
    sides = []
    for ranks, Ga, Gb in ((BRA_RANKS, G0, Gt), (KET_RANKS, Gi, G0)):
        K = np.array([scale * random_symmetric(rng, D, D if r is None else min(r, D), Ga, Gb) for r in ranks])
        sides.append((rng.normal(size=4), project(rng.normal(size=(4, D)), Ga, Gb), K))
    return tuple(sides)


# ------------------------------------------------------------------------------------------- 8. engine vs restatement

ENGINE_CASES = ["hk_1d", "hk_as5_chi002", "hk_as33", "hk_as60_n96", "hk_methylium", "hk_coumarin_harmonic"]


@pytest.mark.parametrize("name", ENGINE_CASES)
def test_engine_matches_restatement(name):
    """measured on the MI355X (deviation / max |X|): see DESIGN.md section 4.16"""
    select = slice(0, 45) if name == "hk_as33" else None
    g, pot, prop = _prepared(name, select=select)
    for _ in range(3):
        prop.step(pot, float(g["dt"]))
    bra, ket = _operators(prop, np.random.default_rng(len(name)))
    E0 = float(g["E0"])
    before = [t.clone() for t in (prop._qp, prop._act, prop._mono, prop._c2, prop._sgn)]
    X, sigma = prop.operator_correlation(bra, ket, energy0_es=E0, standard_errors=True)
    assert X.shape == sigma.shape == (4,) and X.dtype == np.complex128
    assert np.array_equal(prop.operator_correlation(bra, ket, energy0_es=E0), X)          # the same bits in every call
    rows = _restated(bra, ket, _read_back(prop))
    want = (rows[:, 0] + 1j * rows[:, 1]) * np.exp(1j * prop.t * E0)
    scale = abs(want).max()
    print(f"{name}: |X_a| {np.array2string(abs(want), precision=3)}, deviation {abs(X - want).max() / scale:.2e} of the largest")
    assert scale > 0 and abs(X - want).max() <= TOL * scale
    # ket=None: the operators of the bra on both sides, K included
    if np.array_equal(g["Gamma_i"], g["Gamma_t"]):
        same = prop.operator_correlation(bra, energy0_es=E0)
        rows2 = _restated(bra, bra, _read_back(prop))
        want2 = (rows2[:, 0] + 1j * rows2[:, 1]) * np.exp(1j * prop.t * E0)
        assert abs(same - want2).max() <= TOL * abs(want2).max()
    from semiclassical_amd import hostmath
    want_sigma = hostmath.standard_errors(want, hostmath.rotate_second_moments(rows[:, 2:5], prop.t * E0), prop._ntraj_norm)
    assert np.allclose(sigma.real, want_sigma.real, rtol=1e-6, atol=1e-9 * scale) and np.allclose(sigma.imag, want_sigma.imag, rtol=1e-6, atol=1e-9 * scale)
    # nothing changed
    assert all(torch.equal(a, b) for a, b in zip(before, (prop._qp, prop._act, prop._mono, prop._c2, prop._sgn)))


def test_refusals():
    g, pot, prop = _prepared("hk_as5_chi002")
    D, dt = prop.dim, float(g["dt"])
    c, m, K = np.ones(2), np.ones((2, D)), np.array([np.eye(D)] * 2)
    skew, broken = K.copy(), K.copy()
    skew[1, 0, 1] = 1e-6
    broken[0, 1, 1] = np.inf
    for ops in ((c, m, skew), (c, m, broken), (c, m, K[:, 0]), (c, m, np.concatenate((K, K[:1]))), (c, m, K[:1])):
        with pytest.raises(ValueError):
            prop.operator_correlation(ops)
        with pytest.raises(ValueError):
            prop.operator_correlation((c, m), ops)
        with pytest.raises(ValueError):
            prop.run(pot, dt, 2, operators=((c, m, K), ops))
    with pytest.raises(ValueError):
        prop.operator_correlation((c, m, K), (np.ones(3), np.ones((3, D)), None))           # a ket with another M
    with pytest.raises(ValueError, match="use_graph"):
        prop.run(pot, dt, 4, operators=(c, m, K), use_graph=True)
    assert prop.t == 0.0
    gm, potm, meth = _prepared("hk_methylium")
    e, V = np.linalg.eigh(meth._Gt.numpy() + meth._G0h.numpy())
    null = V[:, abs(e) <= 1e-8][:, 0]
    Dm = meth.dim
    with pytest.raises(ValueError, match="range"):
        meth.operator_correlation((np.zeros(1), np.zeros((1, Dm)), np.outer(null, null)[None]))
    gw, potw, wm = _prepared("wm_as5_chi002")
    with pytest.raises(NotImplementedError):
        wm.operator_correlation((c, m, K))
    with pytest.raises(NotImplementedError):
        wm.run(potw, float(gw["dt"]), 2, operators=(c, m, K))


# ------------------------------------------------------------------------------------------- 9. the bra side, without cq

def test_bra_side_against_the_wavefunction():
    """A = x^2, B = 1 on hk_1d after 3 steps: X = <phi_0|x^2|psi(t)> by the trapezoid rule on phi_0^*(x) x^2 psi(x, t), psi from
    wavefunction(), on the grid of tests/test_opcorr_gpu.py::test_bra_side_against_the_wavefunction (8 widths of phi_0 to either
    side at a sixteenth of a width), and the bound derived as there: ten times what the restatement alone reaches on this grid
    (psi summed on the host from the state read back against the restated X, measured at run time and printed), plus the rounding
    floor n 2^-53 (sum_i |x_i| + h sum_k |phi_0(x_k) x_k^2| sum_i |v_i <x_k|Q_i,P_i>|) / |X| of the engine's own sums of n terms.
    Both parts are asserted to stay below 1e-12."""
    g, pot, prop = _prepared("hk_1d")
    for _ in range(3):
        prop.step(pot, float(g["dt"]))
    E0 = float(g["E0"])
    bra, ket = (np.zeros(1), np.zeros((1, 1)), np.full((1, 1, 1), 2.0)), (np.ones(1), np.zeros((1, 1)), np.zeros((1, 1, 1)))
    X = prop.operator_correlation(bra, ket, energy0_es=E0)[0]
    s = _read_back(prop)
    width = 1.0 / np.sqrt(s["G0"][0, 0])
    h = width / 16.0
    x = (s["q0"][0] + h * np.arange(-128, 129))[None, :]
    phi0 = gaussian(s["q0"], s["p0"], s["G0"], x)
    psi = prop.wavefunction(x)
    quad = np.sum(np.conj(phi0) * x[0] ** 2 * psi) * h * np.exp(1j * prop.t * E0)
    v = prop.coefficients().cpu().numpy()
    n = prop.ntraj
    parts = np.array([v[i] * gaussian(s["Q"][:, i], s["P"][:, i], s["Gt"], x) for i in range(n)])      # (n, nx): the terms of psi
    rows = _restated(bra, ket, s)
    host = abs(np.sum(np.conj(phi0) * x[0] ** 2 * parts.sum(0)) * h - (rows[0, 0] + 1j * rows[0, 1])) / abs(X)
    terms = (bra_factors(*bra, s["Q"], s["P"], s["Gt"], s["G0"], s["q0"], s["p0"])[:, 0]
             * ket_factors(*ket, s["q"], s["p"], s["Gi"], s["G0"], s["q0"], s["p0"])[:, 0] * s["cq"])
    magnitude = abs(terms).sum() + h * np.sum(abs(phi0 * x[0] ** 2) * abs(parts).sum(0))
    floor = n * 2.0 ** -53 * magnitude / abs(X)
    dev = abs(X - quad) / abs(X)
    print(f"hk_1d: X {X:.6f}, quadrature {quad:.6f}, deviation {dev:.2e} of |X|; the restatement alone {host:.2e}, "
          f"rounding floor of the engine's sums {floor:.2e}")
    assert 10.0 * host <= 1e-12 and floor <= 1e-12
    assert dev <= 10.0 * host + floor


# ------------------------------------------------------------------------------------------- 10. tile edges through the C-ABI

class _Opquad(object):
    """sc_hk_opquad / sc_hk_opquad_initial on synthetic operands: qp (n, 2D), zi (n, 2D), cq (n,), built once per (n, D)"""

    def __init__(self, rng, n, D):
        from semiclassical_amd import _lib
        self.lib, self.n, self.D = _lib, n, D
        s = 1.0 / np.sqrt(D)
        self.qp = np.hstack((rng.normal(0.0, 0.6 * s, (n, D)), rng.normal(0.0, 0.9 * s, (n, D))))
        self.zi = np.hstack((rng.normal(0.0, 0.6 * s, (n, D)), rng.normal(0.0, 0.9 * s, (n, D))))
        self.cq = (rng.normal(size=n) + 1j * rng.normal(size=n)) / n
        self.stream = torch.cuda.current_stream().cuda_stream
        self.d_qp, self.d_zi, self.d_cq = self.dev(self.qp), self.dev(self.zi), self.dev(self.cq)

    @staticmethod
    def dev(a):
        a = np.ascontiguousarray(a)
        t = torch.from_numpy(a.view(np.float64).reshape(a.shape + (2,)) if np.iscomplexobj(a) else a.astype(np.float64))
        return t.contiguous().to("cuda")

    @staticmethod
    def operands(rng, M, R, D, unit=False):
        """(u, w (M, 1 + R, D), kappa (M, 1 + R) complex, lam (M, 1 + R)) of one side; ``unit``: lam = 1"""
        lam = np.ones((M, 1 + R)) if unit else rng.normal(size=(M, 1 + R))
        return (rng.normal(size=(M, 1 + R, D)), rng.normal(size=(M, 1 + R, D)), rng.normal(size=(M, 1 + R)) + 1j * rng.normal(size=(M, 1 + R)),
                lam)

    def value(self, z, side):
        """sum over the columns of lam z^p: (n, M)"""
        u, w, kap, lam = side
        zc = kap[None] + np.einsum('acd,nd->nac', u, z[:, :self.D]) + 1j * np.einsum('acd,nd->nac', w, z[:, self.D:])
        return lam[None, :, 0] * zc[:, :, 0] + (lam[None, :, 1:] * zc[:, :, 1:] ** 2).sum(2)

    def initial(self, ket):
        """g (n, M) complex from sc_hk_opquad_initial"""
        lib, ptr = self.lib.lib, self.lib.ptr
        M, RB = ket[3].shape[0], ket[3].shape[1] - 1
        g = torch.full((self.n, M, 2), np.nan, device="cuda")
        bufs = [self.dev(a) for a in ket]
        self.lib.check(lib.sc_hk_opquad_initial(ptr(self.d_zi), self.n, self.D, ptr(bufs[0]), ptr(bufs[1]), ptr(bufs[2]), ptr(bufs[3]), M,
                                                RB, ptr(g), self.stream))
        torch.cuda.synchronize()
        return torch.view_as_complex(g).cpu().numpy()

    def bra(self, side):
        """the bra's columns on the device, for the calls that follow"""
        self.side = [self.dev(a) for a in side]
        self.M, self.RA = side[3].shape[0], side[3].shape[1] - 1

    def __call__(self, g, kept=None, cursor=None, rows=1, qp=None, cq=None, linear=False):
        lib, ptr = self.lib.lib, self.lib.ptr
        M, b = self.M, self.side
        d_qp, d_cq, d_g = self.d_qp if qp is None else self.dev(qp), self.d_cq if cq is None else self.dev(cq), self.dev(g)
        state = self.lib.sc_state(n=self.n, dim=self.D, mono_layout=0, qp=d_qp.data_ptr(), act=None, mono=None, c2=None, sgn=None,
                                  work=None, flags=None)
        part = torch.full((int(lib.sc_hk_opquad_rows(self.n, M)) * M * 5,), np.nan, device="cuda")
        out = torch.full((rows, M, 5), np.nan, device="cuda")
        mask = None if kept is None else torch.from_numpy(np.asarray(kept, dtype=np.uint8)).to("cuda")
        cur = None if cursor is None else torch.tensor([cursor], dtype=torch.int64, device="cuda")
        if linear:                                               # sc_hk_opcorr on the same operands (RA = 0)
            self.lib.check(lib.sc_hk_opcorr(state, ptr(d_cq), ptr(b[0]), ptr(b[1]), ptr(b[2]), ptr(d_g), M, ptr(mask), ptr(part),
                                            ptr(out), ptr(cur), self.stream))
        else:
            self.lib.check(lib.sc_hk_opquad(state, ptr(d_cq), ptr(b[0]), ptr(b[1]), ptr(b[2]), ptr(b[3]), ptr(d_g), M, self.RA, ptr(mask),
                                            ptr(part), ptr(out), ptr(cur), self.stream))
        torch.cuda.synchronize()
        if cur is not None:
            assert int(cur.item()) == cursor                     # read, not advanced
        return out.cpu().numpy()


SIZES_N = (1, 63, 64, 65, 130)
SHAPES_MR = ((1, 0), (1, 1), (3, 2), (1, 62), (1, 63), (1, 64), (1, 130), (2, 31), (2, 32), (5, 12), (65, 1), (130, 0))
RANKS_KET = (0, 3)


@pytest.mark.parametrize("D", [1, 15, 16, 17, 33])
def test_tile_edges_through_the_c_abi(D):
    rng = np.random.default_rng(2000 + D)
    worst = worst_g = worst_lin = 0.0
    for n in SIZES_N:
        call = _Opquad(rng, n, D)
        masks = [None, np.arange(n) >= 64, np.arange(n) == n // 2]      # none; the first 64-band discarded; a single one kept
        for M, RA in SHAPES_MR:
            bra = call.operands(rng, M, RA, D, unit=RA == 0)
            call.bra(bra)
            f = call.value(call.qp, bra)
            for RB in RANKS_KET:
                ket = call.operands(rng, M, RB, D, unit=RB == 0)
                g = call.initial(ket)
                want_g = call.value(call.zi, ket)
                assert g.shape == want_g.shape == (n, M)
                dev_g = abs(g - want_g).max() / abs(want_g).max()
                assert dev_g <= 1e-12, (n, M, RB, dev_g)
                worst_g = max(worst_g, dev_g)
                x = f * g * call.cq[:, None]
                for kept in masks:
                    got = call(g, kept)[0]
                    want = restated_rows(x, kept)
                    assert got.shape == want.shape == (M, 5) and np.isfinite(got).all()
                    scale = abs(want).max(axis=1)                # every row against its largest entry
                    dev = abs(got - want).max(axis=1)
                    assert (dev <= TOL * scale).all(), (n, M, RA, RB, kept is not None, dev.max(), scale)
                    worst = max(worst, (dev[scale > 0] / scale[scale > 0]).max() if (scale > 0).any() else 0.0)
                    if kept is not None and not kept.any():
                        assert not got.any()                     # nobody kept: exact zeros
                    assert np.array_equal(call(g, kept)[0], got)       # two calls, the same bits
                    if RA == 0 and RB == 0:
                        # through the new entry points with no squared column: the rows of sc_hk_opcorr on the same operands
                        lin = call(g, kept, linear=True)[0]
                        dev_lin = abs(got - lin).max(axis=1)
                        assert (dev_lin <= 1e-13 * abs(lin).max(axis=1)).all(), (n, M, dev_lin.max())
                        worst_lin = max(worst_lin, (dev_lin[scale > 0] / abs(lin).max(axis=1)[scale > 0]).max() if (scale > 0).any() else 0.0)
                # a non-finite cq, g or state of a discarded trajectory never reaches the sums: each alone, and all together
                if n > 1:
                    kept = np.arange(n) > 0
                    clean = call(g, kept)[0]
                    qp, cq, gd = call.qp.copy(), call.cq.copy(), g.copy()
                    qp[0], cq[0], gd[0] = np.nan, np.inf, np.nan
                    for dirty in (dict(qp=qp), dict(cq=cq)):
                        assert np.array_equal(call(g, kept, **dirty)[0], clean), (n, M, RA, sorted(dirty))
                    assert np.array_equal(call(gd, kept)[0], clean), (n, M, RA, "g")
                    assert np.array_equal(call(gd, kept, qp=qp, cq=cq)[0], clean), (n, M, RA, "all")
    # with a cursor the row goes to out[*cursor]
    got = call(g, None, cursor=2, rows=3)
    assert np.isnan(got[:2]).all() and np.array_equal(got[2], call(g)[0])
    print(f"D={D}: largest deviation of a row {worst:.2e} of its largest entry; of g {worst_g:.2e}; R = 0 against sc_hk_opcorr {worst_lin:.2e}")


def test_c_abi_refusals():
    from semiclassical_amd import _lib
    lib, ptr = _lib.lib, _lib.ptr
    buf = torch.zeros(4096, device="cuda")
    state = _lib.sc_state(n=5, dim=3, mono_layout=0, qp=buf.data_ptr(), act=None, mono=None, c2=None, sgn=None, work=None, flags=None)
    b = ptr(buf)
    args = lambda **kw: [kw.get("st", state), kw.get("cq", b), b, b, b, kw.get("lam", b), b, kw.get("M", 1), kw.get("R", 0), None, b,
                         kw.get("out", b), None, None]
    assert lib.sc_hk_opquad(*args()) == 0
    for null in ("cq", "lam", "out"):
        assert lib.sc_hk_opquad(*args(**{null: None})) == -1
    assert lib.sc_hk_opquad(*args(M=0)) == -1 and lib.sc_hk_opquad(*args(R=-1)) == -1
    assert lib.sc_hk_opquad(*args(R=513)) == -2 and b"512" in lib.sc_last_error()
    assert lib.sc_hk_opquad(*args(M=65536)) == -2 and b"65535" in lib.sc_last_error()
    assert lib.sc_hk_opquad(*args(M=65535, R=256)) == -2 and b"16777216" in lib.sc_last_error()       # 65535 x 257 >= 2^24
    big = _lib.sc_state.from_buffer_copy(state)
    big.dim = 513
    assert lib.sc_hk_opquad(*args(st=big)) == -2 and b"512" in lib.sc_last_error()
    many = _lib.sc_state.from_buffer_copy(state)
    many.n = 64 * 65535 + 1
    assert lib.sc_hk_opquad(*args(st=many)) == -2 and str(64 * 65535).encode() in lib.sc_last_error()
    init = lambda **kw: [kw.get("zi", b), kw.get("n", 5), kw.get("D", 3), b, b, b, kw.get("lam", b), kw.get("M", 1), kw.get("R", 0),
                         kw.get("g", b), None]
    assert lib.sc_hk_opquad_initial(*init()) == 0
    assert all(lib.sc_hk_opquad_initial(*init(**{null: None})) == -1 for null in ("zi", "lam", "g"))
    assert lib.sc_hk_opquad_initial(*init(M=0)) == -1 and lib.sc_hk_opquad_initial(*init(R=-1)) == -1
    assert lib.sc_hk_opquad_initial(*init(R=513)) == -2 and lib.sc_hk_opquad_initial(*init(D=513)) == -2
    assert lib.sc_hk_opquad_initial(*init(M=65535, R=256)) == -2 and lib.sc_hk_opquad_initial(*init(n=64 * 65535 + 1)) == -2
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------- 12. run(operators=...)

@pytest.mark.parametrize("name,nt,attrs,entry,bits", ROUTES, ids=[f"{r[0]}-{r[3]}" for r in ROUTES])
def test_run_with_quadratic_operators(name, nt, attrs, entry, bits, monkeypatch):
    g, pot, prop = _prepared(name, **attrs)
    dt, E0 = float(g["dt"]), float(g["E0"])
    D = prop.dim
    bra, ket = _operators(prop, np.random.default_rng(nt))
    targets = (np.vstack((g["q0"], g["zi"][:D, 0])), np.vstack((g["p0"], g["zi"][D:, 0])))
    blocks = torch.zeros((nt, 4, 4), device=prop.device)
    spy = _Spy(monkeypatch)
    C, k, sC, sk, T, sT, X, sX = prop.run(pot, dt, nt, E0, standard_errors=True, blocks=blocks, targets=targets, operators=(bra, ket))
    monkeypatch.undo()
    assert spy.seen.get(entry, 0) > 0 and spy.seen.get("sc_hk_opquad", 0) == nt and spy.seen.get("sc_hk_cross", 0) == nt, spy.seen
    assert "sc_hk_opcorr" not in spy.seen and "sc_hk_run" not in spy.seen and "sc_hk_run_m" not in spy.seen
    assert X.shape == sX.shape == (nt, 4) and X.dtype == np.complex128
    # with K removed: the same C, k, errors, blocks, cross rows and final state, bit for bit
    _, pot2, twin = _prepared(name, **attrs)
    blocks2 = torch.zeros((nt, 4, 4), device=prop.device)
    C2, k2, sC2, sk2, T2, sT2, X2, sX2 = twin.run(pot2, dt, nt, E0, standard_errors=True, blocks=blocks2, targets=targets,
                                                  operators=(bra[:2], ket[:2]))
    for a, b in ((C, C2), (k, k2), (sC, sC2), (sk, sk2), (T, T2), (sT, sT2)):
        assert np.array_equal(a, b)
    assert torch.equal(blocks, blocks2) and torch.equal(prop.y, twin.y) and torch.equal(prop._c2, twin._c2) and prop.t == twin.t
    assert not np.array_equal(X, X2)                               # the K matter
    # all-zero K: sc_hk_opcorr, not sc_hk_opquad, and the bits of (c, m)
    _, pot5, zero = _prepared(name, **attrs)
    spy = _Spy(monkeypatch, names=("sc_hk_opcorr", "sc_hk_opquad", "sc_hk_opcorr_initial", "sc_hk_opquad_initial"))
    out5 = zero.run(pot5, dt, nt, E0, standard_errors=True, targets=targets,
                    operators=(bra[:2] + (np.zeros_like(bra[2]),), ket[:2] + (None,)))
    monkeypatch.undo()
    assert spy.seen == {"sc_hk_opcorr": nt, "sc_hk_opcorr_initial": 1}, spy.seen
    assert np.array_equal(out5[6], X2) and np.array_equal(out5[7], sX2) and np.array_equal(out5[0], C2)
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


# ------------------------------------------------------------------------------------------- 13. under a discard mask

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
    bra, ket = _operators(prop, np.random.default_rng(18))
    X = prop.operator_correlation(bra, ket, energy0_es=E0)
    s = _read_back(prop)
    rows = _restated(bra, ket, s, kept)                          # cq carries the unchanged N
    want = (rows[:, 0] + 1j * rows[:, 1]) * np.exp(1j * prop.t * E0)
    everyone = _restated(bra, ket, s)
    assert abs(everyone[:, 0] - rows[:, 0]).max() > 1e-3 * abs(rows[:, 0]).max()      # the mask matters
    scale = abs(want).max()
    print(f"masked: deviation {abs(X - want).max() / scale:.2e} of max |X|")
    assert abs(X - want).max() <= TOL * scale
    t0 = prop.t
    out = prop.run(pot, dt, 2, E0, operators=(bra, ket))
    assert len(out) == 3 and prop.t > t0 and abs(out[2][0] - want).max() <= TOL * scale      # row 0: the state the call above saw


# ------------------------------------------------------------------------------------------- 14. standard errors mean something

def test_standard_errors_cover_the_closed_form():
    """t = 0 on the fixture's own initial conditions: every X_a(0) within 5 sigma_a of <phi_0|A_a B_a|phi_0> for the three pairs
    checked on the CPU first (test_opquad_host.py::test_five_sigma_at_t0_on_the_cpu), and sigma equal to the restatement's"""
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
    big = want.imag > 1e-6 * abs(exact)                          # (pair 1: Im x_i = 0 up to rounding, sigma_Im is rounding noise)
    assert big[[0, 2]].all() and (abs(sigma.imag - want.imag)[big] <= 1e-9 * want.imag[big]).all()


# ------------------------------------------------------------------------------------------- 15. driver

def test_driver_key_with_k(tmp_path):
    import os
    from semiclassical_amd import driver, propagators, units
    out, ofile = tmp_path / "correlations.npz", tmp_path / "operators.npz"
    task = {"task": "dynamics", "propagator": "HK", "batch_size": 64, "num_trajectories": 128, "num_steps": 6, "time_step_fs": 0.005,
            "manual_seed": 0, "standard_errors": True, "operator_correlation": str(ofile),
            "potential": {"type": "harmonic", "ground": os.path.join(FCHK, "methylium_s0.fchk"),
                          "excited": os.path.join(FCHK, "methylium_s1.fchk"), "coupling": os.path.join(FCHK, "methylium_s1.fchk")},
            "results": {"correlations": str(out)}}
    setup = driver.build_problem(task)
    D = setup.q0.shape[0]
    G0 = setup.Gamma_0.numpy()
    e, V = np.linalg.eigh(G0)
    bra_c, bra_m = np.array([1.0, 0.0, 0.5]), np.vstack((np.zeros(D), V[:, -1], 2.0 * V[:, -2]))
    rng = np.random.default_rng(15)
    bra_k = np.array([np.zeros((D, D)), random_symmetric(rng, D, 2, G0, G0), random_symmetric(rng, D, 6, G0, G0)])
    np.savez(ofile, bra_c=bra_c, bra_m=bra_m, bra_k=bra_k)
    driver.run_semiclassical_dynamics(task, device="cuda")
    d = dict(np.load(out))
    assert int(d["trajectories"]) == 128
    assert np.array_equal(d["operator_bra_k"], bra_k) and np.array_equal(d["operator_ket_k"], bra_k)
    assert np.array_equal(d["operator_bra_c"], bra_c) and np.array_equal(d["operator_ket_m"], bra_m)
    X = d["operator_correlation"]
    assert X.shape == (6, 3) and d["operator_correlation_error"].shape == (6, 3)
    assert abs(X[:, 0] - d["autocorrelation"]).max() <= 1e-9       # pair 0 is (1, 1)
    # the stored rows are those of a direct run() on the same two batches (the driver's own seeds: device sampling, subsequence b)
    dt, pooled = task["time_step_fs"] / units.autime_to_fs, 0.0
    for batch in range(2):
        prop = propagators.HermanKlukPropagator(setup.Gamma_0, setup.Gamma_0, device="cuda")
        prop.initial_conditions(setup.q0, setup.p0, setup.Gamma_0, ntraj=64, ntraj_total=64, seed=0, subsequence=batch, first_index=0)
        pooled = pooled + prop.run(setup.potential, dt, 6, setup.zero_point_energy, operators=(bra_c, bra_m, bra_k))[2] / 2.0
    dev = abs(X - pooled).max() / abs(pooled).max()
    print(f"driver: stored rows against a direct run() {dev:.2e} of max |X|")
    assert dev <= 1e-9
    # another K, adding to the file: refused before anything runs, the file as it was
    again = dict(task, results={"correlations": str(out), "overwrite": False})
    again.pop("manual_seed")
    for other in (dict(bra_k=2.0 * bra_k), dict()):
        np.savez(ofile, bra_c=bra_c, bra_m=bra_m, **other)
        with pytest.raises(driver.ConfigurationError, match="operators"):
            driver.run_semiclassical_dynamics(again, device="cuda")
    after = dict(np.load(out))
    assert set(after) == set(d) and all(np.array_equal(after[k], d[k]) for k in d)
    # the same task without the K arrays: the keys and values it writes today (an all-zero K among them: the linear path)
    plain_out, zero_out = tmp_path / "plain.npz", tmp_path / "zero.npz"
    np.savez(ofile, bra_c=bra_c, bra_m=bra_m)
    driver.run_semiclassical_dynamics(dict(task, results={"correlations": str(plain_out)}), device="cuda")
    p = dict(np.load(plain_out))
    assert set(d) - set(p) == {"operator_bra_k", "operator_ket_k"} and set(p) - set(d) == set()
    assert set(p) == {"propagator", "times", "autocorrelation", "ic_correlation", "adiabatic_gap", "zero_point_energy", "trajectories",
                      *driver.CorrelationStore.ERROR_KEYS, *driver.CorrelationStore.OPERATOR_KEYS, *driver.CorrelationStore.OPERATOR_ERROR_KEYS}
    for key in ("autocorrelation", "ic_correlation", "autocorrelation_error", "operator_bra_m", "operator_ket_c"):
        assert np.array_equal(p[key], d[key]), key
    # K_0 = 0: the same numbers from the other kernel (another order of the sums)
    assert abs(p["operator_correlation"][:, 0] - d["operator_correlation"][:, 0]).max() <= 1e-12
    np.savez(ofile, bra_c=bra_c, bra_m=bra_m, bra_k=np.zeros_like(bra_k))
    driver.run_semiclassical_dynamics(dict(task, results={"correlations": str(zero_out)}), device="cuda")
    z = dict(np.load(zero_out))
    assert not z.pop("operator_bra_k").any() and not z.pop("operator_ket_k").any()
    assert set(z) == set(p) and all(np.array_equal(z[key], p[key]) for key in p)
    # the same K pools
    np.savez(ofile, bra_c=bra_c, bra_m=bra_m, bra_k=bra_k)
    driver.run_semiclassical_dynamics(again, device="cuda")
    both = np.load(out)
    assert int(both["trajectories"]) == 256 and np.array_equal(both["operator_bra_k"], bra_k)
