"""HermanKlukPropagator.time_average / run(time_average=...) (sc_hk_ta_*) against the numpy restatement
of the definitions (tests/timeavg_cases.py): the tile edges through the C-ABI, every route of run(), cut loops, Parseval, the
harmonic oscillator's closed form, the discard mask, the refusals and the driver key."""
import os

import numpy as np
import pytest
import torch

from tests import timeavg_cases as ta
from tests.lib_spy import LibSpy as _Spy
from tests.test_cross_gpu import _prepared, _synthetic, _widths
from tests.test_cross_host import overlap_constants, psd_sqrt

pytestmark = pytest.mark.gpu
torch.set_default_dtype(torch.float64)

TOL = 1e-9          # x max |I|: the standing bound of sections 4.12 to 4.16 for a sum over trajectories against the host


def _read(prop):
    """(q, p, c, S) of the engine's current state as numpy, through the public accessors; c = signs x sqrt(previous)"""
    q, p = prop.current_positions_and_momenta()
    c = prop.semiclassical_prefactor().cpu().numpy()
    tracker = prop.sign_trackers["prefactorC"]
    assert np.array_equal(c, (tracker["signs"] * torch.sqrt(tracker["previous"])).cpu().numpy())
    return q.cpu().numpy().copy(), p.cpu().numpy().copy(), c, prop.classical_action().cpu().numpy().copy()


def _terms_of(prop, Q, P, kept=None):
    q, p, c, act = _read(prop)
    return ta.restated_terms(q, p, c, act, prop._Gt.numpy(), prop._G0h.numpy(), Q, P, kept)


def _loop_terms(name, attrs, ns, Q=None, P=None):
    """g (ns, n, K) of the step-by-step loop: row s = the state before step s, read back at every step"""
    g, pot, loop = _prepared(name, **attrs)
    Q, P = (g["q0"][None, :], g["p0"][None, :]) if Q is None else (Q, P)
    rows = []
    for _ in range(ns):
        rows.append(_terms_of(loop, Q, P))
        loop.step(pot, float(g["dt"]))
    return np.stack(rows)


def _energies(g, NE=7):
    """NE energies around the zero-point energy"""
    E0 = float(g["E0"])
    return E0 * (1.0 + 0.5 * np.linspace(-1.0, 1.0, NE))


def _mc_norm(prop):
    return prop._ntraj_norm * (2.0 * np.pi) ** prop.dim


# ------------------------------------------------------------------------------------------- 1. tile edges through the C-ABI

SIZES = (1, 63, 64, 65, 130)
COUNTS_K = (1, 2, 5)
COUNTS_NE = (1, 15, 64, 65)


class _TimeAverage(object):
    """sc_hk_ta_terms / _accumulate / _finish on synthetic states, one state per column: device buffers built once per n"""

    def __init__(self, states, Gt, G0, diag, mc_norm):
        from semiclassical_amd import _lib
        self.lib, self.mc_norm, self.diag = _lib, mc_norm, diag
        D, n = states[0]["q"].shape
        self.D, self.n = D, n
        dev = lambda a: torch.from_numpy(np.array(a, dtype=np.float64, order="C")).to("cuda")
        cx = lambda a: torch.view_as_real(torch.from_numpy(np.array(a, dtype=complex, order="C"))).contiguous().to("cuda")
        A, B, C, self.fac = overlap_constants(Gt, G0)
        self.La, self.Lb, self.C = psd_sqrt(A), psd_sqrt(B), C
        self.consts = [dev(np.diag(self.La)), dev(np.diag(self.Lb)), dev(np.diag(C))] if diag else [dev(self.La), dev(self.Lb), dev(C.T)]
        self.keep, self.states = [], []
        for st in states:
            b = dict(qp=dev(np.vstack((st["q"], st["p"])).T), act=dev(st["act"]), c2=cx(st["c2"]), sgn=dev(st["sgn"]))
            self.keep.append(b)
            self.states.append(_lib.sc_state(n=n, dim=D, mono_layout=0, qp=b["qp"].data_ptr(), act=b["act"].data_ptr(), mono=None,
                                             c2=b["c2"].data_ptr(), sgn=b["sgn"].data_ptr(), work=None, flags=None))
        self.probi = dev(states[0]["probi"])
        self.operands = None if diag else torch.full((n, 4 * D), np.nan, device="cuda")
        self.TB = int(_lib.lib.sc_hk_ta_block())

    def __call__(self, Q, P, columns, energy_sets, t_a, dt, kept=None):
        """the raw sums (K, NE, 2) of the first `columns` states, for every set of energies from ONE pass over the terms"""
        lib, ptr, check = self.lib.lib, self.lib.ptr, self.lib.check
        K, n, TB = Q.shape[0], self.n, self.TB
        stream = torch.cuda.current_stream().cuda_stream
        refs = torch.from_numpy(np.ascontiguousarray(np.hstack((Q @ self.La.T, P @ self.Lb.T, Q, P @ self.C.T, P)))).to("cuda")
        mask = None if kept is None else torch.from_numpy(np.asarray(kept, dtype=np.uint8)).to("cuda")
        G = torch.full((TB, n * K, 2), np.nan, device="cuda")
        sets = [(torch.from_numpy(np.ascontiguousarray(E)).to("cuda"), torch.zeros((n * K, len(E), 2), device="cuda"),
                 torch.full((TB, len(E), 2), np.nan, device="cuda")) for E in energy_sets]
        c, pending = self.consts, 0
        for s in range(columns):
            check(lib.sc_hk_ta_terms(self.states[s], ptr(c[0]), ptr(c[1]), ptr(c[2]), int(self.diag), float(self.fac), ptr(refs), K,
                                     ptr(mask), ptr(self.operands), ptr(G), pending, stream))
            pending += 1
            if pending == TB or s == columns - 1:
                for E, A, W in sets:
                    check(lib.sc_hk_ta_accumulate(ptr(G), n, K, pending, ptr(E), E.shape[0], t_a, dt, s + 1 - pending, ptr(W), ptr(A),
                                                  stream))
                pending = 0
        outs = []
        for E, A, W in sets:
            part = torch.full((int(lib.sc_hk_ta_finish_rows(n)) * K * E.shape[0] * 2,), np.nan, device="cuda")
            out = torch.full((K, E.shape[0], 2), np.nan, device="cuda")
            before = A.clone()
            check(lib.sc_hk_ta_finish(ptr(A), n, K, E.shape[0], ptr(self.probi), self.mc_norm, ptr(mask), ptr(part), ptr(out), stream))
            torch.cuda.synchronize()
            assert torch.equal(A, before)                        # finishing does not change the accumulator
            outs.append(out.cpu().numpy())
        return outs


@pytest.mark.parametrize("diag,D", [(True, 1), (True, 16), (True, 17), (True, 33), (False, 2), (False, 12)])
def test_tile_edges_through_the_c_abi(diag, D):
    from semiclassical_amd import _lib
    TB = int(_lib.lib.sc_hk_ta_block())
    COLUMNS = (1, TB - 1, TB, TB + 1, 2 * TB + 3)
    rng = np.random.default_rng(1000 * D + diag)
    Gt, G0 = _widths(rng, D, diag)
    t_a, dt = 0.37, 0.05
    energy_sets = [rng.uniform(-2.0, 3.0, NE) for NE in COUNTS_NE]
    worst = 0.0
    for n in SIZES:
        states = [_synthetic(rng, n, D) for _ in range(COLUMNS[-1])]
        for st in states[1:3]:
            st["c2"][0] = 0.0                                    # c_i = 0: u_i = 0
        probi, mc_norm = states[0]["probi"], float(n) * 1.7
        call = _TimeAverage(states, Gt, G0, diag, mc_norm)
        dirty = [dict(st, q=st["q"].copy(), c2=st["c2"].copy()) for st in states]
        for st in dirty:
            st["q"][:, 0], st["c2"][0] = np.nan, np.inf
        call_dirty = _TimeAverage(dirty, Gt, G0, diag, mc_norm)
        # no mask; the first band of 64 discarded; a single trajectory kept; a non-finite state in a discarded trajectory
        masks = [(call, None), (call, np.arange(n) >= 64), (call, np.arange(n) == n // 2), (call_dirty, np.arange(n) > 0)]
        for K in COUNTS_K:
            s = 1.0 / np.sqrt(D)
            Q, P = rng.normal(0.0, 0.6 * s, (K, D)), rng.normal(0.0, 0.9 * s, (K, D))
            everyone = np.stack([ta.restated_terms(st["q"], st["p"], st["sgn"] * np.sqrt(st["c2"]), st["act"], Gt, G0, Q, P)
                                 for st in states])
            for engine, kept in masks:
                g = everyone if kept is None else np.where(kept[None, :, None], everyone, 0.0)       # exact zeros, as restated_terms(kept)
                for columns in COLUMNS:
                    got = engine(Q, P, columns, energy_sets, t_a, dt, kept)
                    again = engine(Q, P, columns, energy_sets, t_a, dt, kept)
                    for E, out, twice in zip(energy_sets, got, again):
                        A = ta.restated_accumulator(g[:columns], E, t_a, dt)
                        want = np.stack(ta.restated_sums(A, 1.0, mc_norm, probi, kept), axis=2)      # (T = 1: the raw sums)
                        assert out.shape == want.shape == (K, len(E), 2) and np.isfinite(out).all()
                        for col in range(2):
                            scale = abs(want[..., col]).max()
                            dev = abs(out[..., col] - want[..., col]).max()
                            assert dev <= TOL * scale, (n, K, len(E), columns, kept is not None, col, dev, scale)
                            worst = max(worst, dev / scale if scale > 0 else 0.0)
                        if kept is not None and not kept.any():
                            assert not out.any()                 # nobody kept: exact zeros
                        assert np.array_equal(out, twice)        # two calls, the same bits
    print(f"diag={diag} D={D}: largest deviation of a column {worst:.2e} of its largest entry")


def test_c_abi_refusals():
    from semiclassical_amd import _lib
    rng = np.random.default_rng(0)
    Gt, G0 = _widths(rng, 3, True)
    call = _TimeAverage([_synthetic(rng, 5, 3)], Gt, G0, True, 5.0)
    lib, ptr = _lib.lib, _lib.ptr
    TB = call.TB
    buf = torch.zeros(4096, device="cuda")
    c = call.consts
    terms = lambda **kw: lib.sc_hk_ta_terms(kw.get("st", call.states[0]), ptr(c[0]), ptr(c[1]), ptr(c[2]), kw.get("diag", 1), 1.0, ptr(buf),
                                            kw.get("K", 1), None, None, kw.get("G", ptr(buf)), kw.get("column", 0), None)
    assert terms() == 0
    assert terms(K=0) == -1 and terms(G=None) == -1 and terms(column=-1) == -1 and terms(column=TB) == -1
    assert terms(diag=0) == -1                                   # dense widths without the operand scratch
    assert terms(K=65) == -2 and b"64" in lib.sc_last_error()
    big = _lib.sc_state.from_buffer_copy(call.states[0])
    big.dim = 513
    assert terms(st=big) == -2 and b"512" in lib.sc_last_error()
    many = _lib.sc_state.from_buffer_copy(call.states[0])
    many.n = 64 * 65535 + 1
    assert terms(st=many) == -2 and str(64 * 65535).encode() in lib.sc_last_error()
    acc = lambda **kw: lib.sc_hk_ta_accumulate(ptr(buf), 5, kw.get("K", 1), kw.get("count", 1), ptr(buf), kw.get("NE", 1), 0.0, 0.1, 0,
                                               ptr(buf), kw.get("A", ptr(buf)), None)
    assert acc() == 0
    assert acc(count=0) == -1 and acc(count=TB + 1) == -1 and acc(K=0) == -1 and acc(NE=0) == -1 and acc(A=None) == -1
    assert acc(NE=65536) == -2 and b"65535" in lib.sc_last_error()
    fin = lambda **kw: lib.sc_hk_ta_finish(ptr(buf), 5, kw.get("K", 1), kw.get("NE", 1), ptr(call.probi), 1.0, None, ptr(buf),
                                           kw.get("out", ptr(buf)), None)
    assert fin() == 0
    assert fin(K=0) == -1 and fin(NE=0) == -1 and fin(out=None) == -1 and fin(NE=65536) == -2 and fin(K=65) == -2
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------- 2. run(time_average=...)

ROUTES = [
    # case, ns, attributes, the entry point that has to run, bit-identical outputs promised (else: a whole-loop shape, 1e-12)
    ("hk_1d", 5, {}, "sc_hk_step", False),
    ("hk_as5_chi002", 5, {}, "sc_hk_step", False),
    ("hk_as33", 5, {"visit_min_bytes": 0, "visit_steps": 2}, "sc_hk_step_multi", True),
    ("hk_as60_n96", 7, {"visit_min_bytes": 0, "visit_steps": 3}, "sc_hk_step_visit", True),
    ("hk_methylium", 3, {}, None, False),                                # a constant dense Hessian with D <= 16: a whole-loop shape too
    ("hk_coumarin_harmonic", 3, {}, "sc_hk_step_modal", True),
]


@pytest.mark.parametrize("name,ns,attrs,entry,bits", ROUTES, ids=[r[0] for r in ROUTES])
def test_run_with_an_accumulator(name, ns, attrs, entry, bits, monkeypatch):
    """measured on the MI355X (deviation / max |I|): see DESIGN.md section 4.17"""
    g, pot, prop = _prepared(name, **attrs)
    dt, E0 = float(g["dt"]), float(g["E0"])
    rng = np.random.default_rng(ns)
    D, n = prop.dim, prop.ntraj
    zi = g["zi"]
    # (q0, p0) and one more reference state within the ensemble (shrunk by sqrt(D), as the targets of test_cross_gpu.py)
    Q = np.vstack((g["q0"], zi[:D].mean(1) + zi[:D].std(1) * rng.uniform(-1.0, 1.0, D) / np.sqrt(D)))
    P = np.vstack((g["p0"], zi[D:].mean(1) + zi[D:].std(1) * rng.uniform(-1.0, 1.0, D) / np.sqrt(D)))
    energies = _energies(g)
    acc = prop.time_average(energies, dt, references=(Q, P))
    spy = _Spy(monkeypatch)
    C, k, sC, sk = prop.run(pot, dt, ns, E0, standard_errors=True, time_average=acc)
    monkeypatch.undo()
    assert spy.seen.get("sc_hk_ta_terms", 0) == ns and "sc_hk_run" not in spy.seen and "sc_hk_run_m" not in spy.seen, spy.seen
    assert entry is None or spy.seen.get(entry, 0) > 0, spy.seen
    assert acc.steps == ns and acc.pending == ns % acc.TB and acc.window == ns * dt
    I, sigma = acc.spectrum(standard_errors=True)
    assert I.shape == sigma.shape == (2, 7) and acc.pending == 0
    want, want_sigma = ta.restated_spectrum(_loop_terms(name, attrs, ns, Q, P), energies, 0.0, dt, _mc_norm(prop), g["probi"], n)
    scale = abs(want).max()
    print(f"{name}: I {np.array2string(want[0], precision=3)}, deviation {abs(I - want).max() / scale:.2e} of the largest")
    assert scale > 0 and abs(I - want).max() <= TOL * scale
    assert np.allclose(sigma, want_sigma, rtol=1e-6, atol=TOL * scale)
    # the default reference state is (q0, p0)
    _, pot1, one = _prepared(name, **attrs)
    acc1 = one.time_average(energies, dt)
    one.run(pot1, dt, ns, E0, time_average=acc1)
    # (not bit for bit: with dense widths the host forms the operand rows of K reference states by one matrix product, whose
    # rounding depends on K)
    assert abs(acc1.spectrum()[0] - I[0]).max() <= 1e-12 * scale
    # without the accumulator: the same C, k, errors and final state
    _, pot2, twin = _prepared(name, **attrs)
    C2, k2, sC2, sk2 = twin.run(pot2, dt, ns, E0, standard_errors=True)
    for a, b in ((C, C2), (k, k2), (sC, sC2), (sk, sk2)):
        if bits:
            assert np.array_equal(a, b)
        else:
            assert abs(a - b).max() <= 1e-12 * max(abs(b).max(), 1e-300)
    if bits:
        assert torch.equal(prop.y, twin.y) and torch.equal(prop._c2, twin._c2) and torch.equal(prop._sgn, twin._sgn)
    else:
        assert float((prop.y - twin.y).abs().max()) <= 1e-12 * float(twin.y.abs().max())
    assert prop.t == twin.t


@pytest.mark.parametrize("name,ns", [("hk_1d", 5), ("hk_as5_chi002", 5), ("hk_methylium", 3)])
def test_whole_loop_shape_bits_against_the_stepwise_loop(name, ns):
    """on a whole-loop shape C, k and the state with the accumulator are the step-at-a-time loop's, bit for bit"""
    g, pot, prop = _prepared(name)
    dt, E0 = float(g["dt"]), float(g["E0"])
    out = prop.run(pot, dt, ns, E0, standard_errors=True, time_average=prop.time_average(_energies(g), dt))
    _, pot2, twin = _prepared(name)
    twin._whole_loop_ok = False
    for a, b in zip(out, twin.run(pot2, dt, ns, E0, standard_errors=True)):
        assert np.array_equal(a, b)
    assert torch.equal(prop.y, twin.y)


PIECES = [
    ("hk_as33", {"pair_steps": False}, "sc_hk_step", 5, 12),
    ("hk_as33", {"visit_min_bytes": 0, "visit_steps": 2}, "sc_hk_step_multi", 5, 12),
    ("hk_as33", {"visit_min_bytes": 0, "visit_steps": 3}, "sc_hk_step_visit", 30, 67),       # 2 TB + 3 steps: blocks fill mid-visit
]


@pytest.mark.parametrize("name,attrs,entry,first,ns", PIECES, ids=[p[2] for p in PIECES])
def test_pieces_give_the_bits_of_the_uncut_loop(name, attrs, entry, first, ns, monkeypatch):
    g, pot, prop = _prepared(name, **attrs)
    dt, E0 = float(g["dt"]), float(g["E0"])
    energies = _energies(g)
    whole = prop.time_average(energies, dt)
    assert ns in (12, 2 * whole.TB + 3)
    spy = _Spy(monkeypatch)
    prop.run(pot, dt, ns, E0, time_average=whole)
    monkeypatch.undo()
    assert spy.seen.get(entry, 0) > 0 and spy.seen.get("sc_hk_ta_accumulate", 0) == ns // whole.TB, spy.seen
    want = whole.raw_sums()
    assert want.shape == (1, 7, 2) and (want > 0).all()
    # two pieces on one accumulator: the pending columns stay in it between the calls
    _, pot2, cut = _prepared(name, **attrs)
    acc = cut.time_average(energies, dt)
    cut.run(pot2, dt, first, E0, time_average=acc)
    assert acc.pending == first % acc.TB
    cut.run(pot2, dt, ns - first, E0, time_average=acc)
    assert np.array_equal(acc.raw_sums(), want) and torch.equal(cut.y, prop.y)
    # a flush in the middle (spectrum()) moves the block boundaries and changes no bit either
    _, pot3, mid = _prepared(name, **attrs)
    acc = mid.time_average(energies, dt)
    mid.run(pot3, dt, first, E0, time_average=acc)
    acc.spectrum()
    mid.run(pot3, dt, ns - first, E0, time_average=acc)
    assert np.array_equal(acc.raw_sums(), want)
    # step by step
    _, pot4, loop = _prepared(name, **attrs)
    acc = loop.time_average(energies, dt)
    for _ in range(ns):
        acc.add()
        loop.step(pot4, dt)
    assert acc.steps == ns and np.array_equal(acc.raw_sums(), want)


def test_parseval_on_the_engine():
    """ns = NE = 12, E_e = 2 pi hbar e / (ns dt): sum_e I(E_e) 2 pi hbar / (ns dt) = 1/ns sum_s sum_i |g_i(t_s)|^2 / (mc_norm P_i)"""
    name, ns = "hk_as5_chi002", 12
    g, pot, prop = _prepared(name)
    dt = float(g["dt"])
    energies = 2.0 * np.pi * np.arange(ns) / (ns * dt)
    acc = prop.time_average(energies, dt)
    prop.run(pot, dt, ns, float(g["E0"]), time_average=acc)
    left = acc.spectrum()[0].sum() * 2.0 * np.pi / (ns * dt)
    terms = _loop_terms(name, {}, ns)
    right = (abs(terms[:, :, 0]) ** 2 / (_mc_norm(prop) * g["probi"][None, :])).sum() / ns
    print(f"Parseval on the engine: {left:.12e} against {right:.12e}, {abs(left - right) / right:.2e}")
    assert abs(left - right) <= 1e-10 * right


# ------------------------------------------------------------------------------------------- 3. physics

def test_harmonic_oscillator_spectrum():
    """omega = 1, chi = 0, D = 1, Gamma_i = Gamma_t = Gamma_0 = 1, q0 = 1.6, dt = 0.05, ns = 2000, N = 2048: I at the six energies
    within 5 sigma of the closed form, sigma / I <= 0.3 at the three peaks; 16 periods of the square-root branch enter u_i.
    Measured on the MI355X: see DESIGN.md section 4.17."""
    from semiclassical_amd import potentials as P, propagators as PR
    o = ta.OSC
    one = torch.ones(1)
    pot = P.MorsePotential(o["omega"] * one, 0.0 * one, 0.0 * one)
    G = torch.eye(1)
    prop = PR.HermanKlukPropagator(G, G, device="cuda")
    prop.initial_conditions(o["q0"] * one, 0.0 * one, G, ntraj=o["N"], seed=o["N"])
    acc = prop.time_average(ta.OSC_ENERGIES, o["dt"])
    prop.run(pot, o["dt"], o["ns"], time_average=acc)
    I, sigma = acc.spectrum(standard_errors=True)
    exact = ta.oscillator_closed_form(ta.OSC_ENERGIES)
    for e, E in enumerate(ta.OSC_ENERGIES):
        print(f"E = {E}: I {I[0, e]:.5f}  closed form {exact[e]:.5f}  sigma {sigma[0, e]:.2e}  |dev| / sigma "
              f"{abs(I[0, e] - exact[e]) / sigma[0, e]:.2f}  sigma / I {sigma[0, e] / I[0, e]:.3f}")
    assert (abs(I[0] - exact) <= 5.0 * sigma[0]).all()
    peaks = list(ta.OSC_PEAKS)
    assert (sigma[0, peaks] / I[0, peaks] <= 0.3).all()


# ------------------------------------------------------------------------------------------- 4. under a discard mask

def test_discard_mask():
    """discarded after step 2 of 5: I is the restatement with those trajectories' y set to zero, N unchanged"""
    name, ns, cut = "hk_as5_chi002", 5, 2
    g, pot, prop = _prepared(name)
    dt, E0 = float(g["dt"]), float(g["E0"])
    energies = _energies(g)
    acc = prop.time_average(energies, dt)
    prop.run(pot, dt, cut, E0, time_average=acc)
    eps = prop.symplectic_deviation().cpu().numpy()
    prop.discard_nonsymplectic(float(np.median(eps)))
    kept = prop.kept.cpu().numpy().astype(bool)
    print(f"kept {int(kept.sum())} of {prop.ntraj}")
    assert 0 < kept.sum() < prop.ntraj
    prop.run(pot, dt, ns - cut, E0, time_average=acc)
    I, sigma = acc.spectrum(standard_errors=True)
    terms = _loop_terms(name, {}, ns)
    want, want_sigma = ta.restated_spectrum(terms, energies, 0.0, dt, _mc_norm(prop), g["probi"], prop.ntraj, kept)
    everyone, _ = ta.restated_spectrum(terms, energies, 0.0, dt, _mc_norm(prop), g["probi"], prop.ntraj)
    scale = abs(want).max()
    assert abs(everyone - want).max() > 1e-3 * scale             # the mask matters
    print(f"masked: deviation {abs(I - want).max() / scale:.2e} of max |I|")
    assert abs(I - want).max() <= TOL * scale
    assert np.allclose(sigma, want_sigma, rtol=1e-6, atol=TOL * scale)
    # their terms are exact zeros from the discard on
    assert not acc._G[cut:ns][:, torch.from_numpy(~kept).to(acc._G.device)].any()


# ------------------------------------------------------------------------------------------- 5. refusals

def test_refusals():
    g, pot, prop = _prepared("hk_as5_chi002")
    dt, E0 = float(g["dt"]), float(g["E0"])
    D, n = prop.dim, prop.ntraj
    energies = _energies(g)
    before = [t.clone() for t in (prop._qp, prop._act, prop._mono, prop._c2, prop._sgn)]
    acc = prop.time_average(energies, dt)
    with pytest.raises(ValueError, match="dt"):
        prop.run(pot, 2.0 * dt, 2, E0, time_average=acc)
    with pytest.raises(ValueError, match="use_graph"):
        prop.run(pot, dt, 4, E0, time_average=acc, use_graph=True)
    with pytest.raises(ValueError, match="64"):
        prop.time_average(energies, dt, references=(np.zeros((65, D)), np.zeros((65, D))))
    with pytest.raises(ValueError, match=str(16 * n * 7)):
        prop.time_average(energies, dt, max_bytes=16 * n * 7 - 1)
    prop.time_average(energies, dt, max_bytes=16 * n * 7)
    for bad in ([], [0.1, np.nan], [[0.1, 0.2]], [0.1, np.inf]):
        with pytest.raises(ValueError, match="energies"):
            prop.time_average(bad, dt)
    for refs in ((np.zeros((2, D + 1)), np.zeros((2, D + 1))), (np.zeros((2, D)), np.zeros((3, D))), (np.zeros(D), np.zeros(D)),
                 (np.zeros((0, D)), np.zeros((0, D))), (np.full((1, D), np.nan), np.zeros((1, D)))):
        with pytest.raises(ValueError, match="references"):
            prop.time_average(energies, dt, references=refs)
    with pytest.raises(ValueError):
        prop.run(pot, dt, 2, E0, time_average=object())
    _, _, other = _prepared("hk_as5_chi002")
    with pytest.raises(ValueError, match="another"):
        other.run(pot, dt, 2, E0, time_average=acc)
    with pytest.raises(ValueError, match="empty"):
        acc.spectrum()
    assert prop.t == 0.0 and other.t == 0.0 and acc.steps == 0 and acc.pending == 0      # none of the refused calls took a step
    assert all(torch.equal(a, b) for a, b in zip(before, (prop._qp, prop._act, prop._mono, prop._c2, prop._sgn)))
    gw, potw, wm = _prepared("wm_as5_chi002")
    with pytest.raises(NotImplementedError):
        wm.time_average(energies, float(gw["dt"]))
    assert wm.t == 0.0


# ------------------------------------------------------------------------------------------- 6. driver

FCHK = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fchk")


def test_driver_key(tmp_path):
    from semiclassical_amd import driver, propagators as PR, units
    out, efile = tmp_path / "correlations.npz", tmp_path / "energies.npz"
    task = {"task": "dynamics", "propagator": "HK", "batch_size": 64, "num_trajectories": 128, "num_steps": 12, "time_step_fs": 0.005,
            "manual_seed": 0, "standard_errors": True, "time_averaged_spectrum": str(efile), "check_symplecticity_every": 2,
            "potential": {"type": "harmonic", "ground": os.path.join(FCHK, "methylium_s0.fchk"),
                          "excited": os.path.join(FCHK, "methylium_s1.fchk"), "coupling": os.path.join(FCHK, "methylium_s1.fchk")},
            "results": {"correlations": str(out)}}
    setup = driver.build_problem(task)
    energies = setup.zero_point_energy * np.linspace(0.5, 1.5, 5)
    np.savez(efile, energies=energies)
    plain = dict(task, results={"correlations": str(tmp_path / "plain.npz")})
    plain.pop("time_averaged_spectrum")
    driver.run_semiclassical_dynamics(plain, device="cuda")
    driver.run_semiclassical_dynamics(task, device="cuda")
    d = dict(np.load(out))
    nt, dt = 12, 0.005 / units.autime_to_fs
    assert int(d["trajectories"]) == 128
    assert np.array_equal(d["ta_energies"], energies) and float(d["ta_window"]) == nt * dt
    assert np.array_equal(d["ta_references_q"], setup.q0.numpy()[None, :]) and np.array_equal(d["ta_references_p"], setup.p0.numpy()[None, :])
    assert d["ta_spectrum"].shape == d["ta_spectrum_error"].shape == d["ta_spectrum_second_moment"].shape == (1, 5)
    assert (d["ta_spectrum"] > 0).all() and (d["ta_spectrum_error"] > 0).all()
    # without the key: exactly the keys there were, and the same numbers (methylium is a whole-loop shape: to 1e-12)
    p = dict(np.load(tmp_path / "plain.npz"))
    assert set(d) - set(p) == {"ta_energies", "ta_references_q", "ta_references_p", "ta_window", "ta_spectrum",
                               "ta_spectrum_second_moment", "ta_spectrum_error"}
    for key in p:
        if p[key].dtype.kind in "fc":
            assert abs(d[key] - p[key]).max() <= 1e-12 * max(abs(p[key]).max(), 1.0), key
        else:
            assert np.array_equal(d[key], p[key]), key
    # the same trajectories in a single-piece run() per batch, pooled with equal weights
    spectra = []
    for repetition in range(2):
        prop = PR.HermanKlukPropagator(setup.Gamma_0, setup.Gamma_0, device="cuda")
        prop.initial_conditions(setup.q0, setup.p0, setup.Gamma_0, ntraj=64, ntraj_total=64, seed=0, subsequence=repetition)
        acc = prop.time_average(energies, dt)
        prop.run(setup.potential, dt, nt, time_average=acc)
        spectra.append(acc.spectrum())
    want = 0.5 * (spectra[0] + spectra[1])
    dev = abs(d["ta_spectrum"] - want).max() / abs(want).max()
    print(f"driver: stored spectrum against single-piece runs {dev:.2e}")
    assert dev <= 1e-12
    # other energies, adding to the file: refused before anything runs, the file stays
    np.savez(efile, energies=energies[:4])
    again = dict(task, results={"correlations": str(out), "overwrite": False})
    again.pop("manual_seed")
    with pytest.raises(driver.ConfigurationError, match="energies"):
        driver.run_semiclassical_dynamics(again, device="cuda")
    after = dict(np.load(out))
    assert set(after) == set(d) and all(np.array_equal(after[k], d[k]) for k in d)
    # the same energies pool
    np.savez(efile, energies=energies)
    driver.run_semiclassical_dynamics(again, device="cuda")
    pooled = np.load(out)
    assert int(pooled["trajectories"]) == 256 and pooled["ta_spectrum"].shape == (1, 5)
