"""HermanKlukPropagator.cross_correlation / run(targets=...) (sc_hk_cross) against the numpy restatement
of the definition (tests/test_cross_host.py): the engine on the golden cases, the tile edges through the C-ABI, every route of
run(), the discard mask, the standard errors and the driver key."""
import os

import numpy as np
import pytest
import torch

from tests import cases
from tests.lib_spy import LibSpy as _Spy
from tests.test_cross_host import exact_overlaps, overlap_constants, psd_sqrt, restated_cross, width_targets, within_five_sigma

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


def _state(prop):
    """(q, p, v, Gamma_t, Gamma_0) read back from the engine, as numpy"""
    q, p = prop.current_positions_and_momenta()
    return (q.cpu().numpy().copy(), p.cpu().numpy().copy(), prop.coefficients().cpu().numpy(), prop._Gt.numpy(), prop._G0h.numpy())


def _targets(g, q, p, K, rng):
    """(q0, p0) first, then K random targets within 2 sigma of the ensemble in every mode -- the box shrunk by sqrt(D), so that the
    overlaps of a 60-mode target with the wavepacket are not all zero to working precision"""
    D = q.shape[0]
    u, w = rng.uniform(-1.0, 1.0, (K, D)), rng.uniform(-1.0, 1.0, (K, D))
    Q = q.mean(1) + 2.0 * q.std(1) * u / np.sqrt(D)
    P = p.mean(1) + 2.0 * p.std(1) * w / np.sqrt(D)
    return np.vstack((g["q0"], Q)), np.vstack((g["p0"], P))


# ------------------------------------------------------------------------------------------- 5. engine vs restatement

ENGINE_CASES = ["hk_1d", "hk_as5_chi002", "hk_as33", "hk_as60_n96", "hk_methylium", "hk_coumarin_harmonic"]


@pytest.mark.parametrize("name", ENGINE_CASES)
def test_engine_matches_restatement(name):
    """measured on the MI355X (deviation / max |X|): see DESIGN.md section 4.13"""
    g, pot, prop = _prepared(name, select=slice(0, 45) if name == "hk_as33" else None)
    for _ in range(3):
        prop.step(pot, float(g["dt"]))
    q, p, v, Gt, G0 = _state(prop)
    Q, P = _targets(g, q, p, 5, np.random.default_rng(len(name)))
    E0 = float(g["E0"])
    before = [t.clone() for t in (prop._qp, prop._act, prop._mono, prop._c2, prop._sgn)]      # (not prop.y: it may change the layout)
    C, sigma = prop.cross_correlation(Q, P, energy0_es=E0, standard_errors=True)
    assert C.shape == sigma.shape == (6,) and C.dtype == np.complex128
    assert np.array_equal(prop.cross_correlation(Q, P, energy0_es=E0), C)            # the same bits in every call
    rows = restated_cross(q, p, v, Gt, G0, Q, P)
    phase = np.exp(1j * prop.t * E0)
    want = (rows[:, 0] + 1j * rows[:, 1]) * phase
    scale = abs(want).max()
    print(f"{name}: |X_k| {np.array2string(abs(want), precision=3)}, deviation {abs(C - want).max() / scale:.2e} of the largest")
    assert scale > 0 and abs(C - want).max() <= TOL * scale
    # the (q0, p0) target is the autocorrelation function
    auto = prop.autocorrelation(E0)
    print(f"{name}: |C_0 - C_auto| {abs(C[0] - auto):.2e}")
    assert abs(C[0] - auto) <= TOL * scale
    # standard errors: the host's algebra on the restated second moments
    from semiclassical_amd import hostmath
    theta = prop.t * E0
    want_sigma = hostmath.standard_errors(want, hostmath.rotate_second_moments(rows[:, 2:5], theta), prop._ntraj_norm)
    assert np.allclose(sigma.real, want_sigma.real, rtol=1e-6, atol=1e-9 * scale) and np.allclose(sigma.imag, want_sigma.imag, rtol=1e-6, atol=1e-9 * scale)
    # nothing changed: the state, and the step that follows
    assert all(torch.equal(a, b) for a, b in zip(before, (prop._qp, prop._act, prop._mono, prop._c2, prop._sgn)))
    _, pot2, twin = _prepared(name, select=slice(0, 45) if name == "hk_as33" else None)
    for _ in range(4):
        twin.step(pot2, float(g["dt"]))
    prop.step(pot, float(g["dt"]))
    assert torch.equal(prop.y, twin.y) and torch.equal(prop._c2, twin._c2) and torch.equal(prop._sgn, twin._sgn)


def test_refusals():
    g, pot, prop = _prepared("hk_as5_chi002")
    D = prop.dim
    ok = np.zeros((2, D))
    bad = ok.copy()
    bad[1, 2] = np.inf
    for Q, P in ((np.zeros((2, D + 1)), np.zeros((2, D + 1))), (ok, np.zeros((3, D))), (np.zeros(D), np.zeros(D)),
                 (np.zeros((0, D)), np.zeros((0, D))), (bad, ok), (ok, bad * np.nan)):
        with pytest.raises(ValueError):
            prop.cross_correlation(Q, P)
        with pytest.raises(ValueError):
            prop.run(pot, float(g["dt"]), 2, targets=(Q, P))
    with pytest.raises(ValueError, match="use_graph"):
        prop.run(pot, float(g["dt"]), 4, targets=(ok, ok), use_graph=True)
    slots = torch.zeros((2, 5), device=prop.device)
    with pytest.raises(ValueError, match="cross"):
        prop.run(pot, float(g["dt"]), 2, slots=slots, targets=(ok, ok))
    for cross in (torch.zeros((2, 2, 4), device=prop.device), torch.zeros((1, 2, 5), device=prop.device),
                  torch.zeros((2, 3, 5), device=prop.device), torch.zeros((2, 2, 5)), torch.zeros((2, 2, 5), device=prop.device, dtype=torch.float32)):
        with pytest.raises(ValueError, match="cross"):
            prop.run(pot, float(g["dt"]), 2, slots=slots, targets=(ok, ok), cross=cross)
    with pytest.raises(ValueError, match="targets"):
        prop.run(pot, float(g["dt"]), 2, cross=torch.zeros((2, 2, 5), device=prop.device))
    assert prop.t == 0.0                                        # none of the refused calls took a step
    gw, potw, wm = _prepared("wm_as5_chi002")
    with pytest.raises(NotImplementedError):
        wm.cross_correlation(ok, ok)
    with pytest.raises(NotImplementedError):
        wm.run(potw, float(gw["dt"]), 2, targets=(ok, ok))


# ------------------------------------------------------------------------------------------- 6. tile edges through the C-ABI

def _synthetic(rng, n, D):
    """a state with every ingredient of v_i non-trivial: c2 on both sides of the branch cut, both signs"""
    s = 1.0 / np.sqrt(D)
    return dict(q=rng.normal(0.0, 0.6 * s, (D, n)), p=rng.normal(0.0, 0.9 * s, (D, n)), act=rng.uniform(-3.0, 3.0, n),
                c2=rng.normal(size=n) + 1j * rng.normal(size=n), sgn=rng.choice([-1.0, 1.0], n),
                vi=rng.normal(size=n) + 1j * rng.normal(size=n), probi=rng.uniform(0.5, 1.5, n))


def _widths(rng, D, diag):
    if diag:
        return np.diag(rng.uniform(0.6, 1.8, D)), np.diag(rng.uniform(0.6, 1.8, D))
    def spd():
        V = np.linalg.qr(rng.normal(size=(D, D)))[0]
        return (V * rng.uniform(0.6, 1.8, D)) @ V.T
    return spd(), spd()


class _Cross(object):
    """sc_hk_cross on a synthetic state: device buffers built once per (n, D), targets and masks vary"""

    def __init__(self, st, Gt, G0, diag, mc_norm):
        from semiclassical_amd import _lib
        self.lib, self.st, self.mc_norm, self.diag = _lib, st, mc_norm, diag
        D, n = st["q"].shape
        self.D, self.n = D, n
        dev = lambda a: torch.from_numpy(np.array(a, dtype=np.float64, order="C")).to("cuda")
        cx = lambda a: torch.view_as_real(torch.from_numpy(np.array(a, dtype=complex, order="C"))).contiguous().to("cuda")
        A, B, C, self.fac = overlap_constants(Gt, G0)
        self.La, self.Lb, self.C = psd_sqrt(A), psd_sqrt(B), C
        if diag:
            self.consts = [dev(np.diag(self.La)), dev(np.diag(self.Lb)), dev(np.diag(C))]
        else:
            self.consts = [dev(self.La), dev(self.Lb), dev(C.T)]
        self.bufs = dict(qp=dev(np.vstack((st["q"], st["p"])).T), act=dev(st["act"]), c2=cx(st["c2"]), sgn=dev(st["sgn"]),
                         vi=cx(st["vi"]), probi=dev(st["probi"]))
        b = self.bufs
        self.state = _lib.sc_state(n=n, dim=D, mono_layout=0, qp=b["qp"].data_ptr(), act=b["act"].data_ptr(), mono=None,
                                   c2=b["c2"].data_ptr(), sgn=b["sgn"].data_ptr(), work=None, flags=None)
        self.operands = None if diag else torch.full((n, 4 * D), np.nan, device="cuda")
        with np.errstate(invalid="ignore"):                      # (the non-finite state of the mask test)
            self.v = st["sgn"] * np.sqrt(st["c2"]) * np.exp(1j * st["act"]) * st["vi"] / (mc_norm * st["probi"])

    def __call__(self, Q, P, kept=None, cursor=None, rows=1):
        lib, ptr = self.lib.lib, self.lib.ptr
        K = Q.shape[0]
        tg = np.hstack((Q @ self.La.T, P @ self.Lb.T, Q, P @ self.C.T, P))
        tg = torch.from_numpy(np.ascontiguousarray(tg)).to("cuda")
        part = torch.full((int(lib.sc_hk_cross_rows(self.n, K)) * K * 5,), np.nan, device="cuda")
        out = torch.full((rows, K, 5), np.nan, device="cuda")
        mask = None if kept is None else torch.from_numpy(np.asarray(kept, dtype=np.uint8)).to("cuda")
        cur = None if cursor is None else torch.tensor([cursor], dtype=torch.int64, device="cuda")
        c = self.consts
        self.lib.check(lib.sc_hk_cross(self.state, ptr(c[0]), ptr(c[1]), ptr(c[2]), int(self.diag), float(self.fac), ptr(tg), K,
                                       ptr(self.bufs["vi"]), ptr(self.bufs["probi"]), self.mc_norm, ptr(mask), ptr(self.operands),
                                       ptr(part), ptr(out), ptr(cur), torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        if cur is not None:
            assert int(cur.item()) == cursor                     # read, not advanced
        return out.cpu().numpy()


SIZES = (1, 63, 64, 65, 130)


@pytest.mark.parametrize("diag,D", [(True, 1), (True, 15), (True, 16), (True, 17), (True, 33), (False, 2), (False, 12)])
def test_tile_edges_through_the_c_abi(diag, D):
    rng = np.random.default_rng(100 * D + diag)
    Gt, G0 = _widths(rng, D, diag)
    worst = 0.0
    for n in SIZES:
        st = _synthetic(rng, n, D)
        call = _Cross(st, Gt, G0, diag, mc_norm=float(n) * 1.7)
        masks = [None, np.arange(n) >= 64, np.arange(n) == n // 2]      # none; the first 64-band discarded; a single one kept
        for K in SIZES:
            s = 1.0 / np.sqrt(D)
            Q, P = rng.normal(0.0, 0.6 * s, (K, D)), rng.normal(0.0, 0.9 * s, (K, D))
            for kept in masks:
                got = call(Q, P, kept)[0]
                want = restated_cross(st["q"], st["p"], call.v, Gt, G0, Q, P, kept)
                assert got.shape == want.shape == (K, 5) and np.isfinite(got).all()
                for col in range(5):
                    scale = abs(want[:, col]).max()
                    dev = abs(got[:, col] - want[:, col]).max()
                    assert dev <= TOL * scale, (n, K, kept is not None, col, dev, scale)
                    worst = max(worst, dev / scale if scale > 0 else 0.0)
                if kept is not None and not kept.any():
                    assert not got.any()                         # nobody kept: exact zeros
                assert np.array_equal(call(Q, P, kept)[0], got)  # two calls, the same bits
        # a non-finite state of a discarded trajectory never reaches the sums
        if n > 1:
            dirty = dict(st, q=st["q"].copy(), c2=st["c2"].copy())
            dirty["q"][:, 0], dirty["c2"][0] = np.nan, np.inf
            kept = np.arange(n) > 0
            got = _Cross(dirty, Gt, G0, diag, mc_norm=float(n) * 1.7)(Q, P, kept)[0]
            assert np.array_equal(got, call(Q, P, kept)[0])
    # with a cursor the row goes to out[*cursor]
    got = call(Q, P, None, cursor=2, rows=3)
    assert np.isnan(got[:2]).all() and np.array_equal(got[2], call(Q, P)[0])
    print(f"diag={diag} D={D}: largest deviation of a column {worst:.2e} of its largest entry")


def test_c_abi_refusals():
    from semiclassical_amd import _lib
    rng = np.random.default_rng(0)
    Gt, G0 = _widths(rng, 3, True)
    call = _Cross(_synthetic(rng, 5, 3), Gt, G0, True, 5.0)
    lib, ptr = _lib.lib, _lib.ptr
    buf = torch.zeros(64, device="cuda")
    c = call.consts
    args = lambda **kw: [kw.get("st", call.state), ptr(c[0]), ptr(c[1]), ptr(c[2]), kw.get("diag", 1), 1.0, ptr(buf), kw.get("K", 1),
                         ptr(call.bufs["vi"]), ptr(call.bufs["probi"]), 5.0, None, None, ptr(buf), kw.get("out", ptr(buf)), None, None]
    assert lib.sc_hk_cross(*args(K=0)) == -1 and lib.sc_hk_cross(*args(out=None)) == -1
    assert lib.sc_hk_cross(*args(diag=0)) == -1                  # dense widths without the operand scratch
    assert lib.sc_hk_cross(*args(K=65536)) == -2 and b"65535" in lib.sc_last_error()
    big = _lib.sc_state.from_buffer_copy(call.state)
    big.dim = 513
    assert lib.sc_hk_cross(*args(st=big)) == -2 and b"512" in lib.sc_last_error()
    many = _lib.sc_state.from_buffer_copy(call.state)
    many.n = 64 * 65535 + 1
    assert lib.sc_hk_cross(*args(st=many)) == -2 and str(64 * 65535).encode() in lib.sc_last_error()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------- 7. run(targets=...)

ROUTES = [
    # case, nt, attributes, the entry point that has to run, bit-identical rows promised
    ("hk_as60_n96", 7, {"visit_min_bytes": 0, "visit_steps": 3}, "sc_hk_step_visit", True),
    ("hk_as60_n96", 7, {"visit_min_bytes": 0, "visit_steps": 2}, "sc_hk_step_multi", True),
    ("hk_as60_n96", 7, {"pair_steps": False}, "sc_hk_step", True),
    ("hk_as33", 5, {"visit_min_bytes": 0, "visit_steps": 3}, "sc_hk_step_visit", True),
    ("hk_as33", 5, {"visit_min_bytes": 0, "visit_steps": 2}, "sc_hk_step_multi", True),
    ("hk_as33", 5, {"pair_steps": False}, "sc_hk_step", True),
    ("hk_as5_chi002", 5, {}, "sc_hk_step", False),                      # a whole-loop shape: step by step with targets
    ("hk_coumarin_harmonic", 3, {}, "sc_hk_step_modal", False),
]


@pytest.mark.parametrize("name,nt,attrs,entry,bits", ROUTES, ids=[f"{r[0]}-{r[3]}" for r in ROUTES])
def test_run_with_targets(name, nt, attrs, entry, bits, monkeypatch):
    g, pot, prop = _prepared(name, **attrs)
    dt, E0 = float(g["dt"]), float(g["E0"])
    D = prop.dim
    Q, P = _targets(g, g["zi"][:D], g["zi"][D:], 4, np.random.default_rng(nt))
    blocks = torch.zeros((nt, 4, 4), device=prop.device)
    spy = _Spy(monkeypatch)
    C, k, sC, sk, X, sX = prop.run(pot, dt, nt, E0, standard_errors=True, blocks=blocks, targets=(Q, P))
    monkeypatch.undo()
    assert spy.seen.get(entry, 0) > 0 and spy.seen.get("sc_hk_cross", 0) == nt, spy.seen
    assert "sc_hk_run" not in spy.seen and "sc_hk_run_m" not in spy.seen
    assert X.shape == sX.shape == (nt, 5) and X.dtype == np.complex128
    # without targets: the same C, k, errors, blocks and final state, bit for bit (a whole-loop shape: under the step-at-a-time loop)
    _, pot2, twin = _prepared(name, **attrs)
    if name == "hk_as5_chi002":
        twin._whole_loop_ok = False
    blocks2 = torch.zeros((nt, 4, 4), device=prop.device)
    C2, k2, sC2, sk2 = twin.run(pot2, dt, nt, E0, standard_errors=True, blocks=blocks2)
    for a, b in ((C, C2), (k, k2), (sC, sC2), (sk, sk2)):
        assert np.array_equal(a, b)
    assert torch.equal(blocks, blocks2) and torch.equal(prop.y, twin.y) and torch.equal(prop._c2, twin._c2)
    assert prop.t == twin.t
    # row k of X is cross_correlation() of the state before step k
    _, pot3, loop = _prepared(name, **attrs)
    want, want_sigma = [], []
    for _ in range(nt):
        c, s = loop.cross_correlation(Q, P, energy0_es=E0, standard_errors=True)
        want.append(c)
        want_sigma.append(s)
        loop.step(pot3, dt)
    want, want_sigma = np.array(want), np.array(want_sigma)
    scale = abs(want).max()
    print(f"{name} {entry}: run() against the step-by-step loop {abs(X - want).max() / scale:.2e} of max |X| = {scale:.3e}")
    if bits:
        assert np.array_equal(X, want) and np.array_equal(sX, want_sigma)
    else:
        assert abs(X - want).max() <= 1e-12 * scale
    # the first row is the autocorrelation's at the (q0, p0) target
    assert abs(X[:, 0] - C).max() <= TOL * abs(C).max()
    # slots= given: the raw rows in the caller's buffer give the same numbers
    _, pot4, raw = _prepared(name, **attrs)
    slots, cross = torch.zeros((nt, 5), device=prop.device), torch.full((nt + 1, 5, 5), np.nan, device=prop.device)
    assert raw.run(pot4, dt, nt, E0, slots=slots, targets=(Q, P), cross=cross) is None
    raw.synchronize()
    X4, sX4 = raw.finalize_cross(cross[:nt], 0.0, dt, E0, raw._ntraj_norm)
    assert np.array_equal(X4, X) and np.array_equal(sX4, sX) and torch.isnan(cross[nt]).all()


# ------------------------------------------------------------------------------------------- 8. under a discard mask

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
    q, p, v, Gt, G0 = _state(prop)
    Q, P = _targets(g, q, p, 5, np.random.default_rng(8))
    rows = restated_cross(q, p, v, Gt, G0, Q, P, kept)           # v carries the unchanged N
    want = (rows[:, 0] + 1j * rows[:, 1]) * np.exp(1j * prop.t * E0)
    everyone = restated_cross(q, p, v, Gt, G0, Q, P)
    assert abs(everyone[:, 0] - rows[:, 0]).max() > 1e-3 * abs(rows[:, 0]).max()      # the mask matters
    C = prop.cross_correlation(Q, P, energy0_es=E0)
    scale = abs(want).max()
    print(f"masked: deviation {abs(C - want).max() / scale:.2e} of max |X|")
    assert abs(C - want).max() <= TOL * scale
    assert abs(C[0] - prop.autocorrelation(E0)) <= TOL * scale
    t0 = prop.t
    out = prop.run(pot, dt, 2, E0, targets=(Q, P))
    X = out[-1]
    assert len(out) == 3 and prop.t > t0 and abs(X[0] - want).max() <= TOL * scale      # row 0: the state the call above saw
    assert abs(X[:, 0] - out[0]).max() <= TOL * scale


# ------------------------------------------------------------------------------------------- 9. standard errors mean something

def test_standard_errors_cover_the_exact_overlap():
    """t = 0 on the fixture's own initial conditions: every C_k(0) within 5 sigma_k of the closed-form <phi_k|phi_0>, for (q0, p0)
    and one width to either side along modes 0 and 4 (checked on the CPU first: test_cross_host.py::test_five_sigma_at_t0_on_the_cpu)"""
    g, pot, prop = _prepared("hk_as5_chi002")
    Q, P = width_targets(g)
    C, sigma = prop.cross_correlation(Q, P, energy0_es=float(g["E0"]), standard_errors=True)
    exact = exact_overlaps(g, Q, P)
    for k in range(len(Q)):
        print(f"target {k}: C {C[k]:.6f}  exact {exact[k]:.6f}  sigma {sigma[k]:.2e}")
    assert (sigma.real[1:] > 1e-3).all() and (sigma.real[1:] < 0.1).all()        # error bars of the size 1/sqrt(256) suggests
    ok = within_five_sigma(C, sigma, exact)
    assert ok.all(), ok


# ------------------------------------------------------------------------------------------- 10. driver

FCHK = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fchk")


def test_driver_key(tmp_path):
    from semiclassical_amd import driver
    out, tfile = tmp_path / "correlations.npz", tmp_path / "targets.npz"
    task = {"task": "dynamics", "propagator": "HK", "batch_size": 64, "num_trajectories": 128, "num_steps": 12, "time_step_fs": 0.005,
            "manual_seed": 0, "standard_errors": True, "cross_correlation_targets": str(tfile),
            "potential": {"type": "harmonic", "ground": os.path.join(FCHK, "methylium_s0.fchk"),
                          "excited": os.path.join(FCHK, "methylium_s1.fchk"), "coupling": os.path.join(FCHK, "methylium_s1.fchk")},
            "results": {"correlations": str(out)}}
    setup = driver.build_problem(task)
    q0, p0 = setup.q0.numpy(), setup.p0.numpy()
    D = q0.shape[0]
    e, V = np.linalg.eigh(setup.Gamma_0.numpy())
    shift = 0.3 / np.sqrt(e[-1]) * V[:, -1]                      # 0.3 widths along the stiffest direction of Gamma_0 (singular: rank 6)
    Q = np.vstack((q0 + shift, q0, q0 - shift))
    P = np.vstack((p0, p0, p0))
    np.savez(tfile, q=Q, p=P)
    driver.run_semiclassical_dynamics(task, device="cuda")
    d = dict(np.load(out))
    assert int(d["trajectories"]) == 128
    assert np.array_equal(d["cross_targets_q"], Q) and np.array_equal(d["cross_targets_p"], P)
    X = d["cross_correlation"]
    assert X.shape == (12, 3) and d["cross_correlation_error"].shape == (12, 3) and d["cross_correlation_second_moment"].shape == (12, 3, 3)
    dev = abs(X[:, 1] - d["autocorrelation"]).max()
    print(f"driver: |cross_correlation[:, k0] - autocorrelation| {dev:.2e}")
    assert dev <= 1e-9
    # a displaced target overlaps less: |<phi_k|phi_0>| = exp(-0.3^2 / 4) for Gamma_i = Gamma_t = Gamma_0
    assert abs(abs(X[0, 0]) - np.exp(-0.0225)) < 0.05 and abs(abs(X[0, 2]) - np.exp(-0.0225)) < 0.05
    # other targets, adding to the file: refused before anything runs
    np.savez(tfile, q=Q[:2], p=P[:2])
    again = dict(task, results={"correlations": str(out), "overwrite": False})
    again.pop("manual_seed")
    with pytest.raises(driver.ConfigurationError, match="targets"):
        driver.run_semiclassical_dynamics(again, device="cuda")
    without = dict(again)
    without.pop("cross_correlation_targets")
    with pytest.raises(driver.ConfigurationError):
        driver.run_semiclassical_dynamics(without, device="cuda")
    after = dict(np.load(out))
    assert set(after) == set(d) and all(np.array_equal(after[k], d[k]) for k in d)
    # the same targets pool
    np.savez(tfile, q=Q, p=P)
    driver.run_semiclassical_dynamics(again, device="cuda")
    pooled = np.load(out)
    assert int(pooled["trajectories"]) == 256 and abs(pooled["cross_correlation"][:, 1] - pooled["autocorrelation"]).max() <= 1e-9
