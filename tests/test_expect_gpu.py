"""HermanKlukPropagator.expectation / wavepacket_moments / energy_expectation (sc_pair_expect) against the numpy
restatement of tests/expect_cases.py on the oracle's state, against norm() and reduced_density(), the tile and chunk edges through
the C-ABI, the untouched state and the refusals."""
import numpy as np
import pytest
import torch

from tests import cases, expect_cases as EC
from tests.test_density_host import HBAR, overlap_constants

pytestmark = pytest.mark.gpu
torch.set_default_dtype(torch.float64)

TOL = 1e-9          # x A_a = sum_ij |T_ij F_a,ij|: the factor norm() and reduced_density() carry
MEANINGFUL = 5e-3   # |E_a| / A_a at least: the bound cannot hide a wrong factor behind cancellation


def _advanced(name, steps, select=None, run=False, oracle=True):
    """the engine's propagator and the oracle's state (q, p, v, Gamma_t as numpy) after `steps` steps"""
    from oracle import norm_oracle
    from tests.engine_cases import engine_potential, engine_propagator
    g = cases.load(name)
    if select is not None:
        g["zi"], g["probi"] = g["zi"][:, select], g["probi"][select]
    pot, prop = engine_potential(g), engine_propagator(g)
    if run:
        prop.run(pot, float(g["dt"]), steps)
    else:
        for _ in range(steps):
            prop.step(pot, float(g["dt"]))
    if not oracle:
        return g, pot, prop, None
    ref, opot = cases.oracle_propagator(g), cases.oracle_potential(g)
    for _ in range(steps):
        ref.step(opot, float(g["dt"]))
    q, p = ref.current_positions_and_momenta()
    return g, pot, prop, (q.numpy().copy(), p.numpy().copy(), norm_oracle.coefficients(ref).numpy(), g["Gamma_t"])


def _normalised_bound(E, A, N2, AN):
    """of E_a / N2 when E_a is off by TOL A_a and N2 by TOL AN = TOL sum |T|"""
    return TOL * (A + abs(E) * AN / abs(N2)) / abs(N2)


_STATES = {}


def _case(name):
    if name not in _STATES:
        _, _, prop, state = _advanced(name, 3)
        _STATES[name] = (prop, state)
    return _STATES[name]


# ------------------------------------------------------------------------------------------- 1. engine vs restatement

def _check_against_restatement(name, prop, state):
    q, p, v, G = state
    full_rank = round(np.trace(EC.projector(G))) == G.shape[0]
    # seed 6: with the oracle alone the smallest |E_a| / A_a of every state used here is 1.76e-2 (p on hk_1d, which has no direction
    # to choose) and at least 0.16 everywhere else; some seeds put <u.p> of hk_as5_chi002 or hk_as60_n96 next to zero
    c, m, K, n, W = EC.standard_operators(np.random.default_rng(6), G)
    E, A, N2 = EC.restated_expectation(q, p, v, G, c, m, K, n, W)
    got, norm2 = prop.expectation(c, m, K, n, W, normalise=False)
    assert got.shape == (6,) and got.dtype == np.complex128 and isinstance(norm2, float)
    for a, label in enumerate(("x", "x^2", "p", "p^2", "mixed", "1")):
        print(f"{name} {label:5s}: |E| / A = {abs(got[a]) / A[a]:.3e}, |E - restatement| / A = {abs(got[a] - E[a]) / A[a]:.2e}, "
              f"|Im E| / A = {abs(got[a].imag) / A[a]:.2e}")
    assert (abs(got) >= MEANINGFUL * A).all()
    assert (abs(got - E) <= TOL * A).all()
    if full_rank:                                           # (the oracle's overlap matrix of methylium is Hermitian to 1.3e-7 only)
        assert (abs(got.imag) <= TOL * A).all()
    # norm2: the restatement's, norm()**2, and the value of the constant 1
    assert abs(norm2 - N2.real) <= TOL * A[5] and got[5].real == norm2
    assert abs(norm2 - prop.norm() ** 2) <= 1e-9 * norm2
    # normalised values, and a call with fewer parts
    vals, again = prop.expectation(c, m, K, n, W)
    assert again == norm2 and (abs(vals - got / norm2) <= 1e-15 * abs(vals)).all()
    few, _ = prop.expectation(x=m[:1], normalise=False)
    assert few.shape == (1,) and abs(few[0] - got[0]) <= 1e-13 * A[0]


@pytest.mark.parametrize("name", ["hk_1d", "hk_as5_chi002", "hk_methylium", "hk_as33", "hk_as60_n96"])
def test_engine_matches_restatement(name):
    prop, state = _case(name)
    _check_against_restatement(name, prop, state)


def test_after_run_on_the_pair_path():
    """D = 33: run() advances two steps per launch and leaves the state of its last single step"""
    _, _, prop, state = _advanced("hk_as33", 5, run=True)
    _check_against_restatement("hk_as33 after run()", prop, state)


# ------------------------------------------------------------------------------------------- 2. the other routes of the engine

def test_moments_of_the_reduced_density():
    """<x_0> N2 and <x_0^2> N2 against int s rho and int s^2 rho along mode 0: trapezoid sums on a uniform grid of spacing <=
    sigma / 2 over [min u.q - 8 sigma, max u.q + 8 sigma], the recipe and the bound of tests/test_density_gpu.py"""
    _, _, prop, _ = _advanced("hk_as5_chi002", 5, oracle=False)
    D = prop.dim
    q = prop.current_positions_and_momenta()[0].cpu().numpy()
    _, B, _, _ = overlap_constants(prop._Gt.cpu().numpy())
    sig, uq = np.sqrt(B[0, 0]), q[0]
    lo, hi = uq.min() - 8.0 * sig, uq.max() + 8.0 * sig
    s = np.linspace(lo, hi, int(np.ceil((hi - lo) / (0.5 * sig))) + 1)
    assert s[1] - s[0] <= 0.5 * sig
    rho = prop.reduced_density(0, s)[0]
    trapezoid = lambda f: (s[1] - s[0]) * (f.sum() - 0.5 * (f[0] + f[-1]))
    u = np.zeros((2, D))
    u[0, 0] = 1.0
    K = np.zeros((2, D, D))
    K[1, 0, 0] = 2.0
    vals, norm2 = prop.expectation(x=u, xx=K, normalise=False)
    first, second = trapezoid(s * rho), trapezoid(s * s * rho)
    print(f"int s rho = {first:.15g}, <x_0> N2 = {vals[0].real:.15g}: {abs(first - vals[0].real) / abs(first):.2e}; "
          f"int s^2 rho = {second:.15g}, <x_0^2> N2 = {vals[1].real:.15g}: {abs(second - vals[1].real) / abs(second):.2e}")
    assert abs(vals[0].real - first) <= 1e-6 * abs(first)
    assert abs(vals[1].real - second) <= 1e-6 * abs(second)
    assert abs(trapezoid(rho) - norm2) <= 1e-6 * norm2


def test_wavepacket_moments():
    _, _, prop, (q, p, v, G) = _advanced("hk_as5_chi000", 3)
    D = prop.dim
    dense = np.random.default_rng(21).uniform(0.5, 1.5, D)
    for directions, U in ((None, np.eye(D)), ([0, D - 1], np.eye(D)[[0, D - 1]]), (dense, dense[None, :])):
        Md = U.shape[0]
        sq, zv, zm = np.stack([2.0 * np.outer(u, u) for u in U]), np.zeros((Md, D)), np.zeros((Md, D, D))
        E, A, N2 = EC.restated_expectation(q, p, v, G, None, np.concatenate((U, zv, zv, zv)), np.concatenate((zm, sq, zm, zm)),
                                           np.concatenate((zv, zv, U, zv)), np.concatenate((zm, zm, zm, sq)))
        AN = abs(EC.pair_terms(q, p, v, G)[0]).sum()
        want, tol = (E / N2).real, _normalised_bound(E, A, N2, AN)
        got = prop.wavepacket_moments() if directions is None else prop.wavepacket_moments(directions)
        assert sorted(got) == ["norm2", "p", "var_p", "var_x", "x"] and abs(got["norm2"] - N2.real) <= TOL * AN
        x, xx, pm, pp = (want[k * Md:(k + 1) * Md] for k in range(4))
        tx, txx, tp, tpp = (tol[k * Md:(k + 1) * Md] for k in range(4))
        assert got["x"].shape == (Md,) and (abs(got["x"] - x) <= tx).all() and (abs(got["p"] - pm) <= tp).all()
        assert (abs(got["var_x"] - (xx - x ** 2)) <= txx + 2.0 * abs(x) * tx).all()
        assert (abs(got["var_p"] - (pp - pm ** 2)) <= tpp + 2.0 * abs(pm) * tp).all()
        assert (got["var_x"] > 0).all() and (got["var_p"] > 0).all()


def test_energy_expectation():
    """hk_as5_chi000: V = sum omega^2 x^2 / 2, unit masses"""
    g, pot, prop, (q, p, v, G) = _advanced("hk_as5_chi000", 3)
    D = prop.dim
    K, W = np.diag(g["omega"] ** 2)[None], np.eye(D)[None]
    E, A, N2 = EC.restated_expectation(q, p, v, G, None, None, K, None, W)
    AN = abs(EC.pair_terms(q, p, v, G)[0]).sum()
    got = prop.energy_expectation(pot)
    print(f"<H> = {got:.15g}, restatement {(E[0] / N2).real:.15g}, |E| / A = {abs(E[0]) / A[0]:.3e}")
    assert isinstance(got, float) and abs(E[0]) >= MEANINGFUL * A[0]
    assert abs(got - (E[0] / N2).real) <= _normalised_bound(E, A, N2, AN)[0]


def test_energy_of_one_gaussian():
    """n = 1: <H> = sum_k (p_k^2 + hbar^2 Gamma_kk / 2) / 2 + omega_k^2 (q_k^2 + B_kk) / 2 with the engine's own q, p; the harmonic
    molecule of methylium's fixture is refused for its singular Gamma_t"""
    g, pot, prop, _ = _advanced("hk_as5_chi000", 2, select=slice(3, 4), oracle=False)
    q, p = (t.cpu().numpy()[:, 0] for t in prop.current_positions_and_momenta())
    G = g["Gamma_t"]
    _, B, _, _ = overlap_constants(G)
    want = 0.5 * np.sum(p ** 2 + 0.5 * HBAR ** 2 * np.diag(G)) + 0.5 * np.sum(g["omega"] ** 2 * (q ** 2 + np.diag(B)))
    got = prop.energy_expectation(pot)
    assert abs(got - want) <= TOL * abs(want)
    vals, norm2 = prop.expectation(x=np.eye(prop.dim), p=np.eye(prop.dim))
    assert abs(vals - (q + p)).max() <= TOL * abs(q + p).max() and abs(norm2 - prop.norm() ** 2) <= TOL * norm2


# ------------------------------------------------------------------------------------------- 3. the state is not touched

def test_state_is_untouched():
    from tests.engine_cases import engine_potential, engine_propagator
    g = cases.load("hk_as5_chi000")
    pot, dt, E0 = engine_potential(g), float(g["dt"]), float(g["E0"])
    prop, twin = engine_propagator(g), engine_propagator(g)
    c, m, K, n, W = EC.standard_operators(np.random.default_rng(5), g["Gamma_t"])
    outs = []
    for pr, calls in ((prop, True), (twin, False)):
        pr.step(pot, dt)
        if calls:
            first = pr.expectation(c, m, K, n, W)
            second = pr.expectation(c, m, K, n, W)
            assert np.array_equal(first[0], second[0]) and first[1] == second[1]            # the same bits in every call
            pr.wavepacket_moments([0, 1])
            pr.energy_expectation(pot)
        assert pr.t == dt
        outs.append(pr.run(pot, dt, 2, E0))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    for name in ("_qp", "_act", "_c2", "_sgn"):
        assert torch.equal(getattr(prop, name), getattr(twin, name)), name
    for a, b in zip(prop.monodromy_matrices(), twin.monodromy_matrices()):
        assert torch.equal(a, b)
    assert torch.equal(prop.coefficients(), twin.coefficients())


# ------------------------------------------------------------------------------------------- 4. refusals

def test_refusals():
    prop, _ = _case("hk_as5_chi002")
    D = prop.dim
    sym = np.eye(D)
    with pytest.raises(ValueError, match="at least one"):
        prop.expectation()
    for kwargs in (dict(x=np.ones(D)), dict(x=np.ones((1, D + 1))), dict(xx=np.ones((1, D))), dict(c=np.ones(2), p=np.ones((1, D))),
                   dict(pp=sym), dict(c=np.array([np.nan])), dict(x=np.full((1, D), np.inf))):
        with pytest.raises(ValueError, match="operators"):
            prop.expectation(**kwargs)
    skew = sym.copy()
    skew[0, 1] = 1e-9
    with pytest.raises(ValueError, match="xx of operator 1 is not symmetric"):
        prop.expectation(xx=np.stack([sym, skew]))
    with pytest.raises(ValueError, match="pp of operator 0 is not symmetric"):
        prop.expectation(pp=skew[None])
    for bad in (5, [0, 7], np.ones(4), np.zeros(D)):
        with pytest.raises(ValueError):
            prop.wavepacket_moments(bad)
    from semiclassical_amd import potentials as P
    with pytest.raises(NotImplementedError, match="constant Hessian"):
        prop.energy_expectation(P.MorsePotential(torch.ones(D), torch.full((D,), 0.02), torch.zeros(D)))
    with pytest.raises(NotImplementedError, match="constant Hessian"):
        prop.energy_expectation(P.NonHarmonicPotential())
    with pytest.raises(ValueError, match="dimensions"):
        prop.energy_expectation(P.MorsePotential(torch.ones(D + 1), torch.zeros(D + 1), torch.zeros(D + 1)))


def test_singular_width_matrix_refusals():
    from tests.engine_cases import engine_potential
    prop, _ = _case("hk_methylium")
    G = prop._Gt.cpu().numpy()
    e, V = np.linalg.eigh(G)
    inside, null = V[:, np.argmax(e)], V[:, np.argmin(abs(e))]
    prop.expectation(x=inside[None], pp=2.0 * np.outer(inside, inside)[None])
    with pytest.raises(ValueError, match="x of operator 1 .* range of Gamma_t"):
        prop.expectation(x=np.stack([inside, inside + 1e-6 * null]))
    with pytest.raises(ValueError, match="p of operator 0 .* range of Gamma_t"):
        prop.expectation(p=null[None])
    with pytest.raises(ValueError, match="pp of operator 0 .* range of Gamma_t"):
        prop.expectation(pp=np.eye(G.shape[0])[None])
    with pytest.raises(ValueError, match="directions in the range"):
        prop.wavepacket_moments()
    assert prop.wavepacket_moments(inside)["var_x"][0] > 0
    with pytest.raises(ValueError, match="range of Gamma_t"):
        prop.wavepacket_moments(null)
    with pytest.raises(ValueError, match="singular"):
        prop.energy_expectation(engine_potential(cases.load("hk_methylium")))


def test_wm_and_thermal_ensembles_refuse():
    from tests.engine_cases import engine_propagator
    from tests.test_thermal_gpu import _golden_case
    wm = engine_propagator(cases.load("wm_as5_chi002"))
    for call in (lambda: wm.expectation(c=np.ones(1)), lambda: wm.wavepacket_moments(0)):
        with pytest.raises(NotImplementedError, match="per-trajectory widths"):
            call()
    _, pot, _, prop, _, _, _ = _golden_case("hk_as5_chi002", 0.006, n=67)
    for call in (lambda: prop.expectation(c=np.ones(1)), lambda: prop.wavepacket_moments(0), lambda: prop.energy_expectation(pot)):
        with pytest.raises(NotImplementedError, match="thermal ensemble"):
            call()


# ------------------------------------------------------------------------------------------- 5. tile and chunk edges through the C-ABI

def _pack(q, p, v, G, conj, fac, centre):
    """the operands norm() packs for one set of trajectories (rows = trajectories); q, p (D, n)"""
    A, B, C, _ = overlap_constants(G)
    q, p = (q - centre[:, None]).T, p.T
    Aq, Bp, Cp = q @ A.T, p @ B.T, p @ C.T
    cc = (q * Cp).sum(1)
    return dict(X1=np.hstack((q, p)), Y1=np.hstack((Aq, Bp)), X2=np.hstack((q, Cp, q)), Y2=np.hstack((p, -q, -Cp)),
                rs=-0.5 * (q * Aq).sum(1) - 0.5 * (p * Bp).sum(1), ib=cc, ik=cc - (p * q).sum(1),
                w=fac * np.conj(v) if conj else v)


def _device(bra, ket):
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda")
    cx = lambda a: torch.view_as_real(torch.from_numpy(np.ascontiguousarray(a, dtype=complex))).contiguous().to("cuda")
    return [dev(bra["X1"]), dev(ket["Y1"]), dev(bra["X2"]), dev(ket["Y2"]), dev(bra["rs"]), dev(ket["rs"]), dev(bra["ib"]),
            dev(ket["ik"]), cx(bra["w"]), cx(ket["w"])], cx


def _call(bra, ket, D, za, zb, lam, kap, M, R):
    """sc_pair_expect on packed operands -> complex (M + 1,)"""
    from semiclassical_amd._lib import check, lib, ptr
    bufs, cx = _device(bra, ket)
    ni, nj = bra["rs"].shape[0], ket["rs"].shape[0]
    bufs += [cx(za), cx(zb), torch.from_numpy(np.ascontiguousarray(lam)).to("cuda"), cx(kap)]
    partials = torch.full((lib.sc_pair_expect_tiles(ni, nj), M + 1, 2), float("nan"), device="cuda")
    out = torch.full((M + 1, 2), float("nan"), device="cuda")
    b = [ptr(t) for t in bufs]
    check(lib.sc_pair_expect(b[0], b[1], 2 * D, b[2], b[3], 3 * D, b[4], b[5], b[6], b[7], b[8], b[9], ni, nj, b[10], b[11], b[12], b[13],
                             M, R, ptr(partials), ptr(out), None))
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    return o[:, 0] + 1j * o[:, 1]


def _pair_sum(bra, ket, D):
    """sc_pair_sum_rect + sc_reduce_slot as norm() calls them -> complex"""
    from semiclassical_amd._lib import check, lib, ptr
    bufs, _ = _device(bra, ket)
    ni, nj = bra["rs"].shape[0], ket["rs"].shape[0]
    tiles = lib.sc_pair_sum_rect_tiles(ni, nj)
    partials, slot = torch.empty((tiles, 4), device="cuda"), torch.zeros(8, device="cuda")
    b = [ptr(t) for t in bufs]
    check(lib.sc_pair_sum_rect(b[0], b[1], 2 * D, b[2], b[3], 3 * D, b[4], b[5], b[6], b[7], b[8], b[9], ni, nj, ptr(partials), None))
    check(lib.sc_reduce_slot(ptr(partials), int(tiles), None, 0, 1.0, ptr(slot), None))
    torch.cuda.synchronize()
    s = slot.cpu().numpy()
    return s[0] + 1j * s[1]


def _synthetic(ni, nj, D, M, R, seed):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    G = (Q * rng.uniform(0.5, 2.0, D)) @ Q.T
    G = 0.5 * (G + G.T)
    draw = lambda n: (rng.normal(0.3, 0.8 / np.sqrt(D), (D, n)), rng.normal(0.0, 1.0 / np.sqrt(D), (D, n)),
                      rng.normal(size=n) + 1j * rng.normal(size=n))
    qk, pk, vk = draw(nj)
    qb, pb, vb = (qk, pk, vk) if ni == nj else draw(ni)
    centre = qk.mean(axis=1)
    _, _, _, fac = overlap_constants(G)
    bra, ket = _pack(qb, pb, vb, G, True, fac, centre), _pack(qk, pk, vk, G, False, fac, centre)
    T, _, _ = EC.pair_terms(qk, pk, vk, G, bra=(qb, pb, vb))
    C = M * (1 + R)
    cn = lambda *shape: rng.normal(size=shape) + 1j * rng.normal(size=shape)
    za, zb, lam, kap = cn(C, ni), cn(C, nj), rng.normal(size=C), cn(M)
    return bra, ket, T, za, zb, lam, kap


def _check_synthetic(ni, nj, D, M, R, seed):
    bra, ket, T, za, zb, lam, kap = _synthetic(ni, nj, D, M, R, seed)
    got = _call(bra, ket, D, za, zb, lam, kap, M, R)
    z = (za[:, :, None] + zb[:, None, :]).reshape(M, 1 + R, ni, nj)
    power = np.where(np.arange(1 + R) == 0, 1, 2)[None, :, None, None]
    F = kap[:, None, None] + np.einsum('mc,mcij->mij', lam.reshape(M, 1 + R), z ** power)
    terms = np.concatenate((T[None] * F, T[None]))
    want, scale = terms.sum(axis=(1, 2)), abs(terms).sum(axis=(1, 2))
    assert got.shape == (M + 1,) and (abs(got - want) <= TOL * scale).all()
    assert np.array_equal(got, _call(bra, ket, D, za, zb, lam, kap, M, R))                      # the same bits in every call
    return bra, ket, scale[M], got[M]


@pytest.mark.parametrize("D", [1, 8, 9])
@pytest.mark.parametrize("ni,nj", [(1, 1), (63, 63), (64, 64), (65, 65), (130, 130), (1, 130), (130, 1), (63, 65), (65, 64),
                                   (64, 130)])
def test_tile_edges_through_the_c_abi(ni, nj, D):
    """K1 = 2 D = 2, 16, 18 around the K chunk of 16; full, ragged and several tiles; bras and kets of different sets"""
    bra, ket, sum_abs_t, n2 = _check_synthetic(ni, nj, D, 3, 2, 100 * ni + nj + D)
    # R = 0 with a column of zeros and kappa = 1 is the sum of sc_pair_sum_rect
    zero = lambda n: np.zeros((1, n), dtype=complex)
    one = _call(bra, ket, D, zero(ni), zero(nj), np.ones(1), np.ones(1, dtype=complex), 1, 0)
    plain = _pair_sum(bra, ket, D)
    assert abs(one[0] - plain) <= 1e-12 * sum_abs_t and abs(one[1] - plain) <= 1e-12 * sum_abs_t and one[1] == n2


@pytest.mark.parametrize("M,R", [(1, 0), (1, 1), (3, 2), (1, 15), (1, 16), (1, 17), (2, 40), (65, 0), (130, 1)])
@pytest.mark.parametrize("ni,nj,D", [(65, 130, 9), (130, 63, 8)])
def test_column_chunks_through_the_c_abi(ni, nj, D, M, R):
    """1 + R = 16, 17, 18 columns around the chunk of 16, several chunks, many operators"""
    _check_synthetic(ni, nj, D, M, R, 1000 * M + R + ni)


def test_c_abi_refusals():
    from semiclassical_amd import _lib
    from semiclassical_amd._lib import lib, ptr
    buf, part, out = torch.zeros(64, device="cuda"), torch.zeros(64, device="cuda"), torch.full((4,), 7.0, device="cuda")
    p, s, o = ptr(buf), ptr(part), ptr(out)
    args = lambda M=1, R=0, ni=2, nj=2, first=p, za=p, last=o: (first, p, 2, p, p, 3, p, p, p, p, p, p, ni, nj, za, p, p, p, M, R, s, last,
                                                               None)
    for bad in (dict(first=None), dict(za=None), dict(last=None), dict(M=0), dict(R=-1)):
        assert lib.sc_pair_expect(*args(**bad)) == -1                               # SC_ERR_BAD_ARGUMENT
    assert lib.sc_pair_expect(*args(last=None)) == -1 and b"null argument" in lib.sc_last_error()
    for bad in (dict(M=65536), dict(R=513), dict(M=65535, R=256)):
        assert lib.sc_pair_expect(*args(**bad)) == -2                               # SC_ERR_UNSUPPORTED
        assert b"M <= 65535, R <= 512" in lib.sc_last_error() and b"2^24" in lib.sc_last_error()
    with pytest.raises(_lib.EngineError, match="R <= 512"):
        _lib.check(lib.sc_pair_expect(*args(R=513)))
    assert lib.sc_pair_expect(*args(ni=0)) == 0                                     # no pairs: the sums are zero
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [0.0, 0.0, 0.0, 0.0]
    assert lib.sc_pair_expect(*args()) == 0                                         # 2 x 2 pairs of zeros: exp(0) times w = 0
    torch.cuda.synchronize()
