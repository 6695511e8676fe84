"""HermanKlukPropagator.expectation(ex=...) / anharmonic_energy_expectation (sc_pair_expect_exp) against the
numpy restatement of tests/expect_exp_cases.py on the oracle's state, the untouched state and the unchanged ex=None route, the
refusals, and the tile and chunk edges of the product columns through the C-ABI."""
import numpy as np
import pytest
import torch

from tests import cases, expect_cases as EC, expect_exp_cases as XC
from tests.test_expect_gpu import MEANINGFUL, TOL, _advanced, _call, _case as _plain_case, _device, _normalised_bound, _synthetic

pytestmark = pytest.mark.gpu
torch.set_default_dtype(torch.float64)

GOLDENS = ["hk_1d", "hk_as5_chi002", "hk_as33", "hk_as60_n96"]
# seed 6 of expect_exp_cases.standard_operators: with the oracle alone the smallest |E_a| / At_a of the five operators is 0.330
# (hk_1d), 1.98e-2 (hk_as5_chi002), 2.14e-2 (hk_as33), 2.07e-2 (hk_as60_n96) -- V in the three AS models; H 3.8e-2 ... 4.1e-2 there,
# the mixed operator 0.10 at least: every one above the floor of 5e-3, no other seed was needed
SEED = 6

_STATES = {}


def _case(name):
    """(golden, potential, propagator, oracle state, operators, restatement) after 3 steps, computed once -- the propagator and the
    oracle's state are those of tests/test_expect_gpu.py, which nothing here changes"""
    if name not in _STATES:
        from tests.engine_cases import engine_potential
        g = cases.load(name)
        pot, (prop, state) = engine_potential(g), _plain_case(name)
        q, p, v, G = state
        ops = XC.standard_operators(np.random.default_rng(SEED), G, g)
        _STATES[name] = (g, pot, prop, state, ops, XC.restated_expectation(q, p, v, G, **ops))
    return _STATES[name]


def _engine(prop, ops, **kwargs):
    return prop.expectation(ops["c"], ops["m"], ops["K"], ops["n"], ops["W"], ex=(ops["w"], ops["a"]), **kwargs)


# ------------------------------------------------------------------------------------------- 1. engine vs restatement

@pytest.mark.parametrize("name", GOLDENS)
def test_engine_matches_restatement(name):
    _, _, prop, _, ops, (E, At, N2) = _case(name)
    got, norm2 = _engine(prop, ops, normalise=False)
    assert got.shape == (5,) and got.dtype == np.complex128 and isinstance(norm2, float)
    for a, label in enumerate(XC.LABELS):
        print(f"{name} {label:9s}: |E| / At = {abs(got[a]) / At[a]:.3e}, |E - restatement| / At = {abs(got[a] - E[a]) / At[a]:.2e}, "
              f"|Im E| / At = {abs(got[a].imag) / At[a]:.2e}")
    assert (abs(got) >= MEANINGFUL * At).all()
    assert (TOL * At <= 1e-6 * abs(got)).all()              # what the floor implies: the bound cannot hide a wrong factor
    assert (abs(got - E) <= TOL * At).all()
    assert (abs(got.imag) <= TOL * At).all()                # Hermitian operators, a Gamma_t of full rank
    assert abs(norm2 - N2.real) <= TOL * At[4] and got[4].real == norm2
    vals, again = _engine(prop, ops)
    assert again == norm2 and (abs(vals - got / norm2) <= 1e-15 * abs(vals)).all()
    # the exponential parts alone, without any of the five others: M from ex
    few, _ = prop.expectation(ex=(ops["w"][:1], ops["a"][:1]), normalise=False)
    assert few.shape == (1,) and abs(few[0] - got[0]) <= 1e-13 * At[0]


@pytest.mark.parametrize("name", GOLDENS)
def test_anharmonic_energy_expectation(name):
    _, pot, prop, (q, p, v, G), _, (E, At, N2) = _case(name)
    AN = abs(EC.pair_terms(q, p, v, G)[0]).sum()
    got = prop.anharmonic_energy_expectation(pot)
    want, bound = (E[2] / N2).real, _normalised_bound(E, At, N2, AN)[2]
    print(f"{name}: <H> = {got:.15g}, restatement {want:.15g}, deviation {abs(got - want):.2e}, bound {bound:.2e}, "
          f"|E| / At = {abs(E[2]) / At[2]:.3e}")
    assert isinstance(got, float) and abs(E[2]) >= MEANINGFUL * At[2]
    assert abs(got - want) <= bound


def test_constant_hessian_gives_energy_expectation():
    _, pot, prop, _ = _advanced("hk_as5_chi000", 3, oracle=False)
    assert prop.anharmonic_energy_expectation(pot) == prop.energy_expectation(pot)


# ------------------------------------------------------------------------------------------- 2. nothing else changes

def test_plain_route_keeps_its_bits():
    """ex=None through expectation() before and after a call with ex"""
    _, pot, prop, (_, _, _, G), ops, _ = _case("hk_as5_chi002")
    c, m, K, n, W = EC.standard_operators(np.random.default_rng(6), G)
    before = prop.expectation(c, m, K, n, W, normalise=False)
    first = _engine(prop, ops, normalise=False)
    prop.anharmonic_energy_expectation(pot)
    second = _engine(prop, ops, normalise=False)
    after = prop.expectation(c, m, K, n, W, normalise=False, ex=None)
    assert np.array_equal(before[0], after[0]) and before[1] == after[1]
    assert np.array_equal(first[0], second[0]) and first[1] == second[1]        # the same bits in every call


def test_state_is_untouched():
    from tests.engine_cases import engine_potential, engine_propagator
    g = cases.load("hk_as5_chi002")
    pot, dt, E0 = engine_potential(g), float(g["dt"]), float(g["E0"])
    prop, twin = engine_propagator(g), engine_propagator(g)
    ops = XC.standard_operators(np.random.default_rng(SEED), g["Gamma_t"], g)
    outs = []
    for pr, calls in ((prop, True), (twin, False)):
        pr.step(pot, dt)
        if calls:
            _engine(pr, ops)
            pr.anharmonic_energy_expectation(pot)
        assert pr.t == dt
        outs.append(pr.run(pot, dt, 2, E0))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    for name in ("_qp", "_act", "_c2", "_sgn"):
        assert torch.equal(getattr(prop, name), getattr(twin, name)), name
    for a, b in zip(prop.monodromy_matrices(), twin.monodromy_matrices()):
        assert torch.equal(a, b)
    assert torch.equal(prop.coefficients(), twin.coefficients())


# ------------------------------------------------------------------------------------------- 3. refusals

def test_refusals():
    from semiclassical_amd import potentials as P
    from tests.engine_cases import engine_potential
    _, pot, prop, _, ops, _ = _case("hk_as5_chi002")
    D = prop.dim
    w, a = ops["w"], ops["a"]
    for ex in ((w,), (w, a, a), w, (w[0], a[0]), (w, a[:, :, :-1]), (w[:, :3], a), (np.zeros((0, 1)), np.zeros((0, 1, D)))):
        with pytest.raises(ValueError, match="operators: ex"):
            prop.expectation(ex=ex)
    with pytest.raises(ValueError, match="same number M"):
        prop.expectation(c=np.ones(2), ex=(w, a))
    bad = w.copy()
    bad[1, 0] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        prop.expectation(ex=(bad, a))
    far = np.zeros((2, 2, D))
    far[1, 1, 0] = 1.0e6
    with pytest.raises(ValueError, match="term 1 of operator 1 of ex.*not finite"):
        prop.expectation(ex=(np.ones((2, 2)), far))
    # a trajectory far out on the repulsive wall: the weights are finite, exp(-a.q / 2) at its position is not
    from semiclassical_amd import propagators as PR
    one = torch.eye(1)
    lone = PR.HermanKlukPropagator(one, one, device="cuda")
    lone.set_initial_conditions(torch.zeros(1), torch.zeros(1), one, torch.tensor([[0.1, -2000.0], [0.0, 0.0]]), torch.ones(2))
    assert np.isfinite(lone.expectation(ex=(np.ones((1, 2)), np.full((1, 2, 1), 0.1)))[0]).all()
    with pytest.raises(ValueError, match="term 1 of operator 0 of ex.*not finite.*repulsive wall"):
        lone.expectation(ex=(np.ones((1, 2)), np.array([[[0.1], [1.0]]])))
    with pytest.raises(ValueError, match="dimensions"):
        prop.anharmonic_energy_expectation(P.MorsePotential(torch.ones(D + 1), torch.full((D + 1,), 0.02), torch.zeros(D + 1)))
    # sGDML and quartic force fields
    one = np.ones(1)
    qff = P.QuarticForceFieldPotential.from_arrays(0.0 * one, 0.0, 0.0 * one, np.eye(1), cubic=-0.75 * np.ones((1, 1, 1)),
                                                   quartic_iijj=0.4375 * np.eye(1), masses=one, nac0=0.0 * one)
    for other in (qff, engine_potential(cases.load("hk_coumarin_gdml"))):
        with pytest.raises(NotImplementedError, match="no closed form"):
            prop.anharmonic_energy_expectation(other)


def test_singular_width_matrix_refusals():
    prop, (_, _, _, G) = _plain_case("hk_methylium")
    D = G.shape[0]
    e, V = np.linalg.eigh(G)
    inside, null = V[:, np.argmax(e)], V[:, np.argmin(abs(e))]
    scale = 1.0 / np.sqrt(np.trace(np.linalg.pinv(2.0 * G)))
    vals, _ = prop.expectation(ex=(np.ones((1, 1)), scale * inside[None, None]))
    assert np.isfinite(vals).all()
    with pytest.raises(ValueError, match="term 0 of operator 1 of ex .* range of Gamma_t"):
        prop.expectation(ex=(np.ones((2, 1)), scale * np.stack([inside, inside + 1e-6 * null])[:, None, :]))
    from semiclassical_amd import potentials as P
    with pytest.raises(ValueError, match="singular"):
        prop.anharmonic_energy_expectation(P.MorsePotential(torch.ones(D), torch.full((D,), 0.02), torch.zeros(D)))


def test_wm_and_thermal_ensembles_refuse():
    from tests.engine_cases import engine_potential, engine_propagator
    from tests.test_thermal_gpu import _golden_case
    g = cases.load("wm_as5_chi002")
    wm, D = engine_propagator(g), g["Gamma_t"].shape[0]
    ex = (np.ones((1, 1)), np.ones((1, 1, D)))
    for call in (lambda: wm.expectation(ex=ex), lambda: wm.expectation(c=np.ones(1), ex=ex),
                 lambda: wm.anharmonic_energy_expectation(engine_potential(g))):
        with pytest.raises(NotImplementedError, match="per-trajectory widths"):
            call()
    _, pot, _, prop, _, _, _ = _golden_case("hk_as5_chi002", 0.006, n=67)
    for call in (lambda: prop.expectation(ex=ex), lambda: prop.anharmonic_energy_expectation(pot)):
        with pytest.raises(NotImplementedError, match="thermal ensemble"):
            call()


# ------------------------------------------------------------------------------------------- 4. tile and chunk edges through the C-ABI

def _call_exp(bra, ket, D, za, zb, lam, kap, M, R, ea, eb, P):
    """sc_pair_expect_exp on packed operands -> complex (M + 1,)"""
    from semiclassical_amd._lib import check, lib, ptr
    bufs, cx = _device(bra, ket)
    ni, nj = bra["rs"].shape[0], ket["rs"].shape[0]
    bufs += [cx(za), cx(zb), torch.from_numpy(np.ascontiguousarray(lam)).to("cuda"), cx(kap)]
    bufs += [cx(ea), cx(eb)] if P else [None, None]
    partials = torch.full((lib.sc_pair_expect_tiles(ni, nj), M + 1, 2), float("nan"), device="cuda")
    out = torch.full((M + 1, 2), float("nan"), device="cuda")
    b = [ptr(t) for t in bufs]
    check(lib.sc_pair_expect_exp(b[0], b[1], 2 * D, b[2], b[3], 3 * D, b[4], b[5], b[6], b[7], b[8], b[9], ni, nj, b[10], b[11], b[12],
                                 b[13], M, R, b[14], b[15], P, ptr(partials), ptr(out), None))
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    return o[:, 0] + 1j * o[:, 1]


def _check_synthetic(ni, nj, D, M, R, P, seed):
    bra, ket, T, za, zb, lam, kap = _synthetic(ni, nj, D, M, R, seed)
    rng = np.random.default_rng(seed + 7)
    cn = lambda *shape: rng.normal(size=shape) + 1j * rng.normal(size=shape)
    ea, eb = cn(M * P, ni), cn(M * P, nj)                   # (P = 0: null pointers)
    got = _call_exp(bra, ket, D, za, zb, lam, kap, M, R, ea, eb, P)
    z = (za[:, :, None] + zb[:, None, :]).reshape(M, 1 + R, ni, nj)
    power = np.where(np.arange(1 + R) == 0, 1, 2)[None, :, None, None]
    sums = lam.reshape(M, 1 + R)[:, :, None, None] * z ** power
    prods = (ea[:, :, None] * eb[:, None, :]).reshape(M, P, ni, nj)
    F = kap[:, None, None] + sums.sum(axis=1) + prods.sum(axis=1)
    size = abs(kap)[:, None, None] + abs(sums).sum(axis=1) + abs(prods).sum(axis=1)             # sum of |terms|
    want = np.concatenate(((T[None] * F).sum(axis=(1, 2)), [T.sum()]))
    scale = np.concatenate(((abs(T)[None] * size).sum(axis=(1, 2)), [abs(T).sum()]))
    print(f"ni, nj, D, M, R, P = {ni}, {nj}, {D}, {M}, {R}, {P}: largest deviation {np.max(abs(got - want) / scale):.2e} of sum |terms|")
    assert got.shape == (M + 1,) and (abs(got - want) <= TOL * scale).all()
    assert np.array_equal(got, _call_exp(bra, ket, D, za, zb, lam, kap, M, R, ea, eb, P))       # the same bits in every call
    return bra, ket, za, zb, lam, kap, got, scale


@pytest.mark.parametrize("D", [1, 8, 9])
@pytest.mark.parametrize("ni,nj", [(1, 1), (63, 63), (64, 64), (65, 65), (130, 130), (1, 130), (130, 1), (63, 65), (65, 64),
                                   (64, 130)])
def test_tile_edges_through_the_c_abi(ni, nj, D):
    """K1 = 2 D = 2, 16, 18 around the K chunk of 16; full, ragged and several tiles; bras and kets of different sets; and P = 0
    against sc_pair_expect on the same operands"""
    _check_synthetic(ni, nj, D, 3, 2, 2, 100 * ni + nj + D)
    bra, ket, za, zb, lam, kap, zero, scale = _check_synthetic(ni, nj, D, 3, 2, 0, 100 * ni + nj + D)
    plain = _call(bra, ket, D, za, zb, lam, kap, 3, 2)
    print(f"P = 0 against sc_pair_expect: {np.max(abs(zero - plain) / scale):.2e} of sum |terms|")
    assert (abs(zero - plain) <= 1e-12 * scale).all()


@pytest.mark.parametrize("M,R,P", [(1, 0, 1), (1, 0, 15), (1, 0, 16), (1, 0, 17), (1, 0, 40), (3, 2, 2), (1, 17, 17), (65, 0, 1),
                                   (2, 1, 0)])
@pytest.mark.parametrize("ni,nj,D", [(65, 130, 9), (130, 63, 8)])
def test_column_chunks_through_the_c_abi(ni, nj, D, M, R, P):
    """P = 15, 16, 17 product columns around the chunk of 16, several chunks, both kinds of columns past one chunk, many operators,
    none"""
    _check_synthetic(ni, nj, D, M, R, P, 1000 * M + 10 * R + P + ni)


def test_c_abi_refusals():
    from semiclassical_amd import _lib
    from semiclassical_amd._lib import lib, ptr
    buf, part, out = torch.zeros(64, device="cuda"), torch.zeros(64, device="cuda"), torch.full((4,), 7.0, device="cuda")
    p, s, o = ptr(buf), ptr(part), ptr(out)

    def args(M=1, R=0, P=1, ni=2, nj=2, first=p, za=p, ea=p, eb=p, last=o):
        return (first, p, 2, p, p, 3, p, p, p, p, p, p, ni, nj, za, p, p, p, M, R, ea, eb, P, s, last, None)
    for bad in (dict(first=None), dict(za=None), dict(last=None), dict(M=0), dict(R=-1), dict(P=-1), dict(ea=None), dict(eb=None)):
        assert lib.sc_pair_expect_exp(*args(**bad)) == -1                           # SC_ERR_BAD_ARGUMENT
    assert lib.sc_pair_expect_exp(*args(eb=None, P=3)) == -1 and b"P=3" in lib.sc_last_error()
    for bad in (dict(M=65536), dict(R=513), dict(M=65535, R=256), dict(P=1025), dict(M=16384, P=1024)):
        assert lib.sc_pair_expect_exp(*args(**bad)) == -2                           # SC_ERR_UNSUPPORTED
        assert b"R <= 512" in lib.sc_last_error() and b"P <= 1024" in lib.sc_last_error() and b"M P < 2^24" in lib.sc_last_error()
    with pytest.raises(_lib.EngineError, match="P <= 1024"):
        _lib.check(lib.sc_pair_expect_exp(*args(P=1025)))
    assert lib.sc_pair_expect_exp(*args(ni=0)) == 0                                 # no pairs: the sums are zero
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [0.0, 0.0, 0.0, 0.0]
    out.fill_(7.0)
    assert lib.sc_pair_expect_exp(*args(P=0, ea=None, eb=None)) == 0                # P = 0 allows null ea, eb; 2 x 2 pairs of w = 0
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [0.0, 0.0, 0.0, 0.0]
    assert lib.sc_pair_expect_exp(*args()) == 0
    torch.cuda.synchronize()
