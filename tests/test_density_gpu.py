"""HermanKlukPropagator.reduced_density (sc_density_pair_sum) against the numpy restatement of its
closed form (tests/test_density_host.py), the norm identity, the engine's own wavefunction() and the refusals."""
import numpy as np
import pytest
import torch

from tests import cases
from tests.test_density_host import first_moment, overlap_constants, restated_density

pytestmark = pytest.mark.gpu
torch.set_default_dtype(torch.float64)

TOL = 1e-9          # x max |rho|: the project's tolerance for wavefunction() against the oracle


def _advanced(name, steps, select=None, **kwargs):
    from tests.engine_cases import engine_potential, engine_propagator
    g = cases.load(name)
    pot, prop = engine_potential(g), engine_propagator(g, select=select, **kwargs)
    for _ in range(steps):
        prop.step(pot, float(g["dt"]))
    return g, pot, prop


def _state(prop):
    """(q, p, v, Gamma_t) read back from the engine, as numpy"""
    q, p = prop.current_positions_and_momenta()
    return q.cpu().numpy().copy(), p.cpu().numpy().copy(), prop.coefficients().cpu().numpy(), prop._Gt.cpu().numpy()


def _unit(D, k):
    u = np.zeros(D)
    u[k] = 1.0
    return u


def _grid(q, G, U, ns, rng):
    """ns unsorted grid values that cover the ensemble along the first direction"""
    _, B, _, _ = overlap_constants(G)
    u = np.atleast_2d(U)[0]
    sig, uq = np.sqrt(u @ B @ u), u @ q
    return rng.uniform(uq.min() - 2.0 * sig, uq.max() + 2.0 * sig, ns)


# ------------------------------------------------------------------------------------------- 1. engine vs restated formula

_STATES = {}


def _case(name):
    if name not in _STATES:
        select = slice(0, 45) if name == "hk_as33" else None
        _, _, prop = _advanced(name, 3, select=select)
        _STATES[name] = (prop, _state(prop))
    return _STATES[name]


@pytest.mark.parametrize("shape", ["M1_ns1", "M3_ns100", "M1_ns257"])
@pytest.mark.parametrize("name", ["hk_1d", "hk_as5_chi002", "hk_as33", "hk_as60_n96"])
def test_engine_matches_restated_formula(name, shape):
    prop, (q, p, v, G) = _case(name)
    D = prop.dim
    rng = np.random.default_rng(len(name) + len(shape))
    dense = rng.uniform(0.5, 1.5, D) * rng.choice([-1.0, 1.0], D)           # not an axis, norm != 1
    if shape == "M1_ns1":
        directions, U = D - 1, _unit(D, D - 1)[None, :]                       # a mode index
        s = _grid(q, G, U, 1, rng)
    elif shape == "M3_ns100":
        idx = [0, D // 2, D - 1]
        directions, U = idx, np.stack([_unit(D, k) for k in idx])           # a list of indices
        s = _grid(q, G, U, 100, rng)
    else:
        directions, U = dense, dense[None, :]                                # a dense vector
        s = _grid(q, G, U, 257, rng)
    got = prop.reduced_density(directions, s)
    want = restated_density(q, p, v, G, U, s)
    assert got.shape == want.shape == (U.shape[0], s.shape[0]) and got.dtype == np.float64
    scale = abs(want).max()
    print(f"{name} {shape}: max |rho| {scale:.3e}, deviation {abs(got - want).max() / scale:.2e} of it")
    assert scale > 0 and abs(got - want).max() <= TOL * scale
    if shape == "M3_ns100":
        # the same directions as an (M, D) array of vectors, and each one alone
        assert np.array_equal(prop.reduced_density(U, s), got)
        assert abs(prop.reduced_density(idx[1], s)[0] - got[1]).max() <= 1e-13 * scale


@pytest.mark.parametrize("name,nt", [("hk_as60_n96", 7), ("hk_coumarin_harmonic", 3)])
def test_after_run(name, nt):
    """run() leaves the state in the layouts of its multi-step and normal-mode paths"""
    g, pot, prop = _advanced(name, 0)
    prop.run(pot, float(g["dt"]), nt)
    q, p, v, G = _state(prop)
    rng = np.random.default_rng(3)
    e, V = np.linalg.eigh(G)
    V = V[:, abs(e) > 1e-8]                 # coumarin's Gamma_t is singular (rank 45 of 51): directions projected onto its range
    U = np.stack([_unit(prop.dim, 1), rng.uniform(0.5, 1.5, prop.dim)]) @ V @ V.T
    s = _grid(q, G, U, 33, rng)
    got, want = prop.reduced_density(U, s), restated_density(q, p, v, G, U, s)
    assert abs(want).max() > 0 and abs(got - want).max() <= TOL * abs(want).max()


# ------------------------------------------------------------------------------------------- 2. tile edges through the C-ABI

def _pack(q, p, v, G, conj, fac, centre):
    """the operands norm() packs for one set of trajectories (rows = trajectories); q, p (D, n)"""
    A, B, C, _ = overlap_constants(G)
    q, p = (q - centre[:, None]).T, p.T
    Aq, Bp, Cp = q @ A.T, p @ B.T, p @ C.T
    cc = (q * Cp).sum(1)
    return dict(X1=np.hstack((q, p)), Y1=np.hstack((Aq, Bp)), X2=np.hstack((q, Cp, q)), Y2=np.hstack((p, -q, -Cp)),
                rs=-0.5 * (q * Aq).sum(1) - 0.5 * (p * Bp).sum(1), ib=cc, ik=cc - (p * q).sum(1),
                w=fac * np.conj(v) if conj else v, q=q, p=p)


def _call(bra, ket, G, U, s, centre):
    """sc_density_pair_sum on packed operands -> complex (M, ns)"""
    from semiclassical_amd._lib import check, lib, ptr
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda")
    cx = lambda a: torch.view_as_real(torch.from_numpy(np.ascontiguousarray(a, dtype=complex))).contiguous().to("cuda")
    _, B, _, _ = overlap_constants(G)
    D, M, ns = G.shape[0], U.shape[0], s.shape[0]
    ni, nj = bra["q"].shape[0], ket["q"].shape[0]
    sigma2 = np.einsum('ma,ab,mb->m', U, B, U)
    bufs = [dev(bra["X1"]), dev(ket["Y1"]), dev(bra["X2"]), dev(ket["Y2"]), dev(bra["rs"]), dev(ket["rs"]), dev(bra["ib"]),
            dev(ket["ik"]), cx(bra["w"]), cx(ket["w"]), dev(0.5 * U @ bra["q"].T), dev(U @ B @ bra["p"].T),
            dev(0.5 * U @ ket["q"].T), dev(U @ B @ ket["p"].T), dev(0.5 / sigma2), dev(s), dev(U @ centre)]
    rows = lib.sc_density_pair_sum_rows(ni, nj)
    partials = torch.full((rows, M * ns, 2), float("nan"), device="cuda")
    rho = torch.full((M, ns, 2), float("nan"), device="cuda")
    b = [ptr(t) for t in bufs]
    check(lib.sc_density_pair_sum(b[0], b[1], 2 * D, b[2], b[3], 3 * D, b[4], b[5], b[6], b[7], b[8], b[9], ni, nj,
                                  b[10], b[11], b[12], b[13], b[14], M, b[15], b[16], ns, ptr(partials), ptr(rho), None))
    torch.cuda.synchronize()
    out = rho.cpu().numpy()
    return out[..., 0] + 1j * out[..., 1]


@pytest.mark.parametrize("D", [1, 8, 9])
@pytest.mark.parametrize("ni,nj", [(1, 1), (63, 63), (64, 64), (65, 65), (130, 130), (1, 130), (130, 1), (63, 65), (65, 64),
                                   (64, 130)])
def test_tile_edges_through_the_c_abi(ni, nj, D):
    """K1 = 2 D = 2, 16, 18 around the K chunk of 16; full, ragged and several tiles; bras and kets of different sets"""
    rng = np.random.default_rng(100 * ni + nj + D)
    Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    G = (Q * rng.uniform(0.5, 2.0, D)) @ Q.T
    G = 0.5 * (G + G.T)
    draw = lambda n: (rng.normal(0.3, 0.8 / np.sqrt(D), (D, n)), rng.normal(0.0, 1.0 / np.sqrt(D), (D, n)),
                      rng.normal(size=n) + 1j * rng.normal(size=n))
    qk, pk, vk = draw(nj)
    qb, pb, vb = (qk, pk, vk) if ni == nj else draw(ni)
    U = np.stack([_unit(D, D - 1), rng.uniform(0.5, 1.5, D)])
    s = rng.uniform(-1.5, 2.0, 5)
    centre = qk.mean(axis=1)
    _, _, _, fac = overlap_constants(G)
    got = _call(_pack(qb, pb, vb, G, True, fac, centre), _pack(qk, pk, vk, G, False, fac, centre), G, U, s, centre)
    want = restated_density(qk, pk, vk, G, U, s, complex_sum=True, bra=(qb, pb, vb))
    scale = abs(want).max()
    assert scale > 0 and abs(got - want).max() <= TOL * scale
    if ni == nj:
        assert abs(got.imag).max() <= TOL * scale            # (i, j) and (j, i) are complex conjugates


# ------------------------------------------------------------------------------------------- 3. norm identity, first moment

def test_integral_is_the_squared_norm():
    """trapezoid sums on a uniform grid of spacing <= sigma / 2 over [min u.q - 8 sigma, max u.q + 8 sigma] along mode 0.  The
    restated formula alone meets both identities to 3e-15 on this state (CPU oracle, 49 points): the bound of 1e-6 leaves the
    quadrature more than a factor 1e8."""
    _, _, prop = _advanced("hk_as5_chi002", 5)
    q, p, v, G = _state(prop)
    u = _unit(prop.dim, 0)
    _, B, _, _ = overlap_constants(G)
    sig, uq = np.sqrt(u @ B @ u), u @ q
    lo, hi = uq.min() - 8.0 * sig, uq.max() + 8.0 * sig
    s = np.linspace(lo, hi, int(np.ceil((hi - lo) / (0.5 * sig))) + 1)
    assert s[1] - s[0] <= 0.5 * sig
    rho = prop.reduced_density(0, s)[0]
    trapezoid = lambda f: (s[1] - s[0]) * (f.sum() - 0.5 * (f[0] + f[-1]))
    norm2 = prop.norm() ** 2
    total, moment, want = trapezoid(rho), trapezoid(s * rho), first_moment(q, p, v, G, u)
    print(f"int rho = {total:.15g}, norm^2 = {norm2:.15g}: {abs(total - norm2) / norm2:.2e}; "
          f"int s rho = {moment:.15g}, sum = {want:.15g}: {abs(moment - want) / abs(want):.2e}")
    assert abs(total - norm2) <= 1e-6 * norm2
    assert abs(moment - want) <= 1e-6 * abs(want)


# ------------------------------------------------------------------------------------------- 4. D = 1 against wavefunction()

def test_one_dimension_is_psi_squared():
    prop, (q, p, v, G) = _case("hk_1d")
    s = np.linspace(q.min() - 1.0, q.max() + 1.0, 131)
    rho = prop.reduced_density(0, s)[0]
    psi2 = abs(prop.wavefunction(s[None, :])) ** 2
    assert abs(rho - psi2).max() <= TOL * rho.max()


# ------------------------------------------------------------------------------------------- 5. singular Gamma_t

def test_singular_width_matrix():
    _, _, prop = _advanced("hk_methylium", 3)
    q, p, v, G = _state(prop)
    e, V = np.linalg.eigh(G)
    inside, null = V[:, np.argmax(e)], V[:, np.argmin(abs(e))]
    assert np.count_nonzero(abs(e) > 1e-8) == 6 and abs(e).min() <= 1e-8
    rng = np.random.default_rng(5)
    s = _grid(q, G, inside, 40, rng)
    got, want = prop.reduced_density(inside, s), restated_density(q, p, v, G, inside, s)
    assert abs(want).max() > 0 and abs(got - want).max() <= TOL * abs(want).max()
    with pytest.raises(ValueError, match="range of Gamma_t"):
        prop.reduced_density(null, s)
    with pytest.raises(ValueError, match="range of Gamma_t"):
        prop.reduced_density(np.stack([inside, inside + 1e-6 * null]), s)


# ------------------------------------------------------------------------------------------- 6. determinism, non-interference

def test_same_bits_and_untouched_state():
    g, pot, prop = _advanced("hk_as60_n96", 3)
    _, _, twin = _advanced("hk_as60_n96", 3)
    s = np.linspace(-40.0, 40.0, 300)
    first = prop.reduced_density([0, 59], s)
    assert np.array_equal(first, prop.reduced_density([0, 59], s))
    assert prop.norm() == twin.norm()
    assert torch.equal(prop.coefficients(), twin.coefficients())
    prop.step(pot, float(g["dt"]))
    twin.step(pot, float(g["dt"]))
    assert torch.equal(prop._qp, twin._qp) and torch.equal(prop._c2, twin._c2) and torch.equal(prop._act, twin._act)
    assert torch.equal(prop.coefficients(), twin.coefficients())


# ------------------------------------------------------------------------------------------- 7. refusals

def test_refusals():
    prop, _ = _case("hk_as5_chi002")
    s = np.linspace(-1.0, 1.0, 4)
    for bad in (np.ones(4), np.ones((2, 6)), np.zeros(5), np.stack([np.ones(5), np.zeros(5)]), 5, -1, [0, 7], []):
        with pytest.raises(ValueError):
            prop.reduced_density(bad, s)
    for bad in ([], np.array([0.0, np.nan]), np.array([np.inf]), np.zeros((2, 2))):
        with pytest.raises(ValueError):
            prop.reduced_density(0, bad)


def test_wm_refuses():
    from tests.engine_cases import engine_propagator
    prop = engine_propagator(cases.load("wm_as5_chi002"))
    with pytest.raises(NotImplementedError, match="per-trajectory widths"):
        prop.reduced_density(0, np.linspace(-1.0, 1.0, 4))


def test_c_abi_refusals():
    from semiclassical_amd import _lib
    from semiclassical_amd._lib import lib, ptr
    zeros, out = torch.zeros(2 * 3 * 512, device="cuda"), torch.zeros(8, device="cuda")     # operands of 2 x 2 pairs at D = 512
    p, o = ptr(zeros), ptr(out)
    args = lambda K1, K2, first=p, last=o: (first, p, K1, p, p, K2, p, p, p, p, p, p, 2, 2, p, p, p, p, p, 1, p, p, 1, o, last, None)
    assert lib.sc_density_pair_sum(*args(2, 3, first=None)) == -1                  # SC_ERR_BAD_ARGUMENT
    assert b"null argument" in lib.sc_last_error()
    assert lib.sc_density_pair_sum(*args(2, 3, last=None)) == -1
    assert lib.sc_density_pair_sum(*args(2 * 513, 3 * 513)) == -2                  # SC_ERR_UNSUPPORTED
    assert b"D <= 512" in lib.sc_last_error()
    with pytest.raises(_lib.EngineError, match="K1 <= 1024"):
        _lib.check(lib.sc_density_pair_sum(*args(2 * 513, 3 * 513)))
    assert lib.sc_density_pair_sum(*args(2 * 512, 3 * 512)) == 0                   # D = 512 is held
    torch.cuda.synchronize()
