"""WaltonManolopoulosPropagator.wm_operator_expectation / wm_phase_space_moments / wm_energy_expectation (sc_wm_pair_expect_cols,
DESIGN.md section 4.25) against the numpy restatement of tests/wm_energy_cases.py on the engine's own export and on the oracle's
state, against norm() and wm_expectation, the untouched state, and the C-ABI on synthetic operands: column kinds, per-ket slots on
any column, tile and lane edges, pivoting, limits."""
import numpy as np
import pytest
import torch

from tests import cases, wm_energy_cases as EC, wm_expect_cases as WC

pytestmark = pytest.mark.gpu
torch.set_default_dtype(torch.float64)

TOL = 1e-9          # x A_a, the sum of the absolute terms: the bound of sections 4.24 and 4.23
ORACLE_TOL = 1e-8   # against the oracle's state: the bound of the WM norm tests
MEANINGFUL = 5e-3   # |E_a| / A_a at least, for operators of one sign: the bound cannot hide a wrong factor behind cancellation
LABELS = ("p^2", "rank-2 pp", "exp(-a.x)", "all parts")


def _advanced(name, steps, ntraj=48, oracle=False, harmonic=False):
    from tests.engine_cases import engine_potential, engine_propagator
    g = cases.load(name)
    g["zi"], g["probi"] = g["zi"][:, :ntraj], g["probi"][:ntraj]
    if harmonic:
        g["chi"] = 0.0 * g["chi"]
    pot, prop = engine_potential(g), engine_propagator(g)
    for _ in range(steps):
        prop.step(pot, float(g["dt"]))
    ref = None
    if oracle:
        ref, opot = cases.oracle_propagator(g), cases.oracle_potential(g)
        for _ in range(steps):
            ref.step(opot, float(g["dt"]))
    return g, pot, prop, ref


def _rate_vector(pot, U):
    """a = rate_k e_k of the first mode of a Morse-type potential; a unit vector of the range of U for every other"""
    D = U.shape[0]
    from semiclassical_amd import potentials as P
    if isinstance(pot, P.MorsePotential):
        return float(pot.a[0]) * np.eye(D)[0]
    if isinstance(pot, P.NonHarmonicPotential):
        return float(pot.b[0]) * np.eye(D)[0]
    return U[:, 0].copy()


def _operators(rng, U, pot):
    """p^2 along one random unit vector of the range of U, a rank-2 pp (rank 1 at d' = 1) of positive eigenvalues, exp(-a.x) along a
    mode with that mode's Morse rate, and everything at once"""
    D, dp = U.shape
    u = WC.random_direction(rng, U)
    V = U @ np.linalg.qr(rng.standard_normal((dp, dp)))[0][:, :min(2, dp)]
    a = _rate_vector(pot, U)
    c, m, K, n, W = np.zeros(4), np.zeros((4, D)), np.zeros((4, D, D)), np.zeros((4, D)), np.zeros((4, D, D))
    w, av = np.zeros((4, 2)), np.zeros((4, 2, D))
    W[0] = 2.0 * np.outer(u, u)
    W[1] = (V * np.array([1.5, 0.6])[:V.shape[1]]) @ V.T
    w[2, 0], av[2, 0] = 1.0, a
    c[3], m[3], n[3], K[3], W[3] = 0.7, u, -0.4 * u, -1.1 * np.outer(u, u), W[1] - 0.3 * W[0]
    w[3], av[3] = (-2.0, 1.0), (a, 2.0 * a)
    return dict(c=c, m=m, K=K, n=n, W=W, ex=(w, av))


def _check_engine(label, prop, state, ops, tol):
    E, A, N2 = EC.restated_expectation(state, state, **ops)
    got, norm2 = prop.wm_operator_expectation(ops["c"], ops["m"], ops["K"], ops["n"], ops["W"], ops["ex"], normalise=False)
    assert got.shape == (4,) and got.dtype == np.complex128 and isinstance(norm2, float)
    for a, name in enumerate(LABELS):
        print(f"{label} {name:10s}: |E| / A = {abs(got[a]) / A[a]:.3e}, |E - restatement| / A = {abs(got[a] - E[a]) / A[a]:.2e}")
    assert (abs(got[:3]) >= MEANINGFUL * A[:3]).all()
    assert (abs(got - E) <= tol * A).all()
    AN = abs(WC.pair_system(state, state)[0]).sum()
    assert abs(norm2 - N2.real) <= tol * AN
    return got, norm2, A


# ------------------------------------------------------------------------------------------- 1. engine vs restatement

@pytest.mark.parametrize("name", ["wm_1d", "wm_as5_chi002", "wm_methylium", "wm_as24"])
def test_engine_matches_restatement_on_its_own_export(name):
    _, pot, prop, _ = _advanced(name, 3)
    state = WC.engine_state(prop)
    ops = _operators(np.random.default_rng(1), state["U"], pot)
    got, norm2, A = _check_engine(name, prop, state, ops, TOL)
    assert abs(norm2 - prop.norm() ** 2) <= 1e-9 * norm2
    vals, again = prop.wm_operator_expectation(ops["c"], ops["m"], ops["K"], ops["n"], ops["W"], ops["ex"])
    assert again == norm2 and (abs(vals - got / norm2) <= 1e-15 * abs(vals)).all()
    # the momentum part alone and the exponential part alone: M from pp, from ex
    few, _ = prop.wm_operator_expectation(pp=ops["W"][:1], normalise=False)
    assert few.shape == (1,) and abs(few[0] - got[0]) <= 1e-13 * A[0]
    few, _ = prop.wm_operator_expectation(ex=(ops["ex"][0][2:3], ops["ex"][1][2:3]), normalise=False)
    assert few.shape == (1,) and abs(few[0] - got[2]) <= 1e-13 * A[2]


def test_engine_matches_restatement_on_the_oracle_state():
    _, pot, prop, ref = _advanced("wm_as5_chi002", 3, oracle=True)
    state = WC.oracle_state(ref)
    _check_engine("oracle state", prop, state, _operators(np.random.default_rng(1), state["U"], pot), ORACLE_TOL)


# ------------------------------------------------------------------------------------------- 2. the route without pp and ex

def test_plain_route_returns_the_bits_of_wm_expectation():
    _, _, prop, _ = _advanced("wm_as5_chi002", 2, ntraj=40)
    c, m, K, n = WC.standard_operators(np.random.default_rng(5), prop._wm_bufs["U"].cpu().numpy())
    for normalise in (True, False):
        want = prop.wm_expectation(c, m, K, n, normalise=normalise)
        got = prop.wm_operator_expectation(c, m, K, n, normalise=normalise)
        assert np.array_equal(got[0], want[0]) and got[1] == want[1]
        got = prop.wm_operator_expectation(c=c, x=m, xx=K, p=n, pp=None, ex=None, normalise=normalise)
        assert np.array_equal(got[0], want[0]) and got[1] == want[1]


# ------------------------------------------------------------------------------------------- 3. <H>

def _normalised_bound(E, A, N2, AN):
    """of E_a / N2 when E_a is off by TOL A_a and N2 by TOL sum |T|"""
    return TOL * (A + abs(E) * AN / abs(N2)) / abs(N2)


@pytest.mark.parametrize("name,harmonic", [("wm_1d", False), ("wm_as5_chi002", False), ("wm_as24", False), ("wm_as5_chi002", True)])
def test_energy_expectation(name, harmonic):
    """NonHarmonicPotential; MorsePotential with chi != 0 at D = 5 and at D = 24 -- 1 + 24 + 48 = 73 columns, one call under the
    capacity of 76 --; MorsePotential with chi = 0 on the frequencies of wm_as5_chi002: the constant-Hessian branch"""
    from semiclassical_amd import hostmath
    from semiclassical_amd._lib import lib
    g, pot, prop, _ = _advanced(name, 3, harmonic=harmonic)
    state = WC.engine_state(prop)
    D = prop.dim
    num = lambda t: hostmath.as_f64(t).numpy()
    if harmonic:
        assert pot._is_harmonic()
        c, K, W, ex = np.zeros(1), np.diag(num(pot.omega) ** 2)[None], np.eye(D)[None], None
    elif name == "wm_1d":
        eps, b = num(pot.eps), num(pot.b)
        c, K, W, ex = EC.morse_operator(0.5 * eps / b ** 2, b, harmonic=1.0 - eps)
    else:
        c, K, W, ex = EC.morse_operator(num(pot.D), num(pot.a))
        cols = hostmath.fold_wm_operator_columns(c, None, K, None, W, ex, state["U"])[5]
        assert cols == 1 + 3 * D and cols <= lib.sc_wm_pair_expect_capacity(D, D)
        assert name != "wm_as24" or (cols, lib.sc_wm_pair_expect_capacity(D, D)) == (73, 76)
    E, A, N2 = EC.restated_expectation(state, state, c=c, K=K, W=W, ex=ex)
    AN = abs(WC.pair_system(state, state)[0]).sum()
    want, bound = (E[0] / N2).real, _normalised_bound(E, A, N2, AN)[0]
    got = prop.wm_energy_expectation(pot)
    print(f"{name}{' chi = 0' if harmonic else ''}: <H> = {got:.15g}, restatement {want:.15g}, deviation {abs(got - want):.2e}, "
          f"bound {bound:.2e}, |E| / A = {abs(E[0]) / A[0]:.3e}")
    assert isinstance(got, float) and abs(got - want) <= bound


def test_energy_expectation_refusals():
    from semiclassical_amd import potentials as P
    from tests.engine_cases import engine_potential
    _, pot, prop, _ = _advanced("wm_methylium", 0, ntraj=8)
    with pytest.raises(ValueError, match="singular"):
        prop.wm_energy_expectation(pot)
    one = np.ones(1)
    qff = P.QuarticForceFieldPotential.from_arrays(0.0 * one, 0.0, 0.0 * one, np.eye(1), cubic=-0.75 * np.ones((1, 1, 1)),
                                                   quartic_iijj=0.4375 * np.eye(1), masses=one, nac0=0.0 * one)
    for other in (qff, engine_potential(cases.load("hk_coumarin_gdml"))):
        with pytest.raises(NotImplementedError, match="no closed form"):
            prop.wm_energy_expectation(other)
    _, morse, five, _ = _advanced("wm_as5_chi002", 0, ntraj=8)
    with pytest.raises(ValueError, match="dimensions"):
        five.wm_energy_expectation(P.MorsePotential(torch.ones(6), torch.full((6,), 0.02), torch.zeros(6)))
    U = prop._wm_bufs["U"].cpu().numpy()
    null = np.linalg.svd(U.T)[2][-1]
    with pytest.raises(ValueError, match="pp of operator 0 .* outside the range"):
        prop.wm_operator_expectation(pp=np.eye(prop.dim)[None])
    with pytest.raises(ValueError, match="a of ex of operator 0 .* outside the range"):
        prop.wm_operator_expectation(ex=(np.ones((1, 1)), null[None, None]))
    with pytest.raises(ValueError, match="operator 0 is not finite"):
        five.wm_operator_expectation(ex=(np.ones((1, 1)), np.full((1, 1, 5), 1.0e4)))
    with pytest.raises(ValueError, match="give directions"):
        prop.wm_phase_space_moments()
    for call in (lambda: prop.expectation(c=np.ones(1)), lambda: five.anharmonic_energy_expectation(morse), lambda: prop.wavepacket_moments(0)):
        with pytest.raises(NotImplementedError, match="per-trajectory widths"):
            call()


# ------------------------------------------------------------------------------------------- 4. moments

def test_phase_space_moments():
    _, _, prop, _ = _advanced("wm_as5_chi002", 3)
    state = WC.engine_state(prop)
    D = prop.dim
    dense = np.random.default_rng(21).uniform(0.5, 1.5, D)
    AN = abs(WC.pair_system(state, state)[0]).sum()
    for directions, U in ((None, np.eye(D)), ([0, D - 1], np.eye(D)[[0, D - 1]]), (dense, dense[None, :])):
        Md = U.shape[0]
        sq, zv, zm = np.stack([2.0 * np.outer(u, u) for u in U]), np.zeros((Md, D)), np.zeros((Md, D, D))
        E, A, N2 = EC.restated_expectation(state, state, n=np.concatenate((zv, U)), W=np.concatenate((sq, zm)))
        tol = _normalised_bound(E, A, N2, AN)
        want = (E / N2).real
        (pp, pm), (tpp, tp) = (want[:Md], want[Md:]), (tol[:Md], tol[Md:])
        got = prop.wm_phase_space_moments() if directions is None else prop.wm_phase_space_moments(directions)
        old = prop.wm_wavepacket_moments() if directions is None else prop.wm_wavepacket_moments(directions)
        assert sorted(got) == ["norm2", "p", "var_p", "var_x", "x"] and abs(got["norm2"] - N2.real) <= TOL * AN
        assert got["var_p"].shape == (Md,) and (got["var_p"] > 0).all()
        err = abs(got["var_p"] - (pp - pm ** 2))
        print(f"directions {directions if directions is None else Md}: var_p {got['var_p']}, largest deviation / bound "
              f"{(err / (tpp + 2.0 * abs(pm) * tp)).max():.2e}")
        assert (err <= tpp + 2.0 * abs(pm) * tp).all()
        # x, p and var_x are wm_wavepacket_moments' values: the same columns in another call, within the bound of a normalised value
        Ex, Ax, _ = EC.restated_expectation(state, state, m=np.concatenate((U, zv, zv)), K=np.concatenate((zm, sq, zm)),
                                            n=np.concatenate((zv, zv, U)))
        tx, txx, tpl = (_normalised_bound(Ex, Ax, N2, AN)[k * Md:(k + 1) * Md] for k in range(3))
        assert (abs(got["x"] - old["x"]) <= 2 * tx).all() and (abs(got["p"] - old["p"]) <= 2 * tpl).all()
        assert (abs(got["var_x"] - old["var_x"]) <= 2 * (txx + 2.0 * abs(old["x"]) * tx)).all()
        assert abs(got["norm2"] - old["norm2"]) <= 2 * TOL * AN


# ------------------------------------------------------------------------------------------- 5. the state is not touched

def test_state_is_untouched():
    from tests.engine_cases import engine_potential, engine_propagator
    g = cases.load("wm_as5_chi002")
    g["zi"], g["probi"] = g["zi"][:, :40], g["probi"][:40]
    pot, dt, E0 = engine_potential(g), float(g["dt"]), float(g["E0"])
    prop, twin = engine_propagator(g), engine_propagator(g)
    ops = _operators(np.random.default_rng(5), g["U"].real, pot)
    args = (ops["c"], ops["m"], ops["K"], ops["n"], ops["W"], ops["ex"])
    outs = []
    for pr, calls in ((prop, True), (twin, False)):
        pr.step(pot, dt)
        rows = []
        for _ in range(2):
            if calls:
                first, second = pr.wm_operator_expectation(*args), pr.wm_operator_expectation(*args)
                assert np.array_equal(first[0], second[0]) and first[1] == second[1]            # the same bits in every call
                pr.wm_phase_space_moments([0, 1])
                assert pr.wm_energy_expectation(pot) == pr.wm_energy_expectation(pot)
            t = pr.t
            pr.step(pot, dt)
            assert pr.t == t + dt
            rows.append((pr.autocorrelation(E0), pr.ic_correlation(pot, E0)))
        outs.append(rows)
    assert outs[0] == outs[1]
    for name in ("_qp", "_act", "_c2", "_sgn", "_detA", "_detM", "_sgnA", "_sgnM"):
        assert torch.equal(getattr(prop, name), getattr(twin, name)), name
    for a, b in zip(prop.monodromy_matrices(), twin.monodromy_matrices()):
        assert torch.equal(a, b)
    assert torch.equal(prop.coefficients(), twin.coefficients())


# ------------------------------------------------------------------------------------------- 6. the C-ABI on synthetic operands

def _synthetic(rng, n, D, dp, width=1.0, spread=0.3):
    """per-trajectory inputs of the WM pair sums: complex symmetric C_QQ with a positive definite real part (the recipe of
    tests/test_wm_expect_gpu.py)"""
    U, _ = np.linalg.qr(rng.standard_normal((D, dp)))
    Q = rng.normal(0.0, spread, (n, D))
    coef = rng.normal(size=n) + 1j * rng.normal(size=n)
    cqq = np.empty((n, D, D), dtype=complex)
    for t in range(n):
        A = rng.standard_normal((D, D)) / np.sqrt(D)
        B = rng.standard_normal((D, D)) / np.sqrt(D)
        cqq[t] = width * (np.eye(D) + 0.2 * (A @ A.T) + 0.3j * (B + B.T))
    dvec = 0.1 * width * (rng.normal(size=(n, D)) + 1j * rng.normal(size=(n, D)))
    return dict(Q=Q, coef=coef, cqq=cqq, dvec=dvec, U=U)


def _pair(rng, ni, nj, D, dp, **kwargs):
    ket = _synthetic(rng, nj, D, dp, **kwargs)
    if ni == nj:
        return ket, ket
    bra = _synthetic(rng, ni, D, dp, **kwargs)
    bra["U"] = ket["U"]
    return bra, ket


def _device(bra, ket):
    """(bra tensors, ket tensors, U) as the entries take them"""
    re = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda")
    cx = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=complex)).to("cuda")
    U = ket["U"]
    qp = lambda s: re(np.hstack((s["Q"], np.zeros_like(s["Q"]))))
    cqqp = lambda s: cx(s["cqqp"] if "cqqp" in s else WC.projected(U, s["cqq"]))
    return ((qp(bra), cx(bra["coef"]), cqqp(bra), cx(bra["dvec"] @ U)),
            (qp(ket), cx(ket["coef"]), cx(ket["cqq"]), cx(ket["dvec"]), cqqp(ket), cx(ket["dvec"] @ U)), re(U), cx)


def _random_columns(rng, ni, nj, dp, kind, ketcol):
    """kind, ketcol (M, cols); kind-2 columns get small forms, so that the exponentials stay of order one"""
    kind, ketcol = np.asarray(kind, dtype=np.int32), np.asarray(ketcol, dtype=np.int32)
    M, cols = kind.shape
    C, S = M * cols, int(ketcol.max()) + 1
    cn = lambda *shape: rng.normal(size=shape) + 1j * rng.normal(size=shape)
    size = np.where(kind.reshape(-1) == 2, 0.3, 1.0)
    col = dict(za=cn(C, ni) * size[:, None], zb=cn(C, nj) * size[:, None], g=cn(C, dp) * size[:, None], sfix=cn(C, dp) * size[:, None],
               sket=cn(S, nj, dp) if S else None, lam=rng.normal(size=(M, cols)), kap=cn(M), kind=kind.reshape(-1), ketcol=ketcol.reshape(-1))
    for p in range(S):
        col["sket"][p] *= size[np.nonzero(col["ketcol"] == p)[0][0]]
    return col


def _call(dev, col, ni, nj, D, dp, **over):
    """sc_wm_pair_expect_cols itself -> (rc, out)"""
    from semiclassical_amd._lib import lib, ptr
    b, k, U, cx = dev
    M, cols = col["lam"].shape
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to("cuda")
    S = 0 if col["sket"] is None else col["sket"].shape[0]
    sket = None if col["sket"] is None else cx(col["sket"])
    ops = dict(za=cx(col["za"]), zb=cx(col["zb"]), g=cx(col["g"]), sfix=cx(col["sfix"]), ketcol=i32(col["ketcol"]), kind=i32(col["kind"]),
               lam=torch.from_numpy(np.ascontiguousarray(col["lam"])).to("cuda"), kap=cx(col["kap"]))
    ops.update(over)
    tiles = max(int(lib.sc_wm_pair_expect_tiles(ni, nj)), 1)
    partials = torch.full((tiles, M + 1, 2), float("nan"), device="cuda")
    out = torch.full((M + 1,), float("nan"), dtype=torch.complex128, device="cuda")
    rc = lib.sc_wm_pair_expect_cols(*[ptr(t) for t in b], ni, *[ptr(t) for t in k], nj, ptr(U), D, dp, ptr(ops["za"]), ptr(ops["zb"]),
                                    ptr(ops["g"]), ptr(ops["sfix"]), ptr(sket), S, ptr(ops["ketcol"]), ptr(ops["kind"]), ptr(ops["lam"]),
                                    ptr(ops["kap"]), M, cols, ptr(partials), ptr(out), None)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


def _check_columns(dev, shape, T, Dp, b, col):
    F, Fabs = EC.column_elements(Dp, b, col["za"], col["zb"], col["g"], col["sfix"], col["sket"], col["ketcol"], col["kind"], col["lam"],
                                 col["kap"])
    want = np.concatenate(((T[None] * F).sum(axis=(1, 2)), [T.sum()]))
    scale = np.concatenate(((abs(T)[None] * Fabs).sum(axis=(1, 2)), [abs(T).sum()]))
    rc, got = _call(dev, col, *shape)
    assert rc == 0 and np.isfinite(want).all()
    worst = (abs(got - want) / scale).max()
    assert got.shape == want.shape and (abs(got - want) <= TOL * scale).all(), worst
    assert np.array_equal(got, _call(dev, col, *shape)[1])                                      # the same bits in every call
    return got, scale, worst


MIXES = (([[0, 1, 2]], [[-1, -1, -1]]),                                         # one of each kind
         ([[0, 1, 2, 1], [0, 2, 1, 0], [0, 0, 2, 2]], [[0, 1, 2, -1], [-1, 3, -1, -1], [-1, -1, 4, -1]]),   # slots on kinds 1 and 2
         ([[2, 2], [0, 1]], [[-1, 0], [-1, -1]]))                               # an operator made of kind-2 columns alone


@pytest.mark.parametrize("ni,nj", [(1, 1), (15, 17), (19, 35)])
@pytest.mark.parametrize("D,dp", [(3, 3), (16, 16), (17, 17), (40, 24), (70, 10), (64, 64)])
def test_synthetic_operands_through_the_c_abi(D, dp, ni, nj):
    """one, ragged and several tiles of 16 x 16 pairs; d' around 16, D' rows on one lane and on two"""
    from semiclassical_amd._lib import lib, ptr
    rng = np.random.default_rng(2000 * D + 10 * dp + ni + nj)
    bra, ket = _pair(rng, ni, nj, D, dp)
    T, Dp, b = WC.pair_system(bra, ket)
    dev, shape = _device(bra, ket), (ni, nj, D, dp)
    worst = max(_check_columns(dev, shape, T, Dp, b, _random_columns(rng, ni, nj, dp, kind, ketcol))[2] for kind, ketcol in MIXES)
    # kinds 0 and 1 with a slot on column 0 of every operator: the columns of sc_wm_pair_expect
    col = _random_columns(rng, ni, nj, dp, [[0, 1, 1]] * 3, [[0, -1, -1], [1, -1, -1], [2, -1, -1]])
    got, scale, w = _check_columns(dev, shape, T, Dp, b, col)
    bt, kt, U, cx = dev
    old = torch.full((4,), float("nan"), dtype=torch.complex128, device="cuda")
    partials = torch.empty((max(int(lib.sc_wm_pair_expect_tiles(ni, nj)), 1), 4, 2), device="cuda")
    held = [cx(col[k]) for k in ("za", "zb", "g", "sfix", "sket")] + [torch.from_numpy(col["lam"]).to("cuda"), cx(col["kap"])]
    assert lib.sc_wm_pair_expect(*[ptr(t) for t in bt], ni, *[ptr(t) for t in kt], nj, ptr(U), D, dp, *[ptr(t) for t in held], 3, 2,
                                 ptr(partials), ptr(old), None) == 0
    torch.cuda.synchronize()
    old = old.cpu().numpy()
    print(f"D = {D}, d' = {dp}, {ni} x {nj}: worst |got - want| / sum |terms| = {max(worst, w):.2e}; against sc_wm_pair_expect "
          f"{(abs(got - old) / scale).max():.2e}, bit-equal: {np.array_equal(got, old)}")
    assert (abs(got - old) <= 1e-12 * scale).all()


def test_capacity_at_96():
    """d' = 96: 4 columns are accepted, 5 refused with the capacity in the text"""
    from semiclassical_amd._lib import lib
    rng = np.random.default_rng(13)
    x = _synthetic(rng, 9, 96, 96)
    T, Dp, b = WC.pair_system(x, x)
    dev, shape = _device(x, x), (9, 9, 96, 96)
    _, _, worst = _check_columns(dev, shape, T, Dp, b, _random_columns(rng, 9, 9, 96, [[0, 1], [2, 1]], [[0, 1], [-1, -1]]))
    print(f"d' = 96, 4 columns: worst |got - want| / sum |terms| = {worst:.2e}")
    rc, _ = _call(dev, _random_columns(rng, 9, 9, 96, [[0, 1, 2, 1, 0]], [[-1] * 5]), *shape)
    assert rc == -2 and b"at most 4" in lib.sc_last_error()                                   # SC_ERR_UNSUPPORTED


def test_zero_leading_pivot_with_an_exponential_column():
    """the input of tests/test_wm_norm_large_gpu.py: D'[0,0] = 0 for every pair and Re D' indefinite; exp(-a.x), one kind-2 column"""
    from semiclassical_amd import hostmath
    rng = np.random.default_rng(9)
    x = _synthetic(rng, 23, 33, 20)
    U = x["U"]
    x["cqqp"] = WC.projected(U, x["cqq"])
    for a, b in ((0, 1), (2, 3)):
        x["cqqp"][:, a, a] = 0.7j                     # conj(0.7i) + 0.7i = 0
        x["cqqp"][:, a, b] = x["cqqp"][:, b, a] = 0.9 + 0.1j
    T, Dp, b = WC.pair_system(x, x)
    assert Dp[0, 1, 0, 0] == 0 and np.linalg.eigvalsh(Dp[0, 1].real).min() < 0
    a = 0.3 * WC.random_direction(rng, U)
    vx, vp, kind, lam, kap, cols = hostmath.fold_wm_operator_columns(None, None, None, None, None, (np.ones((1, 1)), a[None, None]), U)
    assert cols == 2 and kind.tolist() == [[0, 2]]
    tt = torch.from_numpy
    za, zb, g, sfix, sket, ketcol, kd = hostmath.wm_operator_columns(vx, vp, kind, lam, tt(x["Q"]), tt(x["dvec"] @ U), tt(x["Q"]),
                                                                     tt(x["cqq"]), tt(x["dvec"]), tt(x["dvec"] @ U), tt(U))
    assert sket is None
    col = dict(za=za.numpy(), zb=zb.numpy(), g=g.numpy(), sfix=sfix.numpy(), sket=None, lam=lam.numpy(), kap=kap.numpy(),
               kind=kd.numpy(), ketcol=ketcol.numpy())
    got, scale, _ = _check_columns(_device(x, x), (23, 23, 33, 20), T, Dp, b, col)
    iD = np.linalg.inv(Dp)                                                                    # the direct formula
    xbar = x["Q"][:, None, :] + np.einsum('ak,ijkl,ijl->ija', U, iD, b, optimize=True)
    aBa = np.einsum('k,ijkl,l->ij', U.T @ a, iD, U.T @ a)
    want = (T * np.exp(-(xbar @ a) + 0.5 * aBa)).sum()
    assert np.isfinite(want) and abs(got[0] - want) <= TOL * scale[0]


def test_c_abi_refusals():
    from semiclassical_amd._lib import lib
    rng = np.random.default_rng(15)
    x = _synthetic(rng, 5, 4, 3)
    dev, shape = _device(x, x), (5, 5, 4, 3)
    col = _random_columns(rng, 5, 5, 3, [[0, 1, 2]], [[-1, 0, 1]])
    assert _call(dev, col, *shape)[0] == 0
    i32 = lambda *a: torch.tensor(a, dtype=torch.int32, device="cuda")
    for kind in (i32(0, 3, 2), i32(-1, 1, 2)):
        assert _call(dev, col, *shape, kind=kind)[0] == -1 and b"kind" in lib.sc_last_error()     # SC_ERR_BAD_ARGUMENT
    for ketcol in (i32(-1, 0, 2), i32(-2, 0, 1)):
        assert _call(dev, col, *shape, ketcol=ketcol)[0] == -1 and b"ketcol" in lib.sc_last_error()
    assert _call(dev, dict(col, sket=None), *shape)[0] == -1 and b"ketcol" in lib.sc_last_error()  # S = 0 and a slot named
    for name in ("za", "kind", "ketcol", "lam"):
        assert _call(dev, col, *shape, **{name: None})[0] == -1 and b"null argument" in lib.sc_last_error()
    rc, out = _call(dev, col, 0, 5, 4, 3)                                          # no pairs: the sums are zero
    assert rc == 0 and out.tolist() == [0.0, 0.0]


def test_more_columns_than_one_call_holds():
    """d' = 64: one call holds 36 columns; two operators of 40 columns of all kinds, slots on every third, go through the split of
    wm_pair_expect_cols in four calls, against numpy"""
    from semiclassical_amd import propagators as PR
    from semiclassical_amd._lib import lib
    rng = np.random.default_rng(17)
    x = _synthetic(rng, 9, 64, 64)
    T, Dp, b = WC.pair_system(x, x)
    assert lib.sc_wm_pair_expect_capacity(64, 64) == 36
    kind = rng.integers(0, 3, size=(2, 40))
    kind[:, 0] = 0
    ketcol = np.full(80, -1)
    ketcol[::3] = np.arange(len(ketcol[::3]))
    col = _random_columns(rng, 9, 9, 64, kind, ketcol.reshape(2, 40))
    col["lam"][1, 5:9] = 0.0                                                     # columns of zeros inside an operator
    col["kind"][45:49] = 1
    F, Fabs = EC.column_elements(Dp, b, col["za"], col["zb"], col["g"], col["sfix"], col["sket"], col["ketcol"], col["kind"], col["lam"],
                                 col["kap"])
    want = np.concatenate(((T[None] * F).sum(axis=(1, 2)), [T.sum()]))
    scale = np.concatenate(((abs(T)[None] * Fabs).sum(axis=(1, 2)), [abs(T).sum()]))
    bt, kt, U, cx = _device(x, x)
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to("cuda")
    run = lambda: PR.wm_pair_expect_cols(bt, kt, U, cx(col["za"]), cx(col["zb"]), cx(col["g"]), cx(col["sfix"]), cx(col["sket"]),
                                         i32(col["ketcol"]), i32(col["kind"]), torch.from_numpy(col["lam"]).to("cuda"), cx(col["kap"]))
    got = run()
    print("d' = 64, 80 columns through the split: |got - want| / sum |terms| =", abs(got - want) / scale)
    assert np.isfinite(want).all() and (abs(got - want) <= TOL * scale).all()
    assert np.array_equal(got, run())
