"""WaltonManolopoulosPropagator.wm_expectation / wm_wavepacket_moments (sc_wm_pair_expect) against the numpy
restatement of tests/wm_expect_cases.py on the engine's own export and on the oracle's state, against norm(), the untouched state,
and the C-ABI on synthetic operands: tile and lane edges, the split into calls, pivoting, limits."""
import numpy as np
import pytest
import torch

from tests import cases, wm_expect_cases as WC

pytestmark = pytest.mark.gpu
torch.set_default_dtype(torch.float64)

TOL = 1e-9          # x A_a = sum_ij |T_ij F_a,ij|: the bound of section 4.21
ORACLE_TOL = 1e-8   # against the oracle's state: the bound of the WM norm tests
MEANINGFUL = 5e-3   # |E_a| / A_a at least: the bound cannot hide a wrong factor behind cancellation
LABELS = ("1", "x", "p", "x^2")


def _advanced(name, steps, ntraj=48, oracle=False):
    from tests.engine_cases import engine_potential, engine_propagator
    g = cases.load(name)
    g["zi"], g["probi"] = g["zi"][:, :ntraj], g["probi"][:ntraj]
    pot, prop = engine_potential(g), engine_propagator(g)
    for _ in range(steps):
        prop.step(pot, float(g["dt"]))
    ref = None
    if oracle:
        ref, opot = cases.oracle_propagator(g), cases.oracle_potential(g)
        for _ in range(steps):
            ref.step(opot, float(g["dt"]))
    return g, pot, prop, ref


# ------------------------------------------------------------------------------------------- 1. engine vs restatement

@pytest.mark.parametrize("name", ["wm_1d", "wm_as5_chi002", "wm_methylium", "wm_as24"])
def test_engine_matches_restatement_on_its_own_export(name):
    """seed 1: on the oracle's states the smallest |E_a| / A_a is 3.4e-2 (p on wm_1d, which has no direction to choose), the
    others are at least 0.27"""
    _, _, prop, _ = _advanced(name, 3)
    state = WC.engine_state(prop)
    c, m, K, n = WC.standard_operators(np.random.default_rng(1), state["U"])
    E, A, N2 = WC.restated_expectation(state, state, c, m, K, n)
    got, norm2 = prop.wm_expectation(c, m, K, n, normalise=False)
    assert got.shape == (4,) and got.dtype == np.complex128 and isinstance(norm2, float)
    for a, label in enumerate(LABELS):
        print(f"{name} {label:4s}: |E| / A = {abs(got[a]) / A[a]:.3e}, |E - restatement| / A = {abs(got[a] - E[a]) / A[a]:.2e}")
    assert (abs(got) >= MEANINGFUL * A).all()
    assert (abs(got - E) <= TOL * A).all()
    assert abs(norm2 - N2.real) <= TOL * A[0] and got[0].real == norm2
    assert abs(norm2 - prop.norm() ** 2) <= 1e-9 * norm2
    vals, again = prop.wm_expectation(c, m, K, n)
    assert again == norm2 and (abs(vals - got / norm2) <= 1e-15 * abs(vals)).all()
    few, _ = prop.wm_expectation(x=m[1:2], normalise=False)
    assert few.shape == (1,) and abs(few[0] - got[1]) <= 1e-13 * A[1]


def test_engine_matches_restatement_on_the_oracle_state():
    _, _, prop, ref = _advanced("wm_as5_chi002", 3, oracle=True)
    state = WC.oracle_state(ref)
    c, m, K, n = WC.standard_operators(np.random.default_rng(1), state["U"])
    E, A, N2 = WC.restated_expectation(state, state, c, m, K, n)
    got, norm2 = prop.wm_expectation(c, m, K, n, normalise=False)
    for a, label in enumerate(LABELS):
        print(f"oracle state {label:4s}: |E| / A = {abs(got[a]) / A[a]:.3e}, |E - restatement| / A = {abs(got[a] - E[a]) / A[a]:.2e}")
    assert (abs(got) >= MEANINGFUL * A).all()
    assert (abs(got - E) <= ORACLE_TOL * A).all() and abs(norm2 - N2.real) <= ORACLE_TOL * A[0]


def test_wavepacket_moments():
    _, _, prop, _ = _advanced("wm_as5_chi002", 3)
    state = WC.engine_state(prop)
    D = prop.dim
    dense = np.random.default_rng(21).uniform(0.5, 1.5, D)
    AN = abs(WC.pair_system(state, state)[0]).sum()
    for directions, U in ((None, np.eye(D)), ([0, D - 1], np.eye(D)[[0, D - 1]]), (D - 2, np.eye(D)[[D - 2]]), (dense, dense[None, :])):
        Md = U.shape[0]
        sq, zv, zm = np.stack([2.0 * np.outer(u, u) for u in U]), np.zeros((Md, D)), np.zeros((Md, D, D))
        E, A, N2 = WC.restated_expectation(state, state, None, np.concatenate((U, zv, zv)), np.concatenate((zm, sq, zm)),
                                           np.concatenate((zv, zv, U)))
        want = (E / N2).real
        tol = TOL * (A + abs(E) * AN / abs(N2)) / abs(N2)       # of E_a / N2 when E_a is off by TOL A_a and N2 by TOL sum |T|
        got = prop.wm_wavepacket_moments() if directions is None else prop.wm_wavepacket_moments(directions)
        assert sorted(got) == ["norm2", "p", "var_x", "x"] and abs(got["norm2"] - N2.real) <= TOL * AN
        x, xx, pm = (want[k * Md:(k + 1) * Md] for k in range(3))
        tx, txx, tp = (tol[k * Md:(k + 1) * Md] for k in range(3))
        assert got["x"].shape == (Md,) and (abs(got["x"] - x) <= tx).all() and (abs(got["p"] - pm) <= tp).all()
        assert (abs(got["var_x"] - (xx - x ** 2)) <= txx + 2.0 * abs(x) * tx).all() and (got["var_x"] > 0).all()


def test_refusals_of_the_methods():
    _, _, prop, _ = _advanced("wm_methylium", 0, ntraj=8)
    U = prop._wm_bufs["U"].cpu().numpy()
    null = np.linalg.svd(U.T)[2][-1]
    inside = U[:, 0]
    assert prop.wm_wavepacket_moments(inside)["var_x"][0] > 0
    with pytest.raises(ValueError, match="x of operator 0 .* outside the range"):
        prop.wm_expectation(x=null[None])
    with pytest.raises(ValueError, match="give directions"):
        prop.wm_wavepacket_moments()
    with pytest.raises(ValueError, match="outside the range"):
        prop.wm_wavepacket_moments(null)
    with pytest.raises(ValueError):
        prop.wm_wavepacket_moments(np.zeros(prop.dim))
    with pytest.raises(TypeError):
        prop.wm_expectation(pp=np.eye(prop.dim)[None])           # there is no quadratic momentum part
    for call in (lambda: prop.expectation(c=np.ones(1)), lambda: prop.wavepacket_moments(0), lambda: prop.reduced_density(0, [0.0])):
        with pytest.raises(NotImplementedError, match="per-trajectory widths"):
            call()


# ------------------------------------------------------------------------------------------- 2. the state is not touched

def test_state_is_untouched():
    from tests.engine_cases import engine_potential, engine_propagator
    g = cases.load("wm_as5_chi002")
    g["zi"], g["probi"] = g["zi"][:, :40], g["probi"][:40]
    pot, dt, E0 = engine_potential(g), float(g["dt"]), float(g["E0"])
    prop, twin = engine_propagator(g), engine_propagator(g)
    c, m, K, n = WC.standard_operators(np.random.default_rng(5), g["U"].real)
    outs = []
    for pr, calls in ((prop, True), (twin, False)):
        pr.step(pot, dt)
        rows = []
        for _ in range(2):
            if calls:
                first = pr.wm_expectation(c, m, K, n)
                second = pr.wm_expectation(c, m, K, n)
                assert np.array_equal(first[0], second[0]) and first[1] == second[1]            # the same bits in every call
                pr.wm_wavepacket_moments([0, 1])
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


# ------------------------------------------------------------------------------------------- 3. the C-ABI on synthetic operands

def _synthetic(rng, n, D, dp, width=1.0, spread=0.3):
    """per-trajectory inputs of the WM pair sums: complex symmetric C_QQ with a positive definite real part (the recipe of
    tests/test_wm_norm_large_gpu.py)"""
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
    """(bra tensors, ket tensors, U) as wm_pair_expect takes them"""
    re = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda")
    cx = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=complex)).to("cuda")
    U = ket["U"]
    qp = lambda s: re(np.hstack((s["Q"], np.zeros_like(s["Q"]))))
    cqqp = lambda s: cx(s["cqqp"] if "cqqp" in s else WC.projected(U, s["cqq"]))
    return ((qp(bra), cx(bra["coef"]), cqqp(bra), cx(bra["dvec"] @ U)),
            (qp(ket), cx(ket["coef"]), cx(ket["cqq"]), cx(ket["dvec"]), cqqp(ket), cx(ket["dvec"] @ U)), re(U), cx)


def _random_columns(rng, ni, nj, dp, M, R, perket):
    C = M * (1 + R)
    cn = lambda *shape: rng.normal(size=shape) + 1j * rng.normal(size=shape)
    return dict(za=cn(C, ni), zb=cn(C, nj), g=cn(C, dp), sfix=cn(C, dp), sket=cn(M, nj, dp) if perket else None,
                lam=rng.normal(size=(M, 1 + R)), kap=cn(M))


def _engine(bra, ket, col):
    from semiclassical_amd import propagators as PR
    b, k, U, cx = _device(bra, ket)
    sket = None if col["sket"] is None else cx(col["sket"])
    lam = torch.from_numpy(np.ascontiguousarray(col["lam"])).to("cuda")
    out = PR.wm_pair_expect(b, k, U, cx(col["za"]), cx(col["zb"]), cx(col["g"]), cx(col["sfix"]), sket, lam, cx(col["kap"]))
    torch.cuda.synchronize()
    return out


def _pair_sum(bra, ket):
    """sc_wm_pair_sum_rect + the sum of its tiles -> complex"""
    from semiclassical_amd._lib import check, lib, ptr
    b, k, U, _ = _device(bra, ket)
    ni, nj = b[0].shape[0], k[0].shape[0]
    D, dp = U.shape
    partials = torch.full((lib.sc_wm_pair_sum_rect_tiles(ni, nj), 4), float("nan"), device="cuda")
    check(lib.sc_wm_pair_sum_rect(*[ptr(t) for t in b], ni, *[ptr(t) for t in k], nj, ptr(U), D, dp, ptr(partials), None))
    torch.cuda.synchronize()
    s = partials.cpu().numpy().sum(axis=0)
    return complex(s[0], s[1])


def _check_columns(bra, ket, T, Dp, b, col):
    F = WC.column_elements(Dp, b, col["za"], col["zb"], col["g"], col["sfix"], col["sket"], col["lam"], col["kap"])
    terms = np.concatenate((T[None] * F, T[None]))
    want, scale = terms.sum(axis=(1, 2)), abs(terms).sum(axis=(1, 2))
    got = _engine(bra, ket, col)
    worst = (abs(got - want) / scale).max()
    assert got.shape == want.shape and (abs(got - want) <= TOL * scale).all(), worst
    assert np.array_equal(got, _engine(bra, ket, col))                                          # the same bits in every call
    return got, scale, worst


@pytest.mark.parametrize("ni,nj", [(1, 1), (15, 17), (16, 16), (19, 35)])
@pytest.mark.parametrize("D,dp", [(3, 3), (16, 16), (17, 17), (40, 24), (70, 10), (64, 64)])
def test_synthetic_operands_through_the_c_abi(D, dp, ni, nj):
    """one, ragged, full and several tiles of 16 x 16 pairs; d' around the 16 of the norm's two kernels, D' rows on one lane and on
    two; (M, R) = (2, d') at d' = 64 holds 130 columns, more than one call carries: the split of wm_pair_expect"""
    from semiclassical_amd._lib import lib
    rng = np.random.default_rng(1000 * D + 10 * dp + ni + nj)
    bra, ket = _pair(rng, ni, nj, D, dp)
    T, Dp, b = WC.pair_system(bra, ket)
    worst = 0.0
    for M, R in ((1, 0), (3, 2), (2, dp)):
        for perket in (False, True):
            _, _, w = _check_columns(bra, ket, T, Dp, b, _random_columns(rng, ni, nj, dp, M, R, perket))
            worst = max(worst, w)
    print(f"D = {D}, d' = {dp}, {ni} x {nj}: capacity {lib.sc_wm_pair_expect_capacity(D, dp)}, worst |got - want| / sum |terms| = {worst:.2e}")
    # M = 1, R = 0 with a column of zeros and kappa = 1 is the sum of sc_wm_pair_sum_rect
    zero = dict(za=np.zeros((1, ni)), zb=np.zeros((1, nj)), g=np.zeros((1, dp)), sfix=np.zeros((1, dp)), sket=None, lam=np.ones((1, 1)),
                kap=np.ones(1))
    one, plain, sum_abs_t = _engine(bra, ket, zero), _pair_sum(bra, ket), abs(T).sum()
    assert abs(one[0] - plain) <= 1e-12 * sum_abs_t and abs(one[1] - plain) <= 1e-12 * sum_abs_t


def test_zero_leading_pivot_and_indefinite_real_part():
    """the input of tests/test_wm_norm_large_gpu.py: D'[0,0] = 0 for every pair and Re D' indefinite; one x operator"""
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
    u = WC.random_direction(rng, U)
    vx, nvec, lam, kap, R = hostmath.fold_wm_expectation_operators(None, u[None], None, None, U)
    tt = torch.from_numpy
    za, zb, g, sfix, sket = hostmath.wm_expectation_columns(vx, nvec, tt(x["Q"]), tt(x["dvec"] @ U), tt(x["Q"]), tt(x["cqq"]),
                                                            tt(x["dvec"]), tt(x["dvec"] @ U), tt(U))
    col = dict(za=za.numpy(), zb=zb.numpy(), g=g.numpy(), sfix=sfix.numpy(), sket=None, lam=lam.numpy(), kap=kap.numpy())
    got, scale, _ = _check_columns(x, x, T, Dp, b, col)
    xbar = x["Q"][:, None, :] + np.einsum('ak,ijkl,ijl->ija', U, np.linalg.inv(Dp), b, optimize=True)         # the direct formula
    want = (T * (xbar @ u)).sum()
    assert np.isfinite(want) and abs(got[0] - want) <= TOL * scale[0]


def test_more_columns_than_one_call_holds():
    """d' = 96: one call holds 4 columns; two operators of 1 + 3 columns go through the split, the call itself refuses them"""
    from semiclassical_amd import hostmath, propagators as PR
    from semiclassical_amd._lib import lib, ptr
    rng = np.random.default_rng(11)
    x = _synthetic(rng, 21, 96, 96)
    U = x["U"]
    assert lib.sc_wm_pair_expect_capacity(96, 96) == 4
    c, n = rng.normal(size=2), rng.normal(size=(2, 96))
    m = rng.normal(size=(2, 96))
    V = np.linalg.qr(rng.standard_normal((96, 3)))[0]
    K = np.stack([(V * np.array([1.0, -0.5, 2.0])) @ V.T, (V[:, :2] * np.array([0.7, 1.1])) @ V[:, :2].T])
    E, A, N2 = WC.restated_expectation(x, x, c, m, K, n)
    vx, nvec, lam, kap, R = hostmath.fold_wm_expectation_operators(c, m, K, n, U)
    assert R == 3
    b, k, Ud, cx = _device(x, x)
    za, zb, g, sfix, sket = hostmath.wm_expectation_columns(vx, nvec, b[0][:, :96], b[3], k[0][:, :96], k[2], k[3], k[5], Ud)
    got = PR.wm_pair_expect(b, k, Ud, za, zb, g, sfix, sket, lam.to("cuda"), kap.to("cuda"))
    print("d' = 96 through the split: |E - restatement| / A =", abs(got[:2] - E) / A, abs(got[2] - N2) / abs(N2))
    assert (abs(got[:2] - E) <= TOL * A).all() and abs(got[2] - N2) <= TOL * abs(WC.pair_system(x, x)[0]).sum()
    partials, out = torch.zeros((4, 3, 2), device="cuda"), torch.zeros(3, dtype=torch.complex128, device="cuda")
    rc = lib.sc_wm_pair_expect(*[ptr(t) for t in b], 21, *[ptr(t) for t in k], 21, ptr(Ud), 96, 96, ptr(za), ptr(zb), ptr(g), ptr(sfix),
                               ptr(sket), ptr(lam.to("cuda")), ptr(kap.to("cuda")), 2, 3, ptr(partials), ptr(out), None)
    assert rc == -2 and b"at most 4" in lib.sc_last_error()                                   # SC_ERR_UNSUPPORTED


def test_c_abi_refusals():
    from semiclassical_amd import _lib
    from semiclassical_amd._lib import lib, ptr
    buf, part, out = torch.zeros(4096, device="cuda"), torch.zeros(64, device="cuda"), torch.full((4,), 7.0, device="cuda")
    p, s, o = ptr(buf), ptr(part), ptr(out)

    def args(M=1, R=0, ni=2, nj=2, D=3, dp=2, first=p, za=p, sket=None, last=o):
        return (first, p, p, p, ni, p, p, p, p, p, p, nj, p, D, dp, za, p, p, p, sket, p, p, M, R, s, last, None)
    for bad in (dict(first=None), dict(za=None), dict(last=None), dict(M=0), dict(R=-1)):
        assert lib.sc_wm_pair_expect(*args(**bad)) == -1                            # SC_ERR_BAD_ARGUMENT
    assert lib.sc_wm_pair_expect(*args(last=None)) == -1 and b"null argument" in lib.sc_last_error()
    for D, dp in ((513, 8), (120, 97), (4, 5)):
        assert lib.sc_wm_pair_expect(*args(D=D, dp=dp)) == -2                       # SC_ERR_UNSUPPORTED
        assert b"D <= 512, d' <= 96" in lib.sc_last_error()
    assert lib.sc_wm_pair_expect(*args(M=65536)) == -2 and b"M <= 65535" in lib.sc_last_error()
    assert lib.sc_wm_pair_expect(*args(M=50, R=1)) == -2 and b"at most 98" in lib.sc_last_error()
    with pytest.raises(_lib.EngineError, match="at most 98"):
        _lib.check(lib.sc_wm_pair_expect(*args(M=99)))
    assert lib.sc_wm_pair_expect(*args(ni=0)) == 0                                  # no pairs: the sums are zero
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [0.0, 0.0, 0.0, 0.0]
    assert lib.sc_wm_pair_expect(*args()) == 0                                      # 2 x 2 pairs of zeros: D' = 0 is singular, nothing added
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [0.0, 0.0, 0.0, 0.0]
