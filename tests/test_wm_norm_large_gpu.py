"""WM norm() beyond 16 non-zero width modes (16 < d' <= 96, or 64 < D <= 512): the wide pair-sum kernel against the
reference's values, the CPU oracle and a numpy restatement of the pair sum."""
import logging

import numpy as np
import pytest
import torch

from tests import cases

pytestmark = pytest.mark.gpu
torch.set_default_dtype(torch.float64)      # the oracle follows the reference's global default (cli.py:121)


@pytest.mark.parametrize("name,tag", [("wm_as24", "as24"), ("wm_as60", "as60"), ("wm_coumarin_harmonic", "cou")])
def test_norm_matches_reference(name, tag):
    from tests.engine_cases import engine_potential, engine_propagator
    g, ref = cases.load(name), cases.load("wm_norms_large")
    pot, prop = engine_potential(g), engine_propagator(g)
    x = cases.T(ref[f"{tag}_xgrid"])
    want = float(ref[f"{tag}_norm_0"])
    assert abs(prop.norm() - want) < 1e-8 * want
    assert cases.rel_err(prop.coefficients().cpu().numpy(), ref[f"{tag}_coeff_0"]) < 1e-9
    assert cases.rel_err(prop.wavefunction(x), ref[f"{tag}_psi_0"]) < 1e-8
    n = int(ref[f"{tag}_nsteps"])
    for _ in range(n):
        prop.step(pot, float(g["dt"]))
    want = float(ref[f"{tag}_norm_{n}"])
    assert abs(prop.norm() - want) < 1e-8 * want
    assert cases.rel_err(prop.coefficients().cpu().numpy(), ref[f"{tag}_coeff_{n}"]) < 1e-9
    assert cases.rel_err(prop.wavefunction(x), ref[f"{tag}_psi_{n}"]) < 1e-8


@pytest.mark.parametrize("D,dp,n", [(17, 17, 61), (33, 32, 75), (40, 33, 100), (64, 48, 53), (64, 64, 45), (80, 72, 39),
                                    (96, 96, 37), (80, 12, 83)])
def test_norm_matches_oracle_at_random_shapes(D, dp, n):
    """dense rotated widths, rank deficient where d' < D; n not a multiple of the 16-pair tile; a few Morse steps.
    At D > 64 the per-trajectory C_QQ that the WM step exports already differs from the oracle's by ~1e-6 per step (the
    coefficients agree to 1e-14), so there the pair sum is compared at t = 0 only."""
    from oracle import norm_oracle, sc_oracle as orc
    from semiclassical_amd import potentials as P, propagators as PR
    rng = np.random.default_rng(1000 + 7 * D + dp)
    omega = torch.from_numpy(np.sort(rng.uniform(600, 2500, D)) / 219474.63)
    S = torch.from_numpy(rng.uniform(0.05, 0.3, D) * rng.choice([-1, 1], D))
    nac = torch.from_numpy(rng.normal(0, 1e-3, D))
    chi = torch.full((D,), 0.01)
    q0 = torch.sqrt(2 * abs(S) / omega) * torch.sign(S)
    p0 = 0.0 * q0
    Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    w = omega.numpy() * rng.uniform(0.7, 1.4, D)
    w[dp:] = 0.0
    G = torch.from_numpy(Q @ np.diag(w) @ Q.T)
    G = 0.5 * (G + G.T)
    ref = orc.WMOracle(G, G, 60.0, 60.0)
    prop = PR.WaltonManolopoulosPropagator(G, G, 60.0, 60.0, device="cuda")
    torch.manual_seed(D + dp)
    ref.initial_conditions(q0, p0, G, ntraj=n)
    prop.set_initial_conditions(q0, p0, G, ref.zi, ref.probi)
    assert prop._wm_host.dprime == dp
    opot, epot = orc.MorseOracle(omega, chi.clone(), nac), P.MorsePotential(omega, chi.clone(), nac)
    want = norm_oracle.wm_norm(ref)
    assert abs(prop.norm() - want) <= 1e-9 * want
    if D > 64:
        return
    for _ in range(3):
        ref.step(opot, 3.0)
        prop.step(epot, 3.0)
    want = norm_oracle.wm_norm(ref)
    assert abs(prop.norm() - want) <= 1e-9 * want


# ---- direct calls of the C ABI on synthetic inputs ------------------------------------------------------------------

def _synthetic(rng, n, D, dp, width=1.0, spread=0.3):
    """per-trajectory inputs of sc_wm_pair_sum: complex symmetric C_QQ with a positive definite real part"""
    U, _ = np.linalg.qr(rng.standard_normal((D, dp)))
    qp = rng.normal(0.0, spread, (n, 2 * D))
    coef = rng.normal(size=n) + 1j * rng.normal(size=n)
    cqq = np.empty((n, D, D), dtype=complex)
    for t in range(n):
        A = rng.standard_normal((D, D)) / np.sqrt(D)
        B = rng.standard_normal((D, D)) / np.sqrt(D)
        cqq[t] = width * (np.eye(D) + 0.2 * (A @ A.T) + 0.3j * (B + B.T))
    dvec = 0.1 * width * (rng.normal(size=(n, D)) + 1j * rng.normal(size=(n, D)))
    cqqp = np.einsum('ak,nab,bl->nkl', U, cqq, U)
    dvecp = dvec @ U
    return dict(qp=qp, coef=coef, cqq=cqq, dvec=dvec, cqqp=cqqp, dvecp=dvecp, U=U)


def _restated(bra, ket):
    """sum_ij conj(v_i) O_ij v_j with O_ij = det(D'/2pi)^-1/2 exp(-1/2 dQ^T C_j dQ - d_j.dQ + 1/2 b'^T D'^-1 b'),
    D' = conj(C'_i) + C'_j, b' = U^T C_j dQ + conj(d'_i) + d'_j; the determinant through slogdet (principal sqrt)"""
    D = ket["U"].shape[0]
    total = 0j
    for i in range(len(bra["coef"])):
        for j in range(len(ket["coef"])):
            dQ = ket["qp"][j, :D] - bra["qp"][i, :D]
            Cj = ket["cqq"][j]
            Dp = bra["cqqp"][i].conj() + ket["cqqp"][j]
            b = ket["U"].T @ (Cj @ dQ) + bra["dvecp"][i].conj() + ket["dvecp"][j]
            sign, logabs = np.linalg.slogdet(Dp / (2 * np.pi))
            ex = -0.5 * dQ @ Cj @ dQ - ket["dvec"][j] @ dQ + 0.5 * b @ np.linalg.solve(Dp, b)
            total += np.conj(bra["coef"][i]) * np.exp(ex - 0.5 * logabs) / np.sqrt(sign) * ket["coef"][j]
    return total


def _engine(bra, ket):
    from semiclassical_amd._lib import lib, check, ptr
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    cx = lambda a: torch.view_as_real(dev(np.ascontiguousarray(a, dtype=complex))).contiguous()
    D, dp = bra["U"].shape
    ni, nj = len(bra["coef"]), len(ket["coef"])
    bufs = [dev(bra["qp"]), cx(bra["coef"]), cx(bra["cqqp"]), cx(bra["dvecp"]), dev(ket["qp"]), cx(ket["coef"]), cx(ket["cqq"]),
            cx(ket["dvec"]), cx(ket["cqqp"]), cx(ket["dvecp"]), dev(ket["U"])]
    tiles = lib.sc_wm_pair_sum_rect_tiles(ni, nj)
    partials = torch.full((tiles, 4), float("nan"), device="cuda")
    p = [ptr(b) for b in bufs]
    check(lib.sc_wm_pair_sum_rect(p[0], p[1], p[2], p[3], ni, p[4], p[5], p[6], p[7], p[8], p[9], nj, p[10], D, dp,
                                  ptr(partials), None))
    torch.cuda.synchronize()
    s = partials.cpu().numpy().sum(axis=0)
    return complex(s[0], s[1])


def _rows(x, sel):
    return dict({k: v[sel] for k, v in x.items() if k != "U"}, U=x["U"])


@pytest.mark.parametrize("D,dp", [(40, 24), (70, 10), (64, 64)])
def test_rectangular_calls_match_the_restated_sum(D, dp):
    rng = np.random.default_rng(D + dp)
    bra, ket = _synthetic(rng, 19, D, dp), _synthetic(rng, 35, D, dp)
    ket["U"] = bra["U"]
    ket["cqqp"] = np.einsum('ak,nab,bl->nkl', ket["U"], ket["cqq"], ket["U"])
    ket["dvecp"] = ket["dvec"] @ ket["U"]
    want = _restated(bra, ket)
    assert abs(_engine(bra, ket) - want) <= 1e-10 * abs(want)


def test_split_bras_sum_to_the_square_call():
    from semiclassical_amd._lib import lib, check, ptr
    rng = np.random.default_rng(5)
    x = _synthetic(rng, 45, 30, 21)
    whole = _engine(x, x)
    halves = _engine(_rows(x, slice(0, 22)), x) + _engine(_rows(x, slice(22, None)), x)
    assert abs(halves - whole) <= 1e-12 * abs(whole)
    # the square entry point is the rectangular call with bras = kets
    dev = lambda a: torch.view_as_real(torch.from_numpy(np.ascontiguousarray(a, dtype=complex))).contiguous().to("cuda")
    bufs = [torch.from_numpy(x["qp"]).cuda(), dev(x["coef"]), dev(x["cqq"]), dev(x["dvec"]), dev(x["cqqp"]), dev(x["dvecp"]),
            torch.from_numpy(x["U"]).cuda()]
    tiles = lib.sc_wm_pair_sum_tiles(45)
    partials = torch.full((tiles, 4), float("nan"), device="cuda")
    p = [ptr(b) for b in bufs]
    check(lib.sc_wm_pair_sum(p[0], p[1], p[2], p[3], p[4], p[5], p[6], 45, 30, 21, ptr(partials), None))
    torch.cuda.synchronize()
    s = partials.cpu().numpy().sum(axis=0)
    assert complex(s[0], s[1]) == whole


def test_zero_leading_pivot_and_indefinite_real_part():
    """D'[0,0] = 0 for every pair and Re D' indefinite: the elimination must pivot.  Re D' gets two negative eigenvalues:
    D'_ii = 2 Re C'_i is real, and with an odd number its determinant would sit on the branch cut of the square root."""
    rng = np.random.default_rng(9)
    x = _synthetic(rng, 23, 33, 20)
    for a, b in ((0, 1), (2, 3)):
        x["cqqp"][:, a, a] = 0.7j                     # conj(0.7i) + 0.7i = 0
        x["cqqp"][:, a, b] = x["cqqp"][:, b, a] = 0.9 + 0.1j
    Dp = x["cqqp"][0].conj() + x["cqqp"][1]
    assert Dp[0, 0] == 0 and np.linalg.eigvalsh(Dp.real).min() < 0
    args = [abs(np.angle(np.linalg.det(x["cqqp"][i].conj() + x["cqqp"][j]))) for i in range(23) for j in range(23)]
    assert np.pi - max(args) > 0.1
    want = _restated(x, x)
    assert np.isfinite(want) and abs(_engine(x, x) - want) <= 1e-10 * abs(want)


def test_determinant_below_the_double_range():
    """det(D'/2pi) ~ 1e-365 underflows a double; O_ij ~ 1e182 is representable and must come out finite"""
    rng = np.random.default_rng(11)
    x = _synthetic(rng, 21, 96, 96, width=5e-4, spread=0.01)
    x["coef"] *= 1e-90
    Dp = x["cqqp"][0].conj() + x["cqqp"][0]
    assert np.linalg.slogdet(Dp / (2 * np.pi))[1] < np.log(1e-300)
    want = _restated(x, x)
    got = _engine(x, x)
    assert np.isfinite(got) and np.isfinite(want) and abs(want) > 1e-10
    assert abs(got - want) <= 1e-10 * abs(want)


def test_refuses_shapes_beyond_the_limits():
    from semiclassical_amd._lib import EngineError, lib, check
    buf = torch.zeros(8, device="cuda")
    from semiclassical_amd._lib import ptr
    p = ptr(buf)
    for D, dp in ((513, 8), (120, 97)):
        with pytest.raises(EngineError, match="D <= 512, d' <= 96"):
            check(lib.sc_wm_pair_sum(p, p, p, p, p, p, p, 4, D, dp, p, None))


def test_driver_calc_norm_every_with_wm(tmp_path, caplog):
    """cli.py:418-429 with the WM propagator on the 24-mode AS model: finite norms logged, correlations unchanged"""
    from semiclassical_amd import driver
    g = cases.load("wm_as24")
    model = tmp_path / "AS_model.dat"
    rows = np.vstack((g["omega"] * 219474.63, 0.5 * g["omega"] * g["q0"] ** 2 * np.sign(g["q0"]), g["nac"], g["chi"])).T
    np.savetxt(model, rows)
    res, norms = [], []
    for every in (0, 3):
        out = tmp_path / f"c{every}.npz"
        task = {"task": "dynamics", "potential": {"type": "anharmonic AS", "model_file": str(model)},
                "propagator": "WM", "batch_size": 40, "num_trajectories": 40, "num_steps": 8, "time_step_fs": 0.04,
                "results": {"correlations": str(out)}, "manual_seed": 3, "calc_norm_every": every}
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="semiclassical_amd.driver"):
            driver.run_semiclassical_dynamics(task, device="cuda")
        res.append(dict(np.load(out)))
        norms.append([float(r.getMessage().split("norm=")[1]) for r in caplog.records if "norm=" in r.getMessage()])
    assert norms[0] == []
    assert len(norms[1]) == 3 and all(np.isfinite(v) and v > 0 for v in norms[1])        # t = 0, 3, 6
    assert np.allclose(res[0]["autocorrelation"], res[1]["autocorrelation"], rtol=1e-13, atol=0)
    assert np.allclose(res[0]["ic_correlation"], res[1]["ic_correlation"], rtol=1e-13, atol=0)
