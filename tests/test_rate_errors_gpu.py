"""Block sums of run(..., blocks=...) on every route.  The oracle is the host grouping, by (i >> 2) & (B - 1), of the
per-trajectory terms the step-at-a-time path exports in _cq / _kq after ic_correlation(); tolerance 1e-12 relative to the sum of
|term| over the block.  In every case the blocks add up to the slot row and slots / moments are the same bit for bit as in a run
without blocks.  Then the driver's task key and two ranks flushing blocks and counts in the one collective."""
import os

import numpy as np
import pytest
import torch

from tests import cases, engine_cases
from tests.lib_spy import LibSpy

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_default_dtype(torch.float64)

TOL = 1e-12


def _group(terms, local, B):
    """(n,) complex terms -> (B,) block sums and (B,) sums of |term|, the trajectories partitioned by their rank-local index"""
    from semiclassical_amd import hostmath
    blk = hostmath.error_block(local, B)
    sums = np.array([terms[blk == b].sum() for b in range(B)])
    scale = np.array([np.abs(terms[blk == b]).sum() for b in range(B)])
    return sums, scale


def _oracle(prop, pot, dt, nt, B, local=None, has_k=True):
    """step-at-a-time path: per step the block sums (B,) of C and k terms and the sums of |term| they are compared against"""
    prop._whole_loop_ok = False
    local = np.arange(prop.ntraj) if local is None else local
    rows = []
    for _ in range(nt):
        prop.ic_correlation(pot)
        cq, kq = prop._cq.cpu().numpy(), prop._kq.cpu().numpy()
        rows.append(_group(cq, local, B) + (_group(kq, local, B) if has_k else (np.zeros(B), np.zeros(B))))
        prop.step(pot, dt)
    prop.synchronize()
    C, sC, k, sk = (np.array(x) for x in zip(*rows))
    return C, k, sC, sk


def _assert_blocks(blocks, want, label=""):
    """blocks (nt, B, 4) raw sums against the oracle (C, k, scale_C, scale_k), each (nt, B)"""
    C, k, sC, sk = want
    gotC, gotk = blocks[:, :, 0] + 1j * blocks[:, :, 1], blocks[:, :, 2] + 1j * blocks[:, :, 3]
    errC = np.max(np.abs(gotC - C) / np.maximum(sC, 1e-300))
    errk = np.max(np.abs(gotk - k) / np.maximum(sk, 1e-300))
    print(f"{label}: largest block deviation / sum |term|: C {errC:.2e}  k {errk:.2e}")
    assert errC <= TOL and errk <= TOL, (label, errC, errk)


def _check_route(monkeypatch, make, pot, dt, nt, B, entry, setup=None, kw=None, moments=False):
    """run(blocks=...) on the route `setup` / `kw` select: the entry point named ran, slots (and moments) bit for bit as without
    blocks, sum_b blocks = slots, blocks against the step-path oracle"""
    kw = kw or {}
    runs = []
    for with_blocks in (True, False):
        prop = make()
        if setup:
            setup(prop)
        slots = torch.zeros((nt, 5), device=prop.device)
        mom = torch.zeros((nt, 6), device=prop.device) if moments else None
        blocks = torch.full((nt + 1, B, 4), 7.5, device=prop.device) if with_blocks else None
        seen = LibSpy(monkeypatch, {entry}).seen if with_blocks else {}
        prop.run(pot, dt, nt, slots=slots, moments=mom, blocks=blocks, **kw)
        prop.synchronize()
        monkeypatch.undo()
        if with_blocks:
            assert seen.get(entry, 0) > 0, f"{entry} was not called"
            assert torch.all(blocks[nt] == 7.5), "a row beyond nt was written"
        runs.append((slots.cpu().numpy(), None if mom is None else mom.cpu().numpy(), None if blocks is None else blocks.cpu().numpy()[:nt]))
    assert np.array_equal(runs[0][0][:, :4], runs[1][0][:, :4]), "C or k changed with blocks on"
    if moments:
        assert np.array_equal(runs[0][1], runs[1][1]), "the moments changed with blocks on"
    blocks = runs[0][2]
    want = _oracle(make(), pot, dt, nt, B)
    # the blocks add up to the slot row: within the same tolerance, relative to the sum of |term| over all blocks
    total, slots = blocks.sum(axis=1), runs[0][0]
    assert np.all(np.abs(total[:, 0] + 1j * total[:, 1] - (slots[:, 0] + 1j * slots[:, 1])) <= TOL * want[2].sum(axis=1))
    assert np.all(np.abs(total[:, 2] + 1j * total[:, 3] - (slots[:, 2] + 1j * slots[:, 3])) <= TOL * np.maximum(want[3].sum(axis=1), 1e-300))
    _assert_blocks(blocks, want, entry)
    return blocks


def _sampled(G, q0, n, seed=5, wm=None, p0=None):
    """factory of propagators with the same n device-sampled trajectories"""
    from semiclassical_amd import propagators as PR

    def make():
        prop = (PR.HermanKlukPropagator(G, G, device="cuda") if wm is None else
                PR.WaltonManolopoulosPropagator(G, G, wm[0], wm[1], device="cuda"))
        prop.initial_conditions(q0, torch.zeros_like(q0) if p0 is None else p0, G, ntraj=n, seed=seed)
        return prop
    return make


def _fixture_sampled(name, n):
    g = cases.load(name)
    from semiclassical_amd import propagators as PR
    Gi, Gt = cases.T(g["Gamma_i"]), cases.T(g["Gamma_t"])

    def make():
        prop = (PR.WaltonManolopoulosPropagator(Gi, Gt, float(g["alpha"]), float(g["beta"])) if "alpha" in g
                else PR.HermanKlukPropagator(Gi, Gt))
        prop.initial_conditions(cases.T(g["q0"]), cases.T(g["p0"]), cases.T(g["Gamma_0"]), ntraj=n, seed=5)
        return prop
    return make, engine_cases.engine_potential(g), float(g["dt"])


def _morse(D, seed):
    from semiclassical_amd import potentials as P
    rng = np.random.default_rng(seed)
    omega = torch.from_numpy(np.sort(rng.uniform(700, 2600, D)) / 219474.63)
    nac = torch.from_numpy(rng.normal(0, 1e-3, D))
    q0 = torch.from_numpy(rng.uniform(-0.3, 0.3, D) / np.sqrt(omega.numpy()))
    return P.MorsePotential(omega, torch.full((D,), 0.02), nac), torch.diag(omega), q0


# ------------------------------------------------------------------------------------------------ 1. whole loop, separable
@pytest.mark.parametrize("n,B,nt", [(203, 8, 6), (16503, 32, 4), (64, 8, 520)], ids=["ragged", "slots-wrap", "two-chunks"])
def test_whole_loop_separable(monkeypatch, n, B, nt):
    """D = 5: a ragged last group and idle rows; more trajectories than wavefront slots; more steps than one chunk of 512"""
    make, pot, dt = _fixture_sampled("hk_as5_chi002", n)
    _check_route(monkeypatch, make, pot, dt, nt, B, "sc_hk_run_blocks")
    _check_route(monkeypatch, make, pot, dt, min(nt, 6), B, "sc_hk_run_blocks", moments=True)


# ------------------------------------------------------------------------------------------------ 2. whole loop, dense Hessian
@pytest.mark.parametrize("nt,entry", [(20, "sc_hk_run_modal"), (4, "sc_hk_run")], ids=["normal-modes", "cartesian"])
def test_whole_loop_constant_dense_hessian(monkeypatch, nt, entry):
    from semiclassical_amd import potentials as P
    from tests.test_harmonic_modal_gpu import _random_case
    args, G, q0, p0 = _random_case(6, 0, False, 77)
    pot = P.MolecularHarmonicPotential.from_arrays(*args, origin=-0.3)
    make = _sampled(G, q0, 203, p0=p0)
    seen = LibSpy(monkeypatch, {entry}).seen
    probe = make()
    probe.run(pot, 4.0, nt, slots=torch.zeros((nt, 5), device=probe.device))
    probe.synchronize()
    monkeypatch.undo()
    assert seen.get(entry, 0) > 0, f"the run did not take {entry}"
    _check_route(monkeypatch, make, pot, 4.0, nt, 8, "sc_hk_run_blocks")


# ------------------------------------------------------------------------------------------------ 3. tiled fast path
def _no_pairs(prop):
    prop.pair_steps = False


@pytest.mark.parametrize("setup,kw,entry,also", [(None, {}, "sc_term_blocks", "sc_hk_step_multi"), (_no_pairs, {}, "sc_term_blocks", "sc_hk_step"),
                                                 (None, {"use_graph": True}, "sc_term_blocks_at", "sc_hk_step")],
                         ids=["pairs", "single", "graph"])
def test_tiled_fast_path(monkeypatch, setup, kw, entry, also):
    """D = 20 separable, five steps: two pairs and a single last step; one launch per step; the captured graph"""
    pot, G, q0 = _morse(20, 3)
    make = _sampled(G, q0, 203)
    seen = LibSpy(monkeypatch, {also}).seen
    probe = make()
    if setup:
        setup(probe)
    probe.run(pot, 2.0, 5, slots=torch.zeros((5, 5), device=probe.device), **kw)
    probe.synchronize()
    monkeypatch.undo()
    assert seen.get(also, 0) > 0 and probe._state.mono_layout == 1
    _check_route(monkeypatch, make, pot, 2.0, 5, 8, entry, setup=setup, kw=kw)
    _check_route(monkeypatch, make, pot, 2.0, 5, 8, entry, setup=setup, kw=kw, moments=True)


# ------------------------------------------------------------------------------------------------ 4. modal step
def test_modal_step(monkeypatch):
    from semiclassical_amd import potentials as P
    from tests.test_harmonic_modal_gpu import _random_case
    args, G, q0, p0 = _random_case(18, 6, False, 1180)
    pot = P.MolecularHarmonicPotential.from_arrays(*args, origin=-0.3)
    make = _sampled(G, q0, 100, p0=p0)
    probe = make()
    assert probe._pre.dprime == 12
    probe.run(pot, 4.0, 2, slots=torch.zeros((2, 5), device=probe.device))
    assert probe._modal_basis is not None, "run() did not take the normal-mode step"
    _check_route(monkeypatch, make, pot, 4.0, 4, 4, "sc_term_blocks")


# ------------------------------------------------------------------------------------------------ 5. dense-state path
def test_dense_state_path(monkeypatch):
    pot, G, q0 = _morse(65, 65)
    _check_route(monkeypatch, _sampled(G, q0, 64), pot, 2.0, 3, 2, "sc_term_blocks")


# ------------------------------------------------------------------------------------------------ 6. position-dependent couplings
def test_position_dependent_couplings(monkeypatch):
    from tests.test_generic_potential_gpu import QuarticWithVaryingCoupling
    rng = np.random.default_rng(33)
    D = 3
    omega = torch.from_numpy(np.sort(rng.uniform(700, 2600, D)) / 219474.63)
    masses = torch.from_numpy(rng.uniform(0.8, 1.6, D))
    pot = QuarticWithVaryingCoupling(omega, 2.0e-6, masses, torch.from_numpy(rng.normal(0, 1e-3, D)))
    make = _sampled(torch.diag(omega * masses), torch.from_numpy(rng.uniform(-6.0, 6.0, D)), 100)
    _check_route(monkeypatch, make, pot, 1.5, 4, 8, "sc_term_blocks")
    _check_route(monkeypatch, make, pot, 1.5, 4, 8, "sc_term_blocks", moments=True)
    probe = make()
    probe._remember_nac(pot)
    assert probe._nac_generic is not None


# ------------------------------------------------------------------------------------------------ 7. Walton-Manolopoulos
@pytest.mark.parametrize("fixture", ["wm_as5_chi002", "wm_as24"])
@pytest.mark.parametrize("moments", [False, True], ids=["plain", "moments"])
def test_walton_manolopoulos(monkeypatch, fixture, moments):
    """D = 5: the register kernel, D = 24: wm_kernel"""
    make, pot, dt = _fixture_sampled(fixture, 100)
    _check_route(monkeypatch, make, pot, dt, 4, 8, "sc_term_blocks", moments=moments)


# ------------------------------------------------------------------------------------------------ 8. no coupling known
def test_without_a_coupling_the_k_columns_are_zero():
    make, pot, dt = _fixture_sampled("hk_as5_chi002", 203)
    prop = make()
    prop.autocorrelation()                       # exports the C terms; no potential has been seen: no coupling
    assert prop._nac is None and prop._nac_generic is None
    out = torch.full((8, 4), 3.25, device=prop.device)
    prop._term_blocks(False, (out.data_ptr(), 8))
    prop.synchronize()
    got = out.cpu().numpy()
    assert np.all(got[:, 2:] == 0.0)
    sums, scale = _group(prop._cq.cpu().numpy(), np.arange(203), 8)
    assert np.all(np.abs(got[:, 0] + 1j * got[:, 1] - sums) <= TOL * scale)
    # twice the same bits
    again = torch.zeros((8, 4), device=prop.device)
    prop._term_blocks(False, (again.data_ptr(), 8))
    assert torch.equal(out, again)


# ------------------------------------------------------------------------------------------------ 9. bad arguments
def test_bad_arguments():
    from semiclassical_amd._lib import lib, ptr
    make, pot, dt = _fixture_sampled("hk_as5_chi002", 64)
    prop = make()
    dev = prop.device
    for B in (3, 128):
        with pytest.raises(ValueError, match="power of two"):
            prop.run(pot, dt, 2, slots=torch.zeros((2, 5), device=dev), blocks=torch.zeros((2, B, 4), device=dev))
        out = torch.zeros((B, 4), device=dev)
        assert lib.sc_term_blocks(ptr(prop._cq), None, 64, B, ptr(out), None) != 0
        assert lib.sc_hk_run_blocks(ptr(out), 64, 5, 1, B, ptr(out), None) != 0
    for bad in (torch.zeros((1, 8, 4), device=dev),                            # too short
                torch.zeros((2, 8, 8), device=dev)[:, :, :4],                  # not contiguous
                torch.zeros((2, 8, 4), device=dev, dtype=torch.float32), torch.zeros((2, 8, 4)), torch.zeros((2, 32), device=dev)):
        with pytest.raises(ValueError, match="blocks has to be a contiguous float64 tensor of shape"):
            prop.run(pot, dt, 2, slots=torch.zeros((2, 5), device=dev), blocks=bad)
    assert prop.t == 0.0


# ------------------------------------------------------------------------------------------------ 10. driver
def _as5_task(tmp_path, out, **extra):
    g = cases.load("hk_as5_chi002")
    model = tmp_path / "AS_model.dat"
    rows = np.vstack((g["omega"] * 219474.63, 0.5 * g["omega"] * g["q0"] ** 2 * np.sign(g["q0"]), g["nac"],
                      np.full(5, 0.02))).T
    np.savetxt(model, rows)
    task = {"task": "dynamics", "potential": {"type": "anharmonic AS", "model_file": str(model)},
            "propagator": "HK", "batch_size": 400, "num_trajectories": 1200, "num_steps": 20, "time_step_fs": 0.04,
            "results": {"correlations": str(out)}, "manual_seed": 5}
    task.update(extra)
    return task


TODAY = ["propagator", "times", "autocorrelation", "ic_correlation", "adiabatic_gap", "zero_point_energy", "trajectories"]


def test_driver_task_with_error_blocks(tmp_path):
    """"error_blocks": 8, three repetitions of 400 device-sampled trajectories, against ONE propagator over the same 1200 points
    regrouped on the host by the repetition-local index; then the rates task"""
    from semiclassical_amd import driver, hostmath, rates, units
    from semiclassical_amd.units import hbar
    B = 8
    out = tmp_path / "with.npz"
    task = _as5_task(tmp_path, out, error_blocks=B)
    driver.run_semiclassical_dynamics(task, device="cuda")
    got = dict(np.load(out))
    assert sorted(got) == sorted(TODAY + ["autocorrelation_blocks", "ic_correlation_blocks", "block_trajectories"])
    setup = driver.build_problem(task)
    zi, probi = [], []
    for rep in range(3):
        p = driver.make_propagator(task, setup.Gamma_0, "cuda")
        p.initial_conditions(setup.q0, setup.p0, setup.Gamma_0, ntraj=400, ntraj_total=400, seed=5, subsequence=rep, first_index=0)
        zi.append(p.zi.cpu())
        probi.append(p.probi.cpu())
    whole = driver.make_propagator(task, setup.Gamma_0, "cuda")
    whole.set_initial_conditions(setup.q0, setup.p0, setup.Gamma_0, torch.cat(zi, 1), torch.cat(probi))
    dt, nt = task["time_step_fs"] / units.autime_to_fs, task["num_steps"]
    C, k, sC, sk = _oracle(whole, setup.potential, dt, nt, B, local=np.arange(1200) % 400)
    phase = np.exp(1j / hbar * hostmath.time_grid(nt, dt) * setup.zero_point_energy)[:, None]
    assert np.array_equal(got["block_trajectories"], 3 * hostmath.block_counts(400, B))
    assert np.max(np.abs(got["autocorrelation_blocks"] - C * phase) / sC) <= TOL
    assert np.max(np.abs(got["ic_correlation_blocks"] - k * phase) / sk) <= TOL
    assert np.max(np.abs(got["autocorrelation_blocks"].sum(1) - got["autocorrelation"])) <= TOL * np.max(sC.sum(1))
    # rates: the error is rate_standard_error of the stored blocks, the rate itself is what it was
    rtask = {"task": "rates", "correlations": str(out), "rates": str(out), "hwhmG_ev": 0.05}
    driver.calculate_rates(rtask)
    r = np.load(out)
    lineshape, _ = driver.lineshape_from_task(rtask)
    e, sigma = rates.rate_standard_error(r["times"], r["ic_correlation_blocks"], r["block_trajectories"], lineshape)
    want = (2.0 * np.pi * sigma)[e >= 0.0]
    assert r["ic_rate_error"].shape == r["ic_rate"].shape and np.all(want > 0)
    assert np.max(np.abs(r["ic_rate_error"] - want) / want) <= TOL
    # without the key: today's keys, the same means and the same rate bit for bit
    plain = tmp_path / "plain.npz"
    driver.run_semiclassical_dynamics(_as5_task(tmp_path, plain), device="cuda")
    d = np.load(plain)
    assert sorted(d.files) == sorted(TODAY)
    assert np.array_equal(d["autocorrelation"], got["autocorrelation"]) and np.array_equal(d["ic_correlation"], got["ic_correlation"])
    driver.calculate_rates(dict(rtask, correlations=str(plain), rates=str(plain)))
    d = np.load(plain)
    assert "ic_rate_error" not in d.files and np.array_equal(d["ic_rate"], r["ic_rate"])


# ------------------------------------------------------------------------------------------------ 11. two ranks
def test_two_ranks_flush_blocks_and_counts_in_one_collective(tmp_path):
    from semiclassical_amd import distributed as D
    from semiclassical_amd import hostmath
    case, nt, B = "hk_as5_chi002", 6, 8
    g = cases.load(case)
    out = str(tmp_path / "blocks.npz")
    rc = D.launch_local_ranks([os.path.join(ROOT, "tests", "_rank_blocks.py"), case, str(nt), str(B), out], 2, timeout=600,
                              extra_env={"SC_DIST_BACKEND": "gloo", "SC_TEST_DEVICE": "0"})
    assert rc == 0, f"a rank process failed (largest exit code {rc})"
    r = np.load(out)
    assert int(r["world"]) == 2 and int(r["collectives"]) == 1
    n = g["zi"].shape[1]
    shards = [D.shard_slice(n, rank, 2) for rank in range(2)]
    local = np.concatenate([np.arange(s.stop - s.start) for s in shards])
    whole, pot = engine_cases.engine_propagator(g), engine_cases.engine_potential(g)
    want = _oracle(whole, pot, float(g["dt"]), nt, B, local=local)
    _assert_blocks(r["blocks"], want, "two ranks")
    assert np.array_equal(r["counts"], sum(hostmath.block_counts(s.stop - s.start, B) for s in shards))
    total = r["blocks"].sum(axis=1)
    assert np.all(np.abs(total - r["slots"][:, :4]) <= TOL * np.maximum(want[2].sum(1), want[3].sum(1))[:, None])
