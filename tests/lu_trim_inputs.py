"""Inputs and runs shared by tests/test_lu_trim_gpu.py and tools/record_lu_parent_bits.py (the recorder of
tests/golden/lu_parent_bits.npz): dense monodromy blocks for the register elimination of the separable fast path
(csrc/sc_hk_lu.h), from an integer hash -- no library random numbers, the same bits on every machine."""
import hashlib

import numpy as np

DIMS = (17, 20, 33, 48, 60, 64)       # 1, 4 and 12 rows in the last diagonal block; full last blocks at 48 and 64
NTRAJ = 64
NOISE = 0.3                            # blocks = identity + NOISE * noise (unit variance)
DT = 4.0
NSTEPS = 3

_MASK = np.uint64(0xFFFFFFFFFFFFFFFF)


def _mix(x):
    """splitmix64 finaliser on uint64 arrays (wrap-around arithmetic)"""
    with np.errstate(over="ignore"):
        x = (x + np.uint64(0x9E3779B97F4A7C15)) & _MASK
        x = ((x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & _MASK
        x = ((x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & _MASK
        return x ^ (x >> np.uint64(31))


def uniform(shape, stream):
    """[0, 1) from the hash of (stream, element index): 53 bits"""
    n = int(np.prod(shape))
    with np.errstate(over="ignore"):
        idx = np.arange(n, dtype=np.uint64) + np.uint64(stream) * np.uint64(0x100000001B3)
    return ((_mix(_mix(idx)) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)).reshape(shape)


def noise(shape, stream):
    """zero mean, unit variance, bounded: sum of four uniforms"""
    s = sum(uniform(shape, 4 * stream + k) for k in range(4))
    return (s - 2.0) * np.sqrt(3.0)


def reference_state(D, n, stream=0, amplitude=NOISE):
    """(q0, omega-model, y): y in the reference's layout (2D + 4 D^2 + 1, n) with dense blocks identity + amplitude * noise and
    phase-space points scattered around q0; trajectory index fastest"""
    import bench
    omega, chi, nac, q0, _ = bench.as60_model(D)
    om = omega.numpy()
    y = np.zeros((2 * D + 4 * D * D + 1, n))
    y[:D] = q0.numpy()[:, None] + 0.1 * noise((D, n), 100 * stream + 1) / np.sqrt(om)[:, None]
    y[D:2 * D] = 0.1 * noise((D, n), 100 * stream + 2) * np.sqrt(om)[:, None]
    eye = np.eye(D).reshape(D * D, 1)
    for k in range(4):
        blk = amplitude * noise((D * D, n), 100 * stream + 10 + k)
        if k in (0, 3):
            blk = blk + eye
        y[2 * D + k * D * D: 2 * D + (k + 1) * D * D] = blk
    return (omega, chi, nac, q0), y


def engine(D, y):
    """HK propagator on cuda holding the state y (prefactor of that state computed: the prefactor-only launch), and the potential"""
    import torch
    from semiclassical_amd import potentials as P, propagators as PR
    torch.set_default_dtype(torch.float64)
    import bench
    omega, chi, nac, q0, _ = bench.as60_model(D)
    G = torch.diag(omega)
    n = y.shape[1]
    prop = PR.HermanKlukPropagator(G, G, device="cuda")
    prop.set_initial_conditions(q0, 0.0 * q0, G, torch.from_numpy(y[:2 * D].copy()), torch.ones(n))
    prop.y = torch.from_numpy(y)
    prop._prefactor_initial()
    torch.cuda.synchronize()
    return prop, P.MorsePotential(omega, chi.clone(), nac)


def oracle_c2(D, y):
    """determinants of the CPU oracle for the state y"""
    import torch
    import bench
    from oracle import sc_oracle as orc
    torch.set_default_dtype(torch.float64)
    omega, chi, nac, q0, _ = bench.as60_model(D)
    G = torch.diag(omega)
    ref = orc.HKOracle(G, G)
    ref.set_initial_conditions(q0, 0.0 * q0, G, torch.from_numpy(y[:2 * D].copy()), torch.ones(y.shape[1]))
    ref.y = torch.from_numpy(y.copy())
    ref._prefactor()
    return ref.c2.numpy()


def flagged(prop):
    """trajectories the register elimination handed to the fully pivoted kernel in the last launch"""
    return int(prop._flags[-2].item())


def run_paths(D, n=NTRAJ):
    """both paths through the register elimination for the dense state of dimension D: the prefactor-only launch and NSTEPS
    sc_hk_step calls with the AS model.  Outputs only (what the fixture holds)."""
    import torch
    _, y = reference_state(D, n)
    prop, pot = engine(D, y)
    out = {"pre_c2": prop._c2.cpu().numpy().copy(), "pre_sgn": prop._sgn.cpu().numpy().copy(),
           "pre_flagged": np.array([flagged(prop)])}
    fl = []
    for _ in range(NSTEPS):
        prop.step(pot, DT)
        torch.cuda.synchronize()
        fl.append(flagged(prop))
    out["step_c2"] = prop._c2.cpu().numpy().copy()
    out["step_sgn"] = prop._sgn.cpu().numpy().copy()
    out["step_flagged"] = np.array(fl)
    blocks = prop.y[2 * D:2 * D + 4 * D * D].cpu().numpy()
    out["blocks_sha256"] = np.frombuffer(hashlib.sha256(np.ascontiguousarray(blocks).tobytes()).digest(), dtype=np.uint8).copy()
    return out
