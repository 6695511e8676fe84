"""Inputs and runs shared by tests/test_lin16_parent_bits_gpu.py and tools/record_lin16_parent_bits.py (the recorder of
tests/golden/lin16_parent_bits.npz): the two register kernels for a constant dense Hessian at D <= 16 (csrc/sc_hk_step_lin.hip,
csrc/sc_hk_run_lin.hip) before and after their shared pieces got one definition (csrc/sc_lin16.h).  Every
input comes from the integer hash of tests/lu_trim_inputs.py -- no library random numbers, no factorisation: rotations are products
of Householder reflectors.  The fixture holds outputs and digests only."""
import functools
import hashlib

import numpy as np

from tests import lu_trim_inputs as inp

# (D, d', diagonal widths): every instantiated shape of hk_step_lin_kernel, and (5, 5, diagonal), which has none and must still
# fall through to the general kernel (run_case asserts both: assert_step_dispatch, dispatch_probe)
STEP_SHAPES = ((12, 6, False), (12, 12, True), (9, 3, False), (9, 9, True), (6, 6, True), (6, 6, False), (3, 3, True),
               (6, 1, False), (9, 4, False), (12, 7, False), (15, 9, False), (15, 15, True), (5, 5, True))
# ... of hk_run_lin_kernel
RUN_SHAPES = tuple(s for s in STEP_SHAPES if s[0] not in (15, 5))
SIZES = (5, 203)                        # less than one workgroup pass; ragged
LARGE = 2 * 8192 + 37                   # every persistent workgroup gets several prefetched passes and a ragged last one
LARGE_SHAPES = ((12, 6, False), (12, 12, True))
NOISE = 0.4                             # monodromy blocks = identity + NOISE * noise: part of the fixed-order eliminations meet weak pivots
DT, NT, NSTEPS, E0 = 2.0, 5, 3, 0.01
VALUES_UP_TO = 1024                     # doubles; larger arrays are recorded as sha256 digests


def cases():
    return [(s, n) for s in STEP_SHAPES for n in SIZES] + [(s, LARGE) for s in LARGE_SHAPES]


def tag(shape, n):
    D, dp, diag = shape
    return f"D{D}_dp{dp}_{'diag' if diag else 'dense'}_n{n}"


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8).copy()


def _rotation(D, stream):
    """orthogonal to rounding: the product of two Householder reflectors of hashed vectors"""
    Q = np.eye(D)
    for k in range(2):
        u = inp.noise((D,), stream + k) + 0.1
        Q = Q @ (np.eye(D) - 2.0 * np.outer(u, u) / (u @ u))
    return Q


@functools.lru_cache(maxsize=4)
def model(shape):
    """(arguments of MolecularHarmonicPotential.from_arrays, origin, Gamma, q0) of a shape: symmetric Hessian, gradient and non-zero
    NAC vector, origin != 0; widths diagonal or rotated with D - d' zero modes"""
    D, dp, diag = shape
    s = 1000 * (100 * D + 2 * dp + diag)
    w = np.sort(500.0 + 2500.0 * inp.uniform((D,), s + 1)) / 219474.63
    masses = (0.8 + 0.7 * inp.uniform((D,), s + 2)) * 1822.0
    Q = _rotation(D, s + 10)
    hess = (Q * (w ** 2 * 1822.0)) @ Q.T
    hess = 0.5 * (hess + hess.T)
    if diag:
        G = np.diag(w * 1822.0)
    else:
        ww = w * 1822.0 * (0.7 + 0.7 * inp.uniform((D,), s + 3))
        ww[:D - dp] = 0.0
        Qg = _rotation(D, s + 20)
        G = (Qg * ww) @ Qg.T
        G = 0.5 * (G + G.T)
    pos0 = 0.05 * inp.noise((D,), s + 4)
    args = (pos0, -0.3, 1e-3 * inp.noise((D,), s + 5), hess, masses, 1e-3 * inp.noise((D,), s + 6))
    q0 = pos0 + 0.02 * inp.noise((D,), s + 7)
    return args, -0.3, G, q0, w


@functools.lru_cache(maxsize=2)
def state(shape, n):
    """(zi (2D, n), probi (n), y in the reference's layout with dense blocks identity + NOISE * noise and S = 0)"""
    D = shape[0]
    _, _, _, q0, w = model(shape)
    s = 1000 * (100 * D + 2 * shape[1] + shape[2]) + 100 + (7 if n == LARGE else n)
    scale = np.sqrt(w * 1822.0)[:, None]
    zi = np.concatenate((q0[:, None] + 0.3 * inp.noise((D, n), s + 1) / scale, 0.3 * inp.noise((D, n), s + 2) * scale))
    probi = 0.5 + inp.uniform((n,), s + 3)
    y = np.zeros((2 * D + 4 * D * D + 1, n))
    y[:2 * D] = zi
    eye = np.eye(D).reshape(D * D, 1)
    for k in range(4):
        blk = NOISE * inp.noise((D * D, n), s + 10 + k)
        y[2 * D + k * D * D: 2 * D + (k + 1) * D * D] = blk + eye if k in (0, 3) else blk
    return zi, probi, y


def engine(shape, n):
    """(HK propagator on cuda holding the state of (shape, n), the potential)"""
    import torch
    from semiclassical_amd import potentials as P, propagators as PR
    torch.set_default_dtype(torch.float64)
    args, origin, G, q0, _ = model(shape)
    zi, probi, y = state(shape, n)
    pot = P.MolecularHarmonicPotential.from_arrays(*args, origin=origin)
    G = torch.from_numpy(G)
    prop = PR.HermanKlukPropagator(G, G, device="cuda")
    prop.set_initial_conditions(torch.from_numpy(q0), torch.zeros(shape[0]), G, torch.from_numpy(zi), torch.from_numpy(probi))
    assert prop._pre.dprime == shape[1] and bool(prop._pre.diag) == shape[2], (shape, prop._pre.dprime, prop._pre.diag)
    prop.y = torch.from_numpy(y)
    return prop, pot


def host_constants(shape):
    """digest of what the host's linear algebra hands to the kernels: Phi(dt), the prefactor and overlap constants and, for dense
    widths of a whole-loop shape, the normal-mode constants.  Compared first: a difference here is the host's, not a kernel's"""
    prop, pot = engine(shape, SIZES[0])
    cpu = lambda t: t.detach().cpu().numpy()
    parts = [pot._step_matrix(DT)] + [cpu(b) for b in prop._pre_bufs] + [cpu(b) for b in prop._ovl_t0_bufs]
    if shape in RUN_SHAPES and not shape[2]:
        modal = prop._modal_constants(pot, prop._potential_descriptor(pot, DT), DT)
        assert modal is not None, shape
        parts += [cpu(c) for c in modal["consts"]] + [cpu(modal[k]) for k in ("phi", "A", "B", "Ainv", "Binv")]
    return digest(*parts)


def _held(a):
    a = np.ascontiguousarray(a)
    return a if a.size * (2 if np.iscomplexobj(a) else 1) <= VALUES_UP_TO else digest(a)


def _final(prop, key, out):
    import torch
    torch.cuda.synchronize()
    D = prop.dim
    for name, t in (("c2", prop._c2), ("sgn", prop._sgn), ("act", prop._act), ("qp", prop._qp)):
        out[f"{key}_{name}"] = _held(t.cpu().numpy())
    out[f"{key}_elog"] = prop._elog.cpu().numpy().copy()
    out[f"{key}_blocks_sha256"] = digest(prop.y[2 * D:2 * D + 4 * D * D].cpu().numpy())


def instantiated(shape):
    """hk_step_lin_kernel has the shape: all of STEP_SHAPES but (5, 5, diagonal)"""
    return shape[0] != 5


def prefactor_only(prop, desc):
    """the prefactor-only launch of sc_hk_step (mode 1) with the descriptor of the constant dense Hessian: the launch that reaches
    hk_step_lin_kernel.  (HermanKlukPropagator._prefactor_initial passes a separable null potential and never does.)"""
    import torch
    from semiclassical_amd import _lib
    from semiclassical_amd._lib import lib, check
    assert desc.kind == _lib.SC_POT_HARMONIC_DENSE
    check(lib.sc_hk_step(desc, prop._state, prop._hk, DT, 1, None, prop._stream()))
    torch.cuda.synchronize()
    return inp.flagged(prop)


def assert_step_dispatch(prop, desc):
    """what sc_hk_step asks before it hands a step to the register kernel, and what the launcher asks of the state: the descriptor of
    a constant dense Hessian with Phi built for DT, the flag array, real L and R, 16-byte aligned state arrays.  (The library exports
    no hook for the launcher's answer: dispatch_probe below observes it.)"""
    from semiclassical_amd import _lib
    assert desc.kind == _lib.SC_POT_HARMONIC_DENSE and desc.lin_prop and desc.lin_dt == DT
    assert prop._state.flags and (prop._pre.diag or prop._hk.real_lr)
    assert all(t.data_ptr() % 16 == 0 for t in (prop._mono, prop._qp, prop._act, prop._c2, prop._sgn))


def dispatch_probe(prop, desc, shape, n):
    """All four monodromy blocks zero: the prefactor matrix is zero, every leading pivot is zero, and a kernel that eliminates in a
    fixed order flags EVERY trajectory; the general kernel pivots fully and flags none.  The number flagged in a prefactor-only launch
    therefore says which kernel ran: n for the instantiated shapes, 0 for (5, 5, diagonal)."""
    import torch
    D = shape[0]
    y = state(shape, n)[2].copy()
    y[2 * D:2 * D + 4 * D * D] = 0.0
    prop.y = torch.from_numpy(y)
    flagged = prefactor_only(prop, desc)
    assert flagged == (n if instantiated(shape) else 0), (shape, n, flagged, "the step dispatcher took another kernel")
    return flagged


def run_case(shape, n):
    """every route of a case through the two kernels: {"{tag}_{route}_{what}": array}.  Routes: pref0 and pref1 (the prefactor-only
    launch of hk_step_lin_kernel, before and after Phi is attached to the descriptor: the first stages zeros in its place), step (NSTEPS
    step() calls), and for a whole-loop shape run() of NT steps with the product with Phi (runphi), in normal-mode coordinates
    (runmodal; dense widths) and each once more with second moments, which takes the _m kernels.  Also held: init, the engine's own
    prefactor at t = 0 (_prefactor_initial: a separable null potential, so the separable fast path or the general kernel, NOT the
    kernels under test -- it initialises the tracker here), and probe, the flagged count of dispatch_probe."""
    import torch
    t = tag(shape, n)
    out = {}
    prop, pot = engine(shape, n)
    prop._prefactor_initial()
    torch.cuda.synchronize()
    out[f"{t}_init_c2"], out[f"{t}_init_sgn"] = _held(prop._c2.cpu().numpy()), _held(prop._sgn.cpu().numpy())
    out[f"{t}_init_flagged"] = np.array([inp.flagged(prop)])
    desc0, desc1 = prop._potential_descriptor(pot), prop._potential_descriptor(pot, DT)
    assert not desc0.lin_prop and desc1.lin_prop
    for key, desc in (("pref0", desc0), ("pref1", desc1)):
        out[f"{t}_{key}_flagged"] = np.array([prefactor_only(prop, desc)])
        c2 = prop._c2.cpu().numpy()
        out[f"{t}_{key}_c2"] = _held(c2) if key == "pref0" else digest(c2)
        out[f"{t}_{key}_sgn"] = _held(prop._sgn.cpu().numpy())
    assert_step_dispatch(prop, desc1)
    fl = []
    for _ in range(NSTEPS):
        prop.step(pot, DT)
        torch.cuda.synchronize()
        fl.append(inp.flagged(prop))
    out[f"{t}_step_flagged"] = np.array(fl)
    if not instantiated(shape):
        assert sum(fl) == 0, (shape, fl, "the general kernel pivots fully and flags nothing")
    _final(prop, f"{t}_step", out)
    out[f"{t}_probe_flagged"] = np.array([dispatch_probe(prop, desc1, shape, n)])
    if shape not in RUN_SHAPES:
        return out
    for route, frm in (("runphi", 10 ** 9), ("runmodal", 1)):
        if route == "runmodal" and shape[2]:
            continue
        for mom in (False, True):
            prop, pot = engine(shape, n)
            prop._prefactor_initial()
            prop.normal_modes_from = frm
            assert prop._whole_loop_applies(prop._potential_descriptor(pot, DT)), (shape, "not taken by the whole-loop kernel")
            slots = torch.zeros((NT, 5), device="cuda")
            moments = torch.zeros((NT, 6), device="cuda") if mom else None
            prop.run(pot, DT, NT, E0, slots=slots, moments=moments)
            assert bool(prop.__dict__.get("_modal_cache")) == (route == "runmodal")
            key = f"{t}_{route}{'_m' if mom else ''}"
            _final(prop, key, out)
            out[f"{key}_slots"] = slots.cpu().numpy()
            if mom:
                out[f"{key}_moments"] = moments.cpu().numpy()
    return out
