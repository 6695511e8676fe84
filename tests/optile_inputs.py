"""Inputs and runs shared by tests/test_optile_parent_bits_gpu.py and its recorder (tools/record_optile_parent_bits.py ->
tests/golden/optile_parent_bits.npz): the tile and pre-pass kernels of the three operator families (sc_opcorr.hip, sc_opquad.hip,
sc_thermal_opcorr.hip) before and after their shared pieces got one definition in csrc/sc_optile.h.
Every input comes from rows5_inputs.HashRng -- no library random numbers, nothing stored; the fixture holds outputs only.

The rows (count, 5) are held in full.  The ket factors g (n, M) of the pre-pass kernels are 3.9 MB of doubles that do not
compress, the fixture stays below the 849 KB of rows5_parent_bits.npz: every g is held as the SHA-256 of its bytes (uint8 (32,)),
equal where every bit of g is equal, and the g that a pre-pass kernel returns is the g that the tile call of the same record reads."""
import hashlib

import numpy as np

from tests.rows5_inputs import HashRng

SIZES_N = (1, 64, 65, 130)             # one band, the band edge, two and three bands
DIMS = (1, 17)                         # one partial d-chunk, two chunks
KERNELS = ("opquad", "thermal", "opcorr_initial")

# (M, R_A): two operators per tile and one; 1 + R = 64 and 65 (the wide path with two tiles); two tile columns
OPQUAD_SHAPES = ((1, 0), (3, 2), (2, 31), (2, 32), (1, 63), (1, 64), (65, 1))
OPQUAD_RANKS_KET = (0, 3)
OPQUAD_VARIANTS = ("plain", "masked", "cursor")        # no mask; the first 64 trajectories discarded; row 2 of a 3-row NaN buffer

THERMAL_M = (1, 3, 64, 65)
THERMAL_MODES = {1: (1,), 17: (1, 16, 17)}             # d'' per D: one partial chunk, the chunk edge of the mode loop, two chunks
THERMAL_TIMES = (0.0, 0.9)
THERMAL_VARIANTS = ("plain", "masked")

OPCORR_INITIAL_N, OPCORR_INITIAL_M = (1, 130), (1, 65)


def digest(g):
    """the SHA-256 of the bytes of g, as uint8 (32,)"""
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(g).tobytes()).digest(), dtype=np.uint8).copy()


def opquad_rows(D):
    """{"opquad_D{D}_n{n}_M{M}_RA{RA}_RB{RB}_{g | variant}"}: the digest of g from sc_hk_opquad_initial and the rows (M, 5) of
    sc_hk_opquad on that g"""
    from tests import test_opquad_gpu as tq
    out = {}
    for n in SIZES_N:
        rng = HashRng(5000 + 100 * D + n)
        call = tq._Opquad(rng, n, D)
        kept = np.arange(n) >= 64
        for M, RA in OPQUAD_SHAPES:
            call.bra(call.operands(rng, M, RA, D, unit=RA == 0))
            for RB in OPQUAD_RANKS_KET:
                g = call.initial(call.operands(rng, M, RB, D, unit=RB == 0))
                assert g.shape == (n, M)
                tag = f"opquad_D{D}_n{n}_M{M}_RA{RA}_RB{RB}_"
                out[tag + "g"] = digest(g)
                out[tag + "plain"] = call(g)[0]
                out[tag + "masked"] = call(g, kept)[0]
                got = call(g, None, cursor=2, rows=3)
                assert np.isnan(got[:2]).all(), tag                  # the untouched rows are still NaN
                out[tag + "cursor"] = got[2]
    return out


def thermal_rows(D):
    """{"thermal_D{D}_dm{d''}_n{n}_M{M}_{g | t{t}_variant}"}: the digest of g from sc_hk_opcorr_thermal_initial and the rows (M, 5)
    of sc_hk_opcorr_thermal on that g"""
    from tests import test_thermal_opcorr_gpu as tt
    out = {}
    for dm in THERMAL_MODES[D]:
        for n in SIZES_N:
            rng = HashRng(9000 + 1000 * dm + 100 * D + n)
            call = tt._ThermalOpcorr(rng, n, D, dm)
            kept = np.arange(n) >= 64
            for M in THERMAL_M:
                bra, ket = call.operands(rng, M), call.operands(rng, M)
                g = call.initial(ket)
                assert g.shape == (n, M)
                tag = f"thermal_D{D}_dm{dm}_n{n}_M{M}_"
                out[tag + "g"] = digest(g)
                for t in THERMAL_TIMES:
                    out[tag + f"t{t}_plain"] = call(bra, g, t)
                    out[tag + f"t{t}_masked"] = call(bra, g, t, kept)
    return out


def opcorr_initial_rows(D):
    """{"opcorr_initial_D{D}_n{n}_M{M}_g"}: the digest of g from sc_hk_opcorr_initial (the rows of sc_hk_opcorr are those of
    rows5_parent_bits.npz)"""
    from tests import test_opcorr_gpu as to
    out = {}
    for n in OPCORR_INITIAL_N:
        rng = HashRng(30000 + 100 * D + n)
        call = to._Opcorr(rng, n, D)
        for M in OPCORR_INITIAL_M:
            g = call.initial(call.operands(rng, M, D))
            assert g.shape == (n, M)
            out[f"opcorr_initial_D{D}_n{n}_M{M}_g"] = digest(g)
    return out


TILE_ROWS = {"opquad": opquad_rows, "thermal": thermal_rows, "opcorr_initial": opcorr_initial_rows}


def tile_keys(kernel, D):
    """the keys and shapes of TILE_ROWS[kernel](D)"""
    keys = {}
    if kernel == "opquad":
        for n in SIZES_N:
            for M, RA in OPQUAD_SHAPES:
                for RB in OPQUAD_RANKS_KET:
                    tag = f"opquad_D{D}_n{n}_M{M}_RA{RA}_RB{RB}_"
                    keys[tag + "g"] = (32,)
                    keys.update({tag + v: (M, 5) for v in OPQUAD_VARIANTS})
    elif kernel == "thermal":
        for dm in THERMAL_MODES[D]:
            for n in SIZES_N:
                for M in THERMAL_M:
                    tag = f"thermal_D{D}_dm{dm}_n{n}_M{M}_"
                    keys[tag + "g"] = (32,)
                    keys.update({tag + f"t{t}_{v}": (M, 5) for t in THERMAL_TIMES for v in THERMAL_VARIANTS})
    else:
        keys = {f"opcorr_initial_D{D}_n{n}_M{M}_g": (32,) for n in OPCORR_INITIAL_N for M in OPCORR_INITIAL_M}
    return keys


# ---- run(): the launch orchestration of both families, in the style of rows5_inputs.run_rows ----
RUN_CASE, RUN_NT, RUN_BLOCKS, RUN_M, RUN_KT = "hk_as33", 5, 4, 3, 0.005
RUNS = ("quadratic", "thermal")


def _run_operators(D, with_k):
    rng = HashRng(41)
    bra, ket = ((rng.normal(size=RUN_M), rng.normal(size=(RUN_M, D))) for _ in range(2))
    if with_k:                                   # a K on the bra only: symmetric, full rank
        A = 0.2 * rng.normal(size=(RUN_M, D, D))
        bra = bra + (A + A.transpose(0, 2, 1),)
    return bra, ket


def run_rows(kind):
    """the raw buffers of run() on hk_as33, five steps in one call, with moments and B = 4 blocks.  "quadratic":
    run(operators=...) with a K on the bra only, visits of three steps.  "thermal": a thermal ensemble of the fixture's size drawn on
    the device (thermal_initial_conditions(..., seed=)), run(thermal_operators=...) in pairs of steps."""
    import torch
    from semiclassical_amd import propagators as PR
    from tests import cases
    from tests.engine_cases import engine_potential, engine_propagator
    g = cases.load(RUN_CASE)
    pot = engine_potential(g)
    if kind == "quadratic":
        prop = engine_propagator(g)
        attrs, arg, buf = {"visit_steps": 3, "visit_min_bytes": 0}, "operators", "opcorr"
    else:
        prop = PR.HermanKlukPropagator(cases.T(g["Gamma_i"]), cases.T(g["Gamma_t"]), device="cuda")
        q0 = cases.T(g["q0"])
        prop.thermal_initial_conditions(q0, torch.zeros_like(q0), cases.T(g["Gamma_0"]), pot.masses().to(torch.float64), RUN_KT,
                                        ntraj=int(g["zi"].shape[1]), seed=3)
        attrs, arg, buf = {"visit_steps": 2, "visit_min_bytes": 0}, "thermal_operators", "thermal_opcorr"
    for key, value in attrs.items():
        setattr(prop, key, value)
    dt, E0, nt, dev = float(g["dt"]), float(g["E0"]), RUN_NT, prop.device
    bufs = {"slots": torch.zeros((nt, 5), device=dev), "moments": torch.zeros((nt, 6), device=dev),
            "blocks": torch.zeros((nt, RUN_BLOCKS, 4), device=dev), buf: torch.full((nt, RUN_M, 5), np.nan, device=dev)}
    prop.run(pot, dt, nt, E0, **{arg: _run_operators(prop.dim, kind == "quadratic")}, **bufs)
    prop.synchronize()
    out = {k: t.cpu().numpy() for k, t in bufs.items()}
    out["slots"] = out["slots"][:, :4].copy()                    # column 4 belongs to the engine
    return {f"run_{kind}_{k}": v for k, v in out.items()}
