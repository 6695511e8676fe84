"""Inputs and runs shared by tests/test_rows5_parent_bits_gpu.py, tests/test_store_rows5_host.py and their recorders
(tools/record_rows5_parent_bits.py -> tests/golden/rows5_parent_bits.npz, tools/record_store_rows5_parent.py ->
tests/golden/store_rows5_parent.npz): the five-sum rows of targets and operators before and after they
got one definition.  Every input comes from the integer hash of tests/lu_trim_inputs.py -- no library random numbers, nothing
stored; the fixtures hold outputs only."""
import numpy as np

from tests import lu_trim_inputs as inp

# ---- the tile kernels through the C ABI: the smallest shapes at which the shared tail and the reduction can go wrong ----
SIZES_N = (1, 63, 64, 65, 130)         # one band, the band edge, two and three bands
SIZES_COUNT = (1, 3, 64, 65, 130)      # the kv edge, two and three tile columns
DIMS = (1, 17)                         # one partial d-chunk, two chunks
KERNELS = ("cross_diag", "cross_dense", "opcorr")
VARIANTS = ("plain", "masked", "cursor")       # no mask; the first 64 trajectories discarded; row 2 of a 3-row NaN buffer


class HashRng(object):
    """the few methods of numpy's Generator that the helpers of the GPU tests call, on the integer hash: every call is a stream"""

    def __init__(self, stream):
        self.stream = 1000 * stream

    def _next(self):
        self.stream += 1
        return self.stream

    @staticmethod
    def _shape(size):
        return () if size is None else tuple(np.atleast_1d(size))

    def normal(self, loc=0.0, scale=1.0, size=None):
        return loc + scale * inp.noise(self._shape(size), self._next())

    def uniform(self, low=0.0, high=1.0, size=None):
        return low + (high - low) * inp.uniform(self._shape(size), self._next())

    def choice(self, values, size=None):
        values = np.asarray(values)
        return values[(inp.uniform(self._shape(size), self._next()) * len(values)).astype(np.int64)]


def _grid(a, bits):
    """rounded to multiples of 2^-bits: the host's matrix products of such operands (_Cross forms the target rows with them) are
    exact, the same bits whatever the order of their sums"""
    return np.round(a * 2.0 ** bits) / 2.0 ** bits


def _cross_call(rng, n, D, diag):
    """tests.test_cross_gpu._Cross on a synthetic state, with the constants of the overlap replaced by hash values: the kernels
    take any La, Lb, C and fac, and nothing a factorisation returns reaches the device"""
    from tests import test_cross_gpu as tc
    import torch
    Gt, G0 = tc._widths(rng, D, True)
    call = tc._Cross(tc._synthetic(rng, n, D), Gt, G0, diag, mc_norm=float(n) * 1.7)
    off = lambda: 0.0 if diag else 0.3 / D * rng.uniform(-1.0, 1.0, (D, D))
    mats = [_grid(np.diag(rng.uniform(0.6, 1.8, D)) + off(), 6) for _ in range(3)]
    if not diag:
        mats[0], mats[1] = 0.5 * (mats[0] + mats[0].T), 0.5 * (mats[1] + mats[1].T)      # La and Lb are symmetric
    call.La, call.Lb, call.C = mats
    call.fac = 0.75
    dev = lambda a: torch.from_numpy(np.array(a, dtype=np.float64, order="C")).to("cuda")
    call.consts = [dev(np.diag(m)) for m in mats] if diag else [dev(mats[0]), dev(mats[1]), dev(mats[2].T)]
    return call


def tile_rows(kernel, D):
    """{"{kernel}_D{D}_n{n}_c{count}_{variant}": rows (count, 5)} of every shape and variant; the helpers of the GPU tests assert
    that the cursor is not advanced, the rows the cursor leaves alone are checked here"""
    from tests import test_opcorr_gpu as to
    out = {}
    for n in SIZES_N:
        rng = HashRng(100 * D + n)
        kept = np.arange(n) >= 64
        call = to._Opcorr(rng, n, D) if kernel == "opcorr" else _cross_call(rng, n, D, kernel == "cross_diag")
        for count in SIZES_COUNT:
            if kernel == "opcorr":
                args = (call.operands(rng, count, D), rng.normal(size=(n, count)) + 1j * rng.normal(size=(n, count)))
            else:
                s = 1.0 / np.sqrt(D)
                args = (_grid(rng.normal(0.0, 0.6 * s, (count, D)), 12), _grid(rng.normal(0.0, 0.9 * s, (count, D)), 12))
            tag = f"{kernel}_D{D}_n{n}_c{count}_"
            out[tag + "plain"] = call(*args)[0]
            out[tag + "masked"] = call(*args, kept)[0]
            got = call(*args, None, cursor=2, rows=3)
            assert np.isnan(got[:2]).all(), tag                  # the untouched rows are still NaN
            out[tag + "cursor"] = got[2]
    return out


# ---- run(): the launch orchestration, unmasked in one call and masked in two ----
RUN_CASE, RUN_NT, RUN_BLOCKS = "hk_as33", 5, 4


def _run_inputs(g, D):
    rng = HashRng(7)
    q0, p0 = np.asarray(g["q0"], dtype=np.float64), np.asarray(g["p0"], dtype=np.float64)
    targets = (q0 + 0.05 * rng.normal(size=(2, D)), p0 + 0.05 * rng.normal(size=(2, D)))
    operators = tuple((rng.normal(size=3), rng.normal(size=(3, D))) for _ in range(2))
    return targets, operators


def run_rows(masked):
    """the raw buffers of run(targets=..., operators=...) on hk_as33 with moments and B = 4 blocks.  Unmasked: visits of three
    steps, one call of five.  Masked: single steps, a call of two, discard_nonsymplectic at the median deviation, a call of
    three."""
    import torch
    from tests import cases
    from tests.engine_cases import engine_potential, engine_propagator
    g = cases.load(RUN_CASE)
    pot, prop = engine_potential(g), engine_propagator(g)
    attrs = {"pair_steps": False} if masked else {"visit_steps": 3, "visit_min_bytes": 0}
    for key, value in attrs.items():
        setattr(prop, key, value)
    dt, E0, nt, dev = float(g["dt"]), float(g["E0"]), RUN_NT, prop.device
    targets, operators = _run_inputs(g, prop.dim)
    bufs = dict(slots=torch.zeros((nt, 5), device=dev), moments=torch.zeros((nt, 6), device=dev),
                blocks=torch.zeros((nt, RUN_BLOCKS, 4), device=dev), cross=torch.full((nt, 2, 5), np.nan, device=dev),
                opcorr=torch.full((nt, 3, 5), np.nan, device=dev))
    piece = lambda a, b: prop.run(pot, dt, b - a, E0, targets=targets, operators=operators, **{k: t[a:b] for k, t in bufs.items()})
    out = {}
    if masked:
        piece(0, 2)
        tol = float(np.median(prop.symplectic_deviation().cpu().numpy()))
        prop.discard_nonsymplectic(tol)
        out["kept"] = prop.kept.cpu().numpy().astype(np.uint8)
        piece(2, nt)
    else:
        piece(0, nt)
    prop.synchronize()
    out.update({k: t.cpu().numpy() for k, t in bufs.items()})
    out["slots"] = out["slots"][:, :4].copy()                    # column 4 belongs to the engine
    tag = "run_masked_" if masked else "run_"
    return {tag + k: v for k, v in out.items()}


# ---- CorrelationStore.add_batch: a scripted sequence on hash-seeded host arrays ----
STORE_NT, STORE_K, STORE_M, STORE_D = 4, 2, 3, 3


def store_batches():
    """the keyword arguments of four add_batch calls: both families with second moments; the same, pooled; without second moments
    (the error keys drop, with a warning); with blocks and a symplecticity record"""
    nt, K, M, D = STORE_NT, STORE_K, STORE_M, STORE_D
    ids = HashRng(11)
    q, p = ids.normal(size=(K, D)), ids.normal(size=(K, D))
    ops = {key: ids.normal(size=(M,) if key.endswith("_c") else (M, D)) for key in ("bra_c", "bra_m", "ket_c", "ket_m")}
    cplx = lambda rng, shape: 0.5 * (rng.normal(size=shape) + 1j * rng.normal(size=shape))
    batches = []
    for b, ntraj in enumerate((100, 60, 40, 50)):
        rng = HashRng(20 + b)
        C = cplx(rng, (nt,))
        C[0] = 1.0
        kw = dict(autocorrelation=C, ic_correlation=cplx(rng, (nt,)), ntraj=ntraj,
                  cross={"q": q, "p": p, "correlation": cplx(rng, (nt, K))},
                  operators=dict(ops, correlation=cplx(rng, (nt, M))))
        if b != 2:                   # per-sample second moments: (S_rr, S_ii) above the squares of any mean drawn here
            moment = lambda shape: np.concatenate((rng.uniform(20.0, 30.0, shape + (2,)), rng.uniform(-1.0, 1.0, shape + (1,))),
                                                  axis=-1)
            kw["second_moments"] = (moment((nt,)), moment((nt,)))
            kw["cross"]["second_moment"] = moment((nt, K))
            kw["operators"]["second_moment"] = moment((nt, M))
        if b == 3:
            kw["blocks"] = (cplx(rng, (nt, 2)), cplx(rng, (nt, 2)), np.array([ntraj // 2, ntraj - ntraj // 2]))
            kw["symplecticity"] = {"steps": np.array([0, 2]), "max": rng.uniform(0.0, 1e-9, (2,)),
                                   "mean": rng.uniform(0.0, 1e-10, (2,)),
                                   "exceeding": np.array([0, 1]), "tolerance": 1e-9}
        batches.append(kw)
    return batches


class _Setup(object):
    adiabatic_gap, zero_point_energy = 0.1, 0.02


def store_times():
    import torch
    return torch.linspace(0.0, 3.0, STORE_NT, dtype=torch.float64)


def replay_store(path):
    """a fresh file at `path`, then the four batches: (the CorrelationStore, {"after{b}_{key}": array} of the file after batch b)"""
    from semiclassical_amd import driver
    store = driver.CorrelationStore(path)
    store.start({"results": {"overwrite": True}}, "HK", store_times(), _Setup())
    held = {}
    for b, kw in enumerate(store_batches()):
        store.add_batch(kw.pop("autocorrelation"), kw.pop("ic_correlation"), kw.pop("ntraj"), **kw)
        held.update({f"after{b}_{key}": val for key, val in np.load(path).items()})
    return store, held
