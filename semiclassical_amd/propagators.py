"""Semiclassical propagators on MI355X.

Host-side mirror of the reference's propagator interface
(semiclassical/propagators.py: ``HermanKlukPropagator`` :407, same method
names, argument meaning and error behaviour) over the HIP kernels of
``libsemiclassical_hip.so``.  Python only prepares O(D^2) constants and issues
kernel launches; all per-trajectory arithmetic runs on the GPU.

Differences a caller can observe:
  * the state lives in an engine-native, trajectory-major layout; the
    reference's ``(rows, n)`` tensor is produced on demand by the ``y``
    property (and accepted by its setter);
  * ``step()`` does not synchronise: the energy-conservation guard
    (reference propagators.py:385-398) is evaluated on the device and raised,
    with the reference's message, at the next host synchronisation point
    (``autocorrelation()``, ``ic_correlation()``, ``synchronize()``, ``run()``);
  * ``run()`` executes the caller loop of cli.py:401-436 (correlate,
    correlate, step -- nt times) without any host synchronisation.
"""
import collections
import logging

import numpy as np
import torch

from . import _lib, hostmath
from ._lib import (lib, check, ptr, sc_state, sc_hk_consts, sc_overlap_consts, sc_nac_consts, sc_wm_consts,
                   sc_dense_scratch, sc_multi_scratch)
from .units import hbar

__all__ = ['HermanKlukPropagator', 'WaltonManolopoulosPropagator', 'TimeAverageAccumulator']

logger = logging.getLogger(__name__)

C128 = torch.complex128
F64 = torch.float64


def _potential_fingerprint(potential):
    """Identity of the constants a potential contributes to the cached device buffers (1/m, coupling vectors).

    Caches are keyed on the object itself (a strong reference, compared with ``is``: a recycled ``id`` cannot alias a
    dead potential) AND on this cheap content fingerprint, so that masses or coupling vectors changed in place are
    picked up at the next step / run entry.  O(D) host work per call.

    The derivative couplings are probed at TWO points.  The reference evaluates them at the initial and the current
    position of every trajectory (propagators.py:880-892, 1685-1693); all of its own potentials return constant vectors,
    which the kernels take as constants.  A potential whose couplings differ between the probes is position dependent:
    the last entry of the fingerprint says so and the propagators evaluate its couplings per trajectory.
    """
    d = potential.dimensions()
    probe = torch.zeros((d, 1), dtype=F64)
    other = (0.05 + 0.1 * torch.arange(1, d + 1, dtype=F64) / d).reshape(d, 1)
    masses = hostmath.as_f64(potential.masses())
    tau1 = hostmath.as_f64(potential.derivative_coupling_1st(probe))[:, 0]
    tau2 = hostmath.as_f64(potential.derivative_coupling_2nd(probe))[:, 0]
    tau1b = hostmath.as_f64(potential.derivative_coupling_1st(other))[:, 0]
    tau2b = hostmath.as_f64(potential.derivative_coupling_2nd(other))[:, 0]
    varies = not (torch.equal(tau1, tau1b) and torch.equal(tau2, tau2b))
    return masses, tau1, tau2, torch.tensor([float(varies)], dtype=F64)


def _same_fingerprint(a, b):
    return a is not None and b is not None and all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b))


def _resolve_device(device):
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise RuntimeError(
            f"semiclassical_amd propagators run on an AMD GPU (device='cuda[:i]'), got device='{device}'. "
            "There is no CPU path.")
    if dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    return dev


# One step's row of run()'s output buffers as the launches take it: the addresses of its slot, of its moments, blocks = (address, B)
# and of its five-sum rows cross and opcorr, None where there is no such buffer.  slots[k] is the slot as a
# tensor, formed only where torch adds the k_ic sum to it (position-dependent couplings).
_Row = collections.namedtuple("_Row", "slot moments blocks cross slots k opcorr", defaults=(None,))

# The two families of five-sum rows as run() and _launch_correlate treat them.  arg: the argument of run(); field: its buffer
# argument and the field of _Row; letter: the count and its key in the prepared dict; what: the launch in messages; prepare: the
# method that validates the caller's argument into the prepared dict; launch: the method that fills a row from it; needs_terms:
# the launch reads the per-trajectory terms, which the correlate kernel then has to export; row: the field of _Row and the buffer
# keyword of _StepRows where they differ from `field` -- the thermal operators travel in the opcorr
# field: a state has a thermal ensemble or it has none, the two operator families never share a row.
_RowFamily = collections.namedtuple("_RowFamily", "arg field letter what prepare launch needs_terms row", defaults=(None,))
_ROW_FAMILIES = (
    _RowFamily("targets", "cross", "K", "cross-correlation", "_prepare_targets", "_launch_cross", False),
    _RowFamily("operators", "opcorr", "M", "operator-correlation", "_prepare_operators", "_launch_opcorr", True),
    _RowFamily("thermal_operators", "thermal_opcorr", "M", "thermal operator-correlation", "_prepare_thermal_operators",
               "_launch_thermal_opcorr", True, "opcorr"),
)
_OPERATOR_ROWS, _THERMAL_OPERATOR_ROWS = _ROW_FAMILIES[1], _ROW_FAMILIES[2]
# The hook of a time-average accumulator in the same place: a terms launch after every correlate launch.
# It fills no row (field None) and is not an argument family of run(): its "prepared dict" is the accumulator itself.
_TIME_AVERAGE = _RowFamily("time_average", None, None, "time-average terms", None, "_launch_ta_terms", False)
# The thermal correlation functions with quadratic operators: a row family of run() like those above, kept
# outside _ROW_FAMILIES, whose names are pinned.  Its rows travel in the opcorr field as the thermal operators' do: one call takes
# one of the two.
_THERMAL_QUADRATIC_ROWS = _RowFamily("thermal_quadratic", "thermal_opquad", "M", "thermal quadratic-correlation",
                                     "_prepare_thermal_quadratic", "_launch_thermal_opquad", True, "opcorr")
_RUN_ROW_FAMILIES = _ROW_FAMILIES + (_THERMAL_QUADRATIC_ROWS,)


class _StepRows(object):
    """The per-step output buffers of run(): what a row of each holds, how far apart the rows lie, where row k is.  The kernels write
    exactly these doubles at base + stride k for k < nt: anything that is not that buffer is refused.  Reads no propagator state."""
    #   buffer     a row, in doubles      bytes from row to row
    #   slots      SLOT = 5               40
    #   moments    MOMENT = 6             48
    #   blocks     (B, BLOCK = 4)         32 B
    #   cross      (K, CROSS = 5)         40 K
    #   opcorr     (M, OPCORR = 5)        40 M
    SLOT, MOMENT, BLOCK, CROSS, OPCORR = 5, 6, 4, 5, 5

    def __init__(self, device, nt, slots, moments=None, blocks=None, cross=None, K=None, *, opcorr=None, M=None):
        device = torch.device(device)
        self._check("slots", slots, nt, (self.SLOT,), device)
        if moments is not None:
            self._check("moments", moments, nt, (self.MOMENT,), device)
        if blocks is not None:
            self._check("blocks", blocks, nt, ("B", self.BLOCK), device)
            if not hostmath.valid_error_blocks(int(blocks.shape[1])):
                raise ValueError(f"the number of blocks has to be a power of two in 2 ... 64, got {int(blocks.shape[1])}")
        for name, t, count, width in (("cross", cross, K, self.CROSS), ("opcorr", opcorr, M, self.OPCORR)):
            if t is not None:
                self._check(name, t, nt, (count, width), device)
        self.slots, self.moments = slots, moments
        self.B, self.K, self.M = (None if t is None else int(t.shape[1]) for t in (blocks, cross, opcorr))
        # per buffer: (address of row 0, bytes from row to row), None where there is none
        given = (("slot", slots, self.SLOT, 1), ("moments", moments, self.MOMENT, 1), ("blocks", blocks, self.BLOCK, self.B),
                 ("cross", cross, self.CROSS, self.K), ("opcorr", opcorr, self.OPCORR, self.M))
        self._base = {name: None if t is None else (t.data_ptr(), 8 * width * count) for name, t, width, count in given}

    @staticmethod
    def _check(name, t, nt, row, device):           # row: the trailing shape ("B": any size)
        if not (isinstance(t, torch.Tensor) and t.dtype == F64 and t.dim() == 1 + len(row) and t.shape[0] >= nt
                and all(w == "B" or w == have for w, have in zip(row, t.shape[1:])) and t.is_contiguous() and t.device == device):
            raise ValueError(f"{name} has to be a contiguous float64 tensor of shape (>= {nt}, {', '.join(map(str, row))}) on {device}, "
                             f"got {getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))} on {getattr(t, 'device', '?')}")

    def row(self, k):
        """row k.  Row 0 is also the base the cursor routes take, row k0 the start of the piece a whole-loop launch fills from k0 on"""
        at = {name: None if base is None else base[0] + base[1] * k for name, base in self._base.items()}
        return _Row(at["slot"], at["moments"], None if at["blocks"] is None else (at["blocks"], self.B), at["cross"], self.slots, k,
                    at["opcorr"])

    @staticmethod
    def single(slot=None, moments=None, cross=None, opcorr=None):
        """the row of buffers that hold one row each: scratch of the caller's own, of any shape, not validated"""
        at = lambda t: None if t is None else t.data_ptr()
        return _Row(at(slot), at(moments), None, at(cross), None if slot is None else slot.view(1, -1), 0, at(opcorr))


class HermanKlukPropagator(object):
    """Herman-Kluk frozen-Gaussian propagator (reference propagators.py:407-1066)."""

    def __init__(self, Gamma_i, Gamma_t, device='cuda', exploit_separability=False):
        """``exploit_separability`` (not in the reference): opt in to the O(D) diagonal-state kernel whenever the
        potential is separable, the width matrices are diagonal and the monodromy matrices are still the diagonal
        ones ``initial_conditions`` created -- the dense blocks the reference carries are then never formed on the
        device unless ``y`` / ``monodromy_matrices()`` ask for them ("separable shortcut")."""
        self.exploit_separability = bool(exploit_separability)
        Gamma_i, Gamma_t = hostmath.as_f64(Gamma_i), hostmath.as_f64(Gamma_t)
        assert hostmath.is_symmetric_non_negative(Gamma_i), "Gamma_i has to be symmetric and positive semi-definite."
        assert hostmath.is_symmetric_non_negative(Gamma_t), "Gamma_t has to be symmetric and positive semi-definite."
        self.device = _resolve_device(device)
        self._Gi, self._Gt = Gamma_i, Gamma_t                 # host copies (setup algebra)
        self.Gamma_i, self.Gamma_t = Gamma_i.to(self.device), Gamma_t.to(self.device)
        self.sqGi, self.isqGi = hostmath.sym_sqrtm(Gamma_i)
        self.sqGt, self.isqGt = hostmath.sym_sqrtm(Gamma_t)
        self._nac, self._nac_pot, self._nac_fp, self._nac_generic = None, None, None, None
        self._ntraj_norm = None
        self._thermal = None

    # ------------------------------------------------------------------ initial conditions
    def initial_conditions(self, q0, p0, Gamma_0, ntraj=5000, ntraj_total=None, generator=None, seed=None, subsequence=0,
                           first_index=0):
        """Sample ``ntraj`` phase-space points from |<qi,pi,Gamma_i|q0,p0,Gamma_0>|^2 and reset the state.

        Two sources of the standard-normal deviates xi (reference propagators.py:537-539):

        * default / ``generator``: drawn on the HOST with the call the reference makes, so on a given torch build
          ``torch.manual_seed(s)`` reproduces the reference's CPU initial conditions (parity fixtures are made this way);
        * ``seed`` (an integer): drawn ON THE DEVICE by ``sc_sample_initial`` (Philox4x32-10 + Box-Muller), together with
          ``zi = z0 + iLz^T xi``, ``probi`` and the state of t = 0 -- nothing crosses PCIe.  Deviate j of the trajectory
          with global index ``first_index + i`` depends only on ``(seed, subsequence, first_index + i, j)``: a rank that
          owns one shard of a larger batch passes its first global index (same ensemble as one big batch) or its own
          ``subsequence`` (an independent ensemble).

        ``ntraj_total`` (default ``ntraj``) is the N of the Monte-Carlo weight 1/(N P(qi,pi)); a rank that owns one shard
        of a larger batch passes the global count.
        """
        q0, p0, Gamma_0 = hostmath.as_f64(q0), hostmath.as_f64(p0), hostmath.as_f64(Gamma_0)
        assert Gamma_0.size() == self._Gi.size(), "Width parameter matrix Gamma_0 has wrong dimensions."
        assert hostmath.is_symmetric_non_negative(Gamma_0), "Gamma_0 has to be symmetric and positive semi-definite."
        d = q0.size()[0]
        U, iGi0, iLz, detLz, dprime = hostmath.sampling_matrices(self._Gi, Gamma_0)
        z0 = torch.cat((q0, p0))
        prob0 = detLz / (2 * np.pi) ** d
        if seed is not None:
            assert generator is None, "either a host generator or a device seed"
            if not 0 <= int(subsequence) < 2 ** 56:
                raise ValueError(f"subsequence {subsequence} outside [0, 2^56)")
            dev = self.device
            self._begin_state(q0, p0, Gamma_0, U, iGi0, int(ntraj), ntraj_total)
            self._zi_t = torch.empty((ntraj, 2 * d), dtype=F64, device=dev)
            self.probi = torch.empty(ntraj, dtype=F64, device=dev)
            ilz_d, z0_d = iLz.contiguous().to(dev), z0.to(dev)
            check(lib.sc_sample_initial(self._state, ptr(ilz_d), ptr(z0_d), dprime, float(prob0), int(seed) & (2 ** 64 - 1),
                                        int(subsequence), int(first_index), 1, ptr(self._zi_t),
                                        ptr(self.probi), None, self._stream()))
            self.zi = self._zi_t.t()                   # the reference's (2D, n) attribute, as a view
            self._finish_state((ilz_d, z0_d))
            return
        zi, probi = self._draw_on_host(z0, iLz, prob0, dprime, ntraj, generator)
        self.set_initial_conditions(q0, p0, Gamma_0, zi, probi, ntraj_total=ntraj_total)

    @staticmethod
    def _draw_on_host(z0, iLz, prob0, dprime, ntraj, generator=None):
        if generator is None:
            xi = torch.distributions.Normal(torch.zeros(2 * dprime, dtype=F64),
                                            torch.ones(2 * dprime, dtype=F64)).sample((ntraj,)).T
        else:
            xi = torch.randn((ntraj, 2 * dprime), dtype=F64, generator=generator).T
        zi = z0.unsqueeze(1) + torch.einsum('ji,jn->in', iLz, xi)
        probi = prob0 * torch.exp(-0.5 * torch.einsum('in,in->n', xi, xi))
        return zi, probi

    def draw_initial_conditions(self, q0, p0, Gamma_0, ntraj, generator=None):
        """The host draw of ``initial_conditions`` without touching the state: ``(zi (2D, ntraj), probi (ntraj,))`` from
        torch's CPU generator with the call the reference makes (propagators.py:537-566).  Ranks that share one batch
        all draw the whole batch from the same seed and hand their slice to ``set_initial_conditions``."""
        q0, p0, Gamma_0 = hostmath.as_f64(q0), hostmath.as_f64(p0), hostmath.as_f64(Gamma_0)
        _, _, iLz, detLz, dprime = hostmath.sampling_matrices(self._Gi, Gamma_0)
        prob0 = detLz / (2 * np.pi) ** q0.size()[0]
        return self._draw_on_host(torch.cat((q0, p0)), iLz, prob0, dprime, int(ntraj), generator)

    def set_initial_conditions(self, q0, p0, Gamma_0, zi, probi, ntraj_total=None):
        """Start from given phase-space points ``zi`` (2D, n) with sampling densities ``probi`` (n,)."""
        q0, p0, Gamma_0 = hostmath.as_f64(q0), hostmath.as_f64(p0), hostmath.as_f64(Gamma_0)
        dev = self.device
        d, n = q0.size()[0], zi.shape[1]
        assert zi.shape[0] == 2 * d and probi.shape[0] == n
        U, iGi0, _, _, dprime = hostmath.sampling_matrices(self._Gi, Gamma_0)
        self._begin_state(q0, p0, Gamma_0, U, iGi0, n, ntraj_total)
        self.zi = torch.as_tensor(zi, dtype=F64).to(dev).contiguous()
        self.probi = torch.as_tensor(probi, dtype=F64).to(dev).contiguous()
        self._zi_t = self.zi.t().contiguous()                          # [n][2D]
        self._qp.copy_(self._zi_t)
        self._act.zero_()
        self._mono.zero_()
        torch.diagonal(self._mono[:, 0], dim1=1, dim2=2).fill_(1.0)
        torch.diagonal(self._mono[:, 3], dim1=1, dim2=2).fill_(1.0)
        self._c2.fill_(1.0)
        self._sgn.fill_(1.0)
        self._finish_state(None)

    # ---- thermal ensembles of a harmonic initial surface (not in the reference) ----
    _thermal_ok = True              # WM has another prefactor and per-trajectory widths: no thermal ensemble
    _thermal = None                 # the active thermal ensemble (constants, centres, sc_thermal_consts), None = one pure state
    _thermal_opcorr = None
    _thermal_opquad = None

    def _thermal_constants(self, q0, p0, Gamma_0, masses, temperature):
        if not self._thermal_ok:
            raise NotImplementedError(f"{type(self).__name__} has no thermal ensembles: the estimator is the Herman-Kluk expression "
                                      "with per-trajectory centres")
        q0, Gamma_0 = hostmath.as_f64(q0), hostmath.as_f64(Gamma_0)
        assert Gamma_0.size() == self._Gi.size(), "Width parameter matrix Gamma_0 has wrong dimensions."
        return hostmath.ThermalConstants(Gamma_0, masses, temperature, p0=p0)

    def thermal_initial_conditions(self, q0, p0, Gamma_0, masses, temperature, ntraj=5000, ntraj_total=None, generator=None,
                                   seed=None, subsequence=0, first_index=0):
        """``initial_conditions`` for the CANONICAL ensemble of the harmonic initial surface whose ground state is
        |q0, 0, Gamma_0> with the ``masses`` (D,) of the final-surface potential, at ``temperature`` = k_B T in Hartree
        (``units.kelvin_to_hartree`` converts): C_auto(t) and k_ic(t) become Tr[rho e^{iH_es t} e^{-iH_gs t}] and its coupling
        analogue.  rho is a positive mixture of coherent states of the width Gamma_0 (Glauber-Sudarshan P function); every
        trajectory draws its own centre from it (``thermal_centres``) and its phase-space point around that centre exactly as
        ``initial_conditions`` draws it around (q0, p0) -- ``probi`` is unchanged, the centres carry no weight.  With
        ``generator`` / by default both are drawn on the host (first the xi of ``initial_conditions``, then the centres), with
        ``seed`` on the device (``sc_sample_thermal``; ``subsequence``, ``first_index`` as in ``initial_conditions``).  At
        temperature 0 every centre is (q0, 0) and the estimator is that of ``initial_conditions``.

        While the ensemble is active ``autocorrelation``, ``ic_correlation``, ``autocorrelation_qp``, ``run`` (with standard
        errors and blocks), ``standard_errors``, ``discard_nonsymplectic``, ``thermal_operator_correlation`` /
        ``run(thermal_operators=...)`` and ``thermal_quadratic_correlation`` / ``run(thermal_quadratic=...)`` work; everything that describes ONE pure state or
        has no thermal kernel is refused (see ``_refuse_thermal``).  ``initial_conditions`` / ``set_initial_conditions`` return
        to the zero-temperature path.  ``ValueError`` for p0 != 0, a negative temperature or masses of the wrong shape."""
        tc = self._thermal_constants(q0, p0, Gamma_0, masses, temperature)
        q0, p0, Gamma_0 = hostmath.as_f64(q0), hostmath.as_f64(p0), hostmath.as_f64(Gamma_0)
        assert hostmath.is_symmetric_non_negative(Gamma_0), "Gamma_0 has to be symmetric and positive semi-definite."
        d = q0.size()[0]
        U, iGi0, iLz, detLz, dprime = hostmath.sampling_matrices(self._Gi, Gamma_0)
        prob0 = detLz / (2 * np.pi) ** d
        if seed is None:
            zi, probi = self._draw_on_host(torch.zeros(2 * d, dtype=F64), iLz, prob0, dprime, int(ntraj), generator)
            centres = tc.draw_centres(ntraj, generator)
            a, b = tc.cartesian(centres)
            zi = zi + torch.cat((q0.unsqueeze(0) + a, b), 1).T
            self.set_thermal_initial_conditions(q0, p0, Gamma_0, masses, temperature, centres, zi, probi, ntraj_total=ntraj_total)
            return
        assert generator is None, "either a host generator or a device seed"
        if not 0 <= int(subsequence) < 2 ** 56:
            raise ValueError(f"subsequence {subsequence} outside [0, 2^56)")
        dev, ntraj = self.device, int(ntraj)
        self._begin_state(q0, p0, Gamma_0, U, iGi0, ntraj, ntraj_total)
        self._zi_t = torch.empty((ntraj, 2 * d), dtype=F64, device=dev)
        self.probi = torch.empty(ntraj, dtype=F64, device=dev)
        centres = torch.empty((ntraj, 2 * tc.dmodes), dtype=F64, device=dev)
        th, bufs = self._thermal_struct(tc, centres)
        ilz_d, sq, sp = iLz.contiguous().to(dev), tc.sigma_q.to(dev), tc.sigma_p.to(dev)
        check(lib.sc_sample_thermal(self._state, ptr(ilz_d), th, ptr(sq), ptr(sp), dprime, float(prob0), int(seed) & (2 ** 64 - 1),
                                    int(subsequence), int(first_index), 1, ptr(centres), ptr(self._zi_t), ptr(self.probi), None,
                                    self._stream()))
        self.zi = self._zi_t.t()
        self._finish_state((ilz_d, sq, sp))
        self._install_thermal(tc, centres, th, bufs)

    def set_thermal_initial_conditions(self, q0, p0, Gamma_0, masses, temperature, centres, zi, probi, ntraj_total=None):
        """Start a thermal ensemble (``thermal_initial_conditions``) from given samples: ``centres`` (n, 2 d'') = (Q_i | P_i) in the
        mass-weighted normal coordinates of ``hostmath.ThermalConstants(Gamma_0, masses, temperature)``, phase-space points
        ``zi`` (2D, n) drawn around their Cartesian images with the sampling densities ``probi`` (n,)."""
        tc = self._thermal_constants(q0, p0, Gamma_0, masses, temperature)
        centres = torch.as_tensor(centres, dtype=F64)
        n = zi.shape[1]
        if centres.dim() != 2 or tuple(centres.shape) != (n, 2 * tc.dmodes):
            raise ValueError(f"centres of shape ({n}, {2 * tc.dmodes}) = (Q | P) in the {tc.dmodes} thermal modes are expected, got "
                             f"{tuple(centres.shape)}")
        self.set_initial_conditions(q0, p0, Gamma_0, zi, probi, ntraj_total=ntraj_total)
        centres = centres.to(self.device).contiguous().clone()
        th, bufs = self._thermal_struct(tc, centres)
        self._install_thermal(tc, centres, th, bufs)

    def _thermal_struct(self, tc, centres):
        """sc_thermal_consts of the constants ``tc`` and the device centres, and the buffers it points to (n1: none yet)"""
        dev = self.device
        maps = (tc.scale_q, tc.scale_p) if tc.diag else (tc.map_q, tc.map_p)
        bufs = [tc.omega.to(dev), maps[0].contiguous().to(dev), maps[1].contiguous().to(dev), self.q0, centres]
        th = _lib.sc_thermal_consts(dim=self.dim, dmodes=tc.dmodes, diag=int(tc.diag), omega=ptr(bufs[0]), map_q=ptr(bufs[1]),
                                    map_p=ptr(bufs[2]), q0=ptr(self.q0), n1=None, centres=ptr(centres))
        return th, bufs

    def _install_thermal(self, tc, centres, th, bufs):
        """switch the state that _finish_state has just completed to the thermal estimator: the initial overlaps with the
        per-trajectory centres replace those with (q0, p0)"""
        self._thermal = {"consts": tc, "centres": centres, "struct": th, "bufs": bufs}
        check(lib.sc_hk_thermal_initial(th, self._ovl_i0, None, ptr(self._zi_t), self.ntraj, ptr(self._vi), None, self._stream()))
        self._corr_step = -1

    @property
    def thermal_centres(self):
        """(n, 2 d'') centres (Q_i | P_i) of the thermal ensemble at t = 0 on the device (do not write to it), None without one"""
        return None if self._thermal is None else self._thermal["centres"]

    def _refuse_thermal(self, what, why):
        if self._thermal is not None:
            raise NotImplementedError(f"{what} is not available with a thermal ensemble: {why}")

    def _begin_state(self, q0, p0, Gamma_0, U, iGi0, n, ntraj_total):
        """host constants + the (uninitialised) engine state of a batch of ``n`` trajectories"""
        dev = self.device
        d = q0.size()[0]
        self.dim, self.ntraj = d, n
        self._ntraj_norm = n if ntraj_total is None else int(ntraj_total)
        self._q0h, self._p0h, self._G0h, self._iGi0h = q0, p0, Gamma_0, iGi0
        self.q0, self.p0, self.Gamma_0 = q0.to(dev), p0.to(dev), Gamma_0.to(dev)
        self.U, self.iGi0 = U.to(dev), iGi0.to(dev)
        # ---- engine state (trajectory-major) ----
        self._qp = torch.empty((n, 2 * d), dtype=F64, device=dev)
        self._act = torch.empty(n, dtype=F64, device=dev)
        self._mono = torch.empty((n, 4, d, d), dtype=F64, device=dev)
        self._c2 = torch.empty(n, dtype=C128, device=dev)
        self._sgn = torch.empty(n, dtype=F64, device=dev)
        self._flags = torch.zeros(n + 2, dtype=torch.int32, device=dev)     # [n] = flagged count, [n + 1] = work cursor
        self._work = torch.zeros((n, 4, d), dtype=F64, device=dev)
        self._state = sc_state(n=n, dim=d, mono_layout=_lib.SC_MONO_ROWMAJOR, qp=ptr(self._qp), act=ptr(self._act),
                               mono=ptr(self._mono), c2=ptr(self._c2), sgn=ptr(self._sgn), work=ptr(self._work),
                               flags=ptr(self._flags))

    def _finish_state(self, keep_alive):
        """per-step scratch, constants and the prefactor of t = 0 once (q, p, S, M) and (zi, probi) are in place"""
        dev, n, d = self.device, self.ntraj, self.dim
        self._ic_bufs = keep_alive                    # device operands of a sampling launch that may still be running
        self._gstep = lib.sc_step_grid(n, d)
        self._gcorr = lib.sc_correlate_grid(n, d)
        self._epart = torch.zeros(self._gstep, dtype=F64, device=dev)
        self._cpart = torch.zeros((self._gcorr, 4), dtype=F64, device=dev)
        self._gterm = lib.sc_term_moments_grid(n)
        # second-moment partials (standard errors): rows of sc_hk_correlate_m or of sc_term_moments
        self._mpart = torch.zeros((max(self._gcorr, self._gterm), 6), dtype=F64, device=dev)
        self._cq = torch.zeros(n, dtype=C128, device=dev)
        self._kq = torch.zeros(n, dtype=C128, device=dev)
        self._slot = torch.zeros(8, dtype=F64, device=dev)
        self._elog = torch.zeros(4, dtype=F64, device=dev)            # energy guard log (sc_energy_guard)
        self._nsteps = 0
        self._corr_step, self._corr_has_nac = -1, False
        self._nac, self._nac_pot, self._nac_fp, self._nac_generic = None, None, None, None
        self._dense = None
        # diagonals of the monodromy blocks for the separable shortcut; _mono is stale while they are ahead of it
        self._mdiag = torch.zeros((n, 4, d), dtype=F64, device=dev)
        self._mdiag[:, 0] = 1.0
        self._mdiag[:, 3] = 1.0
        self._mono_is_diag, self._mono_stale = True, False
        # The monodromy blocks are the identity now and stay DIAGONAL as long as only separable potentials act on them.  Nothing in
        # the dense-state kernels uses that -- except that diagonal blocks cannot meet a weak pivot, which is what lets run() take
        # two time steps per visit (sc_hk_step_multi: an intermediate determinant cannot be repaired after the fact).
        self._blocks_structurally_diagonal = True
        self._multi = None
        # normal-mode constants of the modal step (sc_hk_step_modal) depend on U (Gamma_0): rebuilt for every new state.
        # _modal_basis: the constants whose A, B the monodromy blocks are expressed in, None = Cartesian (the identity of t = 0 is
        # the identity in both bases)
        self._modal_step_cache, self._modal_basis = {}, None
        # discard mask (discard_nonsymplectic): None until the first mark -- every route then runs the launches it always ran
        self._kept, self._discarded_at, self._kept_count, self._masked_scratch = None, None, None, None
        self._cross = None            # constants and scratch of cross_correlation(): depend on Gamma_0 and n
        self._opcorr = None           # folded operators, g and scratch of operator_correlation(): depend on (zi, Gamma_0, q0, p0) and n
        self._thermal = None          # thermal ensemble (thermal_initial_conditions installs it after this): None = one pure state
        self._thermal_opquad = None   # the same of thermal_quadratic_correlation()
        self._thermal_opcorr = None   # folded operators, g and scratch of thermal_operator_correlation(): as _opcorr, and the centres

        self._prepare()
        self.t = 0.0
        self._prefactor_initial()

    def _prepare(self):
        """constants of the three overlaps and of the prefactor (reference propagators.py:633-643)"""
        dev = self.device
        self._pre = hostmath.PrefactorConstants(self._Gi, self._Gt, self.U.cpu())
        up = lambda x: x.contiguous().to(dev)
        self._pre_bufs = ([up(self._pre.st), up(self._pre.si)] if self._pre.diag else
                          [up(self._pre.L1), up(self._pre.L2), up(self._pre.R1), up(self._pre.R2)])
        b = self._pre_bufs
        if self._pre.diag:
            self._hk = sc_hk_consts(dim=self.dim, dprime=self.dim, diag=1, st=ptr(b[0]), si=ptr(b[1]))
        else:
            # imaginary parts of U^T Gt^(+-1/2), Gi^(-+1/2) U: zero for positive semi-definite widths up to rounding dust
            # (1e-24 for methylium); "real" = below one ulp of the largest entry, so dropping them changes no bit
            real = all(float(m.imag.abs().max()) <= 1e-17 * float(m.real.abs().max()) for m in
                       (self._pre.L1, self._pre.L2, self._pre.R1, self._pre.R2))
            self._hk = sc_hk_consts(dim=self.dim, dprime=self._pre.dprime, diag=0, real_lr=int(real),
                                    L1=ptr(b[0]), L2=ptr(b[1]), R1=ptr(b[2]), R2=ptr(b[3]))
        self._ovl_i0, self._ovl_i0_bufs = self._overlap_consts(self._Gi, self._G0h)
        self._ovl_t0, self._ovl_t0_bufs = self._overlap_consts(self._Gt, self._G0h)
        # <qi,pi,Gamma_i|phi(0)> does not depend on time: evaluate once (reference recomputes it every step, :794-795)
        self._vi = torch.zeros(self.ntraj, dtype=C128, device=dev)
        check(lib.sc_overlap(self._ovl_i0, ptr(self._zi_t), self.ntraj, ptr(self._vi), self._stream()))

    def _overlap_consts(self, Gbra, Gket):
        oc = hostmath.OverlapConstants(Gbra, Gket)
        dev = self.device
        if oc.diag:
            mats = [torch.diagonal(m).contiguous().to(dev) for m in (oc.A, oc.B, oc.C)]
        else:
            mats = [m.contiguous().to(dev) for m in (oc.A, oc.B, oc.C)]
        bufs = mats + [self.q0, self.p0]
        c = sc_overlap_consts(dim=self.dim, diag=int(oc.diag), A=ptr(bufs[0]), B=ptr(bufs[1]), C=ptr(bufs[2]),
                              qk=ptr(self.q0), pk=ptr(self.p0), fac=oc.fac)
        return c, bufs

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _prefactor_initial(self):
        """prefactor at t = 0 and initialisation of the branch tracker (reference propagators.py:631)"""
        if self.dim > 64:
            check(lib.sc_dense_mono_step(self._state, self._hk, None, None, self._mono_sums_ptr(), 0.0, 1, self._stream()))
        else:
            check(lib.sc_hk_step(_NULL_POT(self.dim), self._state, self._hk, 0.0, 1, None, self._stream()))
        self._after_prefactor(track=2)

    # ------------------------------------------------------------------ time stepping
    def step(self, potential, dt):
        """propagate all trajectories by one RK4 step t -> t+dt (reference propagators.py:645-655)"""
        assert self.dim == potential.dimensions(), "potential has wrong dimensions"
        self._launch_step(potential, float(dt))
        self.t += float(dt)

    # ---- optional per-kernel timing (bench.py): HIP events on the launch stream around labelled launches ----
    kernel_timing = False

    def _timed(self, label):
        return _KernelTimer(self, label) if self.kernel_timing else _NO_TIMER

    def kernel_times_ms(self):
        """{label: [duration of every launch recorded while ``kernel_timing`` was set]}; synchronises"""
        torch.cuda.current_stream(self.device).synchronize()
        return {k: [a.elapsed_time(b) for a, b in v] for k, v in self.__dict__.get("_kernel_events", {}).items()}

    def _launch_step(self, potential, dt, desc=None, remembered=False):
        """``desc`` / ``remembered``: run() resolves the potential's device descriptor and coupling constants once per
        call instead of once per step"""
        s = self._stream()
        timed = getattr(self, "profile_step_kernel", False)
        if timed:
            # HIP events on the launch stream, bracketing only the step kernel(s) (bench.py roofline)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        if hasattr(potential, "_gdml_model"):
            self._blocks_structurally_diagonal = False
            self._leave_modal()
            self._sync_dense_mono(leave_diagonal=True)
            self._set_mono_layout(_lib.SC_MONO_ROWMAJOR)
            nblocks = self._launch_dense_step(potential, dt, s)
        elif hasattr(potential, "_qff_model") and self.dim <= lib.sc_qff_max_dim():
            # quartic force field (in front of the descriptor test: the molecular base class carries the descriptor mixin)
            self._blocks_structurally_diagonal = False
            self._leave_modal()
            self._sync_dense_mono(leave_diagonal=True)
            self._set_mono_layout(_lib.SC_MONO_ROWMAJOR)
            nblocks = self._launch_qff_step(potential, dt, s)
        elif not hasattr(potential, "_descriptor") or hasattr(potential, "_qff_model") or self.dim > 64:
            # no device descriptor, or beyond the fused kernels' D <= 64: the potential's own torch code + dense path
            self._blocks_structurally_diagonal = False
            self._leave_modal()
            self._sync_dense_mono(leave_diagonal=True)
            self._set_mono_layout(_lib.SC_MONO_ROWMAJOR)
            nblocks = self._launch_generic_step(potential, dt, s)
        else:
            if desc is None:
                desc = self._potential_descriptor(potential, dt)
            if desc.kind not in _lib.SEPARABLE_KINDS:
                self._blocks_structurally_diagonal = False          # a dense Hessian couples the rows
            modal = self._modal_step_constants(potential, desc, dt)
            if modal is not None:
                # constant dense Hessian, 16 < D <= 64: the blocks stay in normal-mode coordinates between such steps
                self._sync_dense_mono(leave_diagonal=True)
                self._set_mono_layout(_lib.SC_MONO_ROWMAJOR)
                self._enter_modal(modal)
                with self._timed("hk_step_modal"):
                    check(lib.sc_hk_step_modal(desc, self._state, modal["hk"], dt, 0, ptr(modal["phi"]), ptr(self._epart), s))
            elif self._shortcut_applies(desc):
                self._leave_modal()
                check(lib.sc_hk_step_diag(desc, self._state, self._hk, ptr(self._mdiag), dt, 0, ptr(self._epart), s))
                self._mono_stale = True
            else:
                self._leave_modal()
                self._sync_dense_mono(leave_diagonal=True)
                self._set_mono_layout(self._fast_path_layout(desc))
                with self._timed("hk_step"):
                    check(lib.sc_hk_step(desc, self._state, self._hk, dt, 0, ptr(self._epart), s))
            nblocks = self._gstep
        if timed:
            e1.record()
            self.__dict__.setdefault("_step_events", []).append((e0, e1, 1))
        check(lib.sc_energy_guard(ptr(self._epart), nblocks, float(self.ntraj), ptr(self._elog), s))
        self._nsteps += 1
        if not remembered:
            self._remember_nac(potential)
        self._after_prefactor(track=1)

    def _shortcut_applies(self, desc):
        return (self.exploit_separability and self._mono_is_diag and bool(self._pre.diag)
                and desc.kind in _lib.SEPARABLE_KINDS)

    # The separable fast path streams the monodromy blocks in 16 x 16 tiles (SC_MONO_TILED16, include/semiclassical_hip.h);
    # everything else reads them row-major.  The state switches order in place when it enters / leaves that path.
    _tiled_fast_path = True

    def _fast_path_layout(self, desc):
        fast = (self._tiled_fast_path and bool(self._pre.diag) and 16 < self.dim <= 64
                and desc.kind in _lib.SEPARABLE_KINDS)
        return _lib.SC_MONO_TILED16 if fast else _lib.SC_MONO_ROWMAJOR

    def _set_mono_layout(self, layout):
        if self._state.mono_layout != layout:
            check(lib.sc_mono_convert(self._state, layout, self._stream()))
            self._state.mono_layout = layout

    def _sync_dense_mono(self, leave_diagonal=False):
        """bring the dense monodromy blocks up to date with the diagonals the shortcut kernel advanced"""
        if self._mono_stale:
            self._state.mono_layout = _lib.SC_MONO_ROWMAJOR       # rebuilt from the diagonals below
            self._mono.zero_()
            torch.diagonal(self._mono, dim1=2, dim2=3).copy_(self._mdiag)
            self._mono_stale = False
        if leave_diagonal:
            self._mono_is_diag = False          # a dense kernel takes over: the diagonals are no longer maintained

    def _launch_dense_step(self, potential, dt, s):
        """unfused RK4 step for a dense, position-dependent Hessian: four stage kernels + the monodromy kernel"""
        self._dense_scratch(potential)
        with torch.cuda.device(self.device):
            model = potential._gdml_model(self.device)
        for stage in range(4):
            with self._timed("gdml_stage"):
                check(lib.sc_gdml_stage_scratch(model, ptr(self._gdml_scratch), self._state, self._dense, dt, stage,
                                                ptr(self._epart), s))
        with self._timed("dense_mono_step"):
            check(lib.sc_dense_mono_step(self._state, self._hk, model.inv_mass, ptr(self._dense_bufs[0]),
                                         self._mono_sums_ptr(), dt, 0, s))
        return self._gdense

    def _launch_qff_step(self, potential, dt, s):
        """unfused RK4 step on a quartic force field: four sc_qff_stage calls (stage Hessians on the FP64 matrix cores, written
        straight into the image of the monodromy kernel) + the monodromy kernel"""
        self._dense_scratch()
        need = lib.sc_qff_scratch_bytes(self.ntraj, self.dim)
        have = getattr(self, "_qff_scratch", None)
        if have is None or have.numel() * 8 < need:
            self._qff_scratch = torch.empty((need + 7) // 8, dtype=F64, device=self.device)
        with torch.cuda.device(self.device):
            model = potential._qff_model(self.device)
        for stage in range(4):
            with self._timed("qff_stage"):
                check(lib.sc_qff_stage(model, ptr(self._qff_scratch), self._state, self._dense, dt, stage, ptr(self._epart), s))
        with self._timed("dense_mono_step"):
            check(lib.sc_dense_mono_step(self._state, self._hk, model.inv_mass, ptr(self._dense_bufs[0]),
                                         self._mono_sums_ptr(), dt, 0, s))
        return self._gdense

    def _dense_scratch(self, gdml=None):
        """scratch of the unfused dense path: stage Hessians, slopes of the previous stage, weighted slope sums; with an
        sGDML potential ``gdml`` also the scratch of sc_gdml_stage (beyond 48 atoms, ``self._gdml_scratch``)"""
        n, d = self.ntraj, self.dim
        if gdml is not None:
            need = gdml.scratch_bytes()
            have = getattr(self, "_gdml_scratch", None)
            if need > 0 and (have is None or have.numel() * 8 < need):
                self._gdml_scratch = torch.empty((need + 7) // 8, dtype=F64, device=self.device)
            elif need == 0 and have is None:
                self._gdml_scratch = None
        if getattr(self, "_dense", None) is None:
            dev = self.device
            bufs = [torch.empty((n, 4, d, d), dtype=F64, device=dev), torch.zeros((n, 2 * d), dtype=F64, device=dev),
                    torch.zeros((n, 2 * d), dtype=F64, device=dev), torch.zeros(n, dtype=F64, device=dev)]
            self._dense_bufs = bufs
            self._dense = sc_dense_scratch(hess=ptr(bufs[0]), kprev=ptr(bufs[1]), ksum=ptr(bufs[2]), ssum=ptr(bufs[3]))
            self._gdense = lib.sc_dense_grid(n)
            if self._gdense > self._epart.numel():
                self._epart = torch.zeros(self._gdense, dtype=F64, device=dev)
        return self._dense

    def _mono_sums_ptr(self):
        """scratch of sc_dense_mono_step beyond D = 64: the RK4 sums of the MFMA kernel up to D = 96, the per-workgroup
        matrix blocks of the any-dimension kernels beyond (sc_dense_mono_scratch_bytes)"""
        need = lib.sc_dense_mono_scratch_bytes(self.ntraj, self.dim, self._hk.dprime)
        assert need >= 0
        if need == 0:
            return None
        if getattr(self, "_mono_sums", None) is None or self._mono_sums.numel() * 8 < need:
            self._mono_sums = torch.empty((need + 7) // 8, dtype=F64, device=self.device)
        return ptr(self._mono_sums)

    def _launch_generic_step(self, potential, dt, s):
        """Any object with the reference's potential protocol (potentials.py:41-204: ``harmonic_approximation(r) ->
        V (n,), grad (D,n), hess (D,D,n)``, ``masses()``): the potential is evaluated by ITS OWN torch code on the
        device at the four RK4 stage points; the RK4 bookkeeping, the monodromy GEMMs and the prefactor stay in HIP
        (generic Python potentials take the unfused path)."""
        n, d = self.ntraj, self.dim
        dense = self._dense_scratch()
        masses = hostmath.as_f64(potential.masses())
        cached = getattr(self, "_generic_masses", None)
        if getattr(self, "_generic_pot", None) is not potential or cached is None or not torch.equal(cached, masses):
            self._generic_inv_mass = (1.0 / masses).to(self.device).contiguous()
            self._generic_r = torch.empty((n, d), dtype=F64, device=self.device)
            self._generic_pot, self._generic_masses = potential, masses.clone()
        r, inv_mass = self._generic_r, self._generic_inv_mass
        for stage in range(4):
            check(lib.sc_stage_point(self._state, dense, dt, stage, ptr(r), s))
            V, grad, hess = potential.harmonic_approximation(r.t())
            assert V.shape == (n,) and grad.shape == (d, n) and hess.shape == (d, d, n), \
                "harmonic_approximation has to return V (n,), grad (D,n), hess (D,D,n)"
            Vc = V.to(F64).contiguous()
            gt = grad.to(F64).t().contiguous()
            # the monodromy kernel takes the stage Hessian image as A[i][k] = image[k][i]: store the transpose
            self._dense_bufs[0][:, stage].copy_(hess.permute(2, 1, 0))
            check(lib.sc_stage_consume(self._state, dense, ptr(inv_mass), ptr(Vc), ptr(gt), dt, stage,
                                       ptr(self._epart), s))
        check(lib.sc_dense_mono_step(self._state, self._hk, ptr(inv_mass), ptr(self._dense_bufs[0]), self._mono_sums_ptr(),
                                     dt, 0, s))
        return self._gdense

    def _after_prefactor(self, track):
        """hook for propagators whose prefactor needs more than the HK determinant (WM)"""

    def _potential_descriptor(self, potential, dt=None):
        if not hasattr(potential, "_descriptor"):
            raise TypeError(f"{type(potential).__name__} has no device descriptor: it takes the unfused path "
                            "(_launch_generic_step), not a fused kernel")
        with torch.cuda.device(self.device):
            return potential._descriptor(self.device) if dt is None else potential._descriptor(self.device, dt)

    def _check_energy_guard(self):
        """raise the reference's RuntimeError (propagators.py:396) if <T+V> jumped by more than 1e-2 Hartree"""
        change = float(self._elog[2].item())
        if change > 1.0e-2:
            raise RuntimeError(f"average energy of classical trajectories is not conserved, change= {change} Hartree")

    def synchronize(self):
        torch.cuda.current_stream(self.device).synchronize()
        self._run_scratch = None              # partial sums of the last whole-loop run(): consumed by now
        if self._multi is not None and int(self._multi["bad"].item()) != 0:
            raise _lib.EngineError("sc_hk_step_multi met a weak pivot in an intermediate determinant although the monodromy blocks "
                                   "were taken to be diagonal: the results of this run() are not reliable")
        self._check_energy_guard()

    def mean_energy(self):
        """<T+V> over the trajectories as the energy guard saw it at the last step: the value at the k4 stage point
        (reference propagators.py:380 ``_en_mean``, quirk Q2), not that of the accepted state.  Host sync."""
        return float(self._elog[1].item())

    def step_kernel_times_ms(self):
        """duration PER TIME STEP of the step-kernel launches recorded while ``profile_step_kernel`` was set (a launch of the
        steps-per-visit paths counts for its number of time steps)"""
        torch.cuda.current_stream(self.device).synchronize()
        return [e0.elapsed_time(e1) / steps for e0, e1, steps in self.__dict__.get("_step_events", [])]

    # ------------------------------------------------------------------ correlation functions
    def _nac_is_current(self, potential):
        """(is the cached coupling data that of `potential`?, fingerprint of `potential`)"""
        fp = _potential_fingerprint(potential)
        return (self._nac_pot is potential and _same_fingerprint(self._nac_fp, fp)), fp

    def _remember_nac(self, potential):
        current, fp = self._nac_is_current(potential)
        if current:
            return
        masses, tau1, tau2, varies = fp
        dev = self.device
        if bool(varies.item()):
            self._refuse_thermal("a potential with position-dependent derivative couplings",
                                 "the thermal correlate kernel takes a constant coupling vector")
        self._nac_pot, self._nac_fp = potential, tuple(x.clone() for x in fp)
        self._corr_step = -1
        if bool(varies.item()):
            # position-dependent couplings: evaluated per trajectory by the potential's own torch code (_nac_terms)
            self._nac, self._nac_bufs, self._nacq = None, None, None
            G = self._G0h @ self._iGi0h
            self._nac_generic = {"minv": (1.0 / masses).to(dev).unsqueeze(1), "R": (G @ self._Gi).to(dev), "G": G.to(dev)}
            self._nac_generic["initial"] = self._nac_terms(potential, self.zi[:self.dim], self.zi[self.dim:], sign=+1.0)
            return
        self._nac_generic = None
        nc = hostmath.NacConstants(self._G0h, self._Gi, self._iGi0h, self._p0h, masses, tau1,
                                   tau2_sum=float(torch.sum(tau2 / masses)))
        bufs = [nc.rn.to(dev), nc.gn.to(dev)]
        self._nac = sc_nac_consts(dim=self.dim, rn=ptr(bufs[0]), gn=ptr(bufs[1]), q0=ptr(self.q0), p0=ptr(self.p0),
                                  p0n1=nc.p0n1, n2=nc.n2)
        self._nac_bufs = bufs
        self._nacq = torch.zeros(self.ntraj, dtype=C128, device=dev)
        if self._thermal is not None:
            # the coupling factor of the initial points with the per-trajectory centres; the kernels need the vector n1 itself
            th = self._thermal
            th["n1"] = (-hbar ** 2 * tau1 / masses).contiguous().to(dev)
            th["struct"].n1 = ptr(th["n1"])
            check(lib.sc_hk_thermal_initial(th["struct"], self._ovl_i0, self._nac, ptr(self._zi_t), self.ntraj, None, ptr(self._nacq),
                                            self._stream()))
            return
        check(lib.sc_nac_initial(self._nac, ptr(self._zi_t), self.ntraj, ptr(self._nacq), self._stream()))

    def _coupling_vectors(self, potential, r):
        """n1 (D, n) and n2 (n,) of eqns (89), (90) at the positions r (D, n) on the device, reference propagators.py:880-892"""
        c = self._nac_generic
        tau1 = potential.derivative_coupling_1st(r).to(F64)
        tau2 = potential.derivative_coupling_2nd(r).to(F64)
        assert tau1.shape == r.shape and tau2.shape == r.shape, "derivative couplings have to be of shape (D, n)"
        return -hbar ** 2 * c["minv"] * tau1, -hbar ** 2 * 0.5 * torch.sum(c["minv"] * tau2, dim=0)

    def _nac_terms(self, potential, r, mom, sign):
        """nacq (sign = +1, initial points) or nacQ (sign = -1, current points) of propagators.py:894-903 for
        position-dependent couplings, (n,) complex on the device"""
        c = self._nac_generic
        n1, n2 = self._coupling_vectors(potential, r)
        PI = self.p0.unsqueeze(1) + c["G"] @ (mom - self.p0.unsqueeze(1))
        real = n2 + torch.sum((self.q0.unsqueeze(1) - r) * (c["R"] @ n1), dim=0)
        return torch.complex(real, sign / hbar * torch.sum(PI * n1, dim=0))

    def _generic_kic(self, slot_row):
        """k_ic sum of the current state for position-dependent couplings into slot_row[2:4] (device, no host sync):
        sum_i nacQ_i nacq_i cq_i / hbar^2 with the per-trajectory C_auto terms the correlate kernel just wrote"""
        c = self._nac_generic
        qp = self._qp.t()
        nacQ = self._nac_terms(self._nac_pot, qp[:self.dim], qp[self.dim:], sign=-1.0)
        kq = nacQ * c["initial"] * self._cq / hbar ** 2
        self._kq.copy_(kq)
        total = torch.sum(kq)
        slot_row[2:4] = torch.view_as_real(total)

    def _mc_norm(self):
        return self._ntraj_norm * (2 * np.pi * hbar) ** self.dim

    def _reduce_into(self, partials, count, row, cursor, mom_rows=None):
        """sums of the per-workgroup partials into the slot of `row`, or into row *cursor of the slot buffer that starts there; with
        `mom_rows` also the six moment sums of the first `mom_rows` rows of self._mpart into the moment row (with a cursor: the same
        launch, one advance)"""
        s = self._stream()
        if cursor is None:
            check(lib.sc_reduce_slot(ptr(partials), count, None, 0, 1.0, C_void(row.slot), s))
            if mom_rows is not None:
                check(lib.sc_reduce_moments(ptr(self._mpart), mom_rows, C_void(row.moments), s))
        elif mom_rows is None:
            check(lib.sc_reduce_slot_at(ptr(partials), count, C_void(row.slot), ptr(cursor), s))
        else:
            check(lib.sc_reduce_slot_moments_at(ptr(partials), count, ptr(self._mpart), mom_rows, C_void(row.slot),
                                                C_void(row.moments), ptr(cursor), s))

    def _term_moments(self, has_k):
        """moment partials of the exported per-trajectory terms _cq (and _kq) into self._mpart; returns their row count"""
        check(lib.sc_term_moments(ptr(self._cq), ptr(self._kq) if has_k else None, self.ntraj, ptr(self._mpart), self._stream()))
        return self._gterm

    def _term_moments_into(self, has_k, moments):
        """the six moment sums of the exported per-trajectory terms into the doubles at `moments`"""
        check(lib.sc_reduce_moments(ptr(self._mpart), self._term_moments(has_k), C_void(moments), self._stream()))

    def _term_blocks(self, has_k, blk, cursor=None):
        """block sums of the exported per-trajectory terms _cq (and _kq) into the (B, 4) doubles at blk = (address, B), or into
        row *cursor of the (., B, 4) buffer there (the cursor is read, not advanced: launch before the reduction that advances it)"""
        out, nblocks = blk
        kq = ptr(self._kq) if has_k else None
        if cursor is None:
            check(lib.sc_term_blocks(ptr(self._cq), kq, self.ntraj, nblocks, C_void(out), self._stream()))
        else:
            check(lib.sc_term_blocks_at(ptr(self._cq), kq, self.ntraj, nblocks, C_void(out), ptr(cursor), self._stream()))

    def _masked_sums(self, has_k, row):
        """the sums of the exported terms _cq (and _kq) over the kept trajectories, in place of _reduce_into / _term_moments /
        _term_blocks: columns 0 ... 3 of the slot of `row` (column 4 is not touched), its six moments, its (B, 4) block sums --
        one pass, sc_term_masked_sums"""
        if self._masked_scratch is None:
            self._masked_scratch = torch.empty(lib.sc_term_masked_scratch_doubles(), dtype=F64, device=self.device)
        out, nblocks = (None, 0) if row.blocks is None else row.blocks
        check(lib.sc_term_masked_sums(ptr(self._cq), ptr(self._kq) if has_k else None, ptr(self._kept), self.ntraj, nblocks,
                                      ptr(self._masked_scratch), C_void(row.slot), None if row.moments is None else C_void(row.moments),
                                      None if out is None else C_void(out), self._stream()))

    def _launch_correlate_thermal(self, row, state, time, cursor, families):
        """_launch_correlate while a thermal ensemble is active: sc_hk_correlate_thermal, which always exports the terms, in the
        place of sc_hk_correlate_m; every sum after it is the launch that follows an exporting correlate kernel today.  `time`: the
        clock of `state` (the bra centres rotate with it)."""
        if cursor is not None:
            raise ValueError("use_graph=True is not available with a thermal ensemble: the time of the state is an argument of the "
                             "correlate kernel, which a graph replay cannot change")
        for fam, _ in families:
            if fam is not _THERMAL_OPERATOR_ROWS and fam is not _THERMAL_QUADRATIC_ROWS:
                raise NotImplementedError(f"{fam.arg} are not available with a thermal ensemble: their kernels take the one "
                                          "centre (q0, p0)")
        s, nac, th = self._stream(), self._nac, self._thermal
        time = float(self.t if time is None else time)
        with self._timed("hk_correlate_thermal"):
            check(lib.sc_hk_correlate_thermal(self._state if state is None else state, time,
                                              self._ovl_t0, nac, th["struct"], ptr(self._vi), ptr(self.probi),
                                              ptr(self._nacq) if nac is not None else None, self._mc_norm(), ptr(self._cq),
                                              ptr(self._kq) if nac is not None else None, ptr(self._cpart), s))
        for fam, prepared in families:
            getattr(self, fam.launch)(prepared, getattr(row, fam.row or fam.field), state=state, time=time)
        if self._kept is not None:
            self._masked_sums(nac is not None, row)
            return
        if row.blocks is not None:
            self._term_blocks(nac is not None, row.blocks)
        self._reduce_into(self._cpart, self._gcorr, row, None)
        if row.moments is not None:
            self._term_moments_into(nac is not None, row.moments)

    def _launch_correlate(self, row, state=None, cursor=None, per_trajectory=True, families=(), time=None):
        """per-trajectory terms + their sums for the current state into `row` (_StepRows): the 5-double slot; the six second-moment
        sums, formed inside the correlate kernel; the block sums -- the terms are exported and sc_term_blocks follows the correlate
        kernel.  `state`: another view of (q, p, S, c2, sign) -- the state between the two steps of sc_hk_step_multi -- and `time`
        its clock (None: self.t; read by the thermal kernel only).  Under a
        discard mask the correlate kernel only exports the terms; sc_term_masked_sums forms every sum from them.  `families`:
        (family of _ROW_FAMILIES, its prepared dict) of the five-sum rows wanted: the (count, 5) sums of the same state go to the
        family's field of the row, one launch each after the correlate kernel, which exports its terms where a launch reads them."""
        if self._thermal is not None:
            return self._launch_correlate_thermal(row, state, time, cursor, families)
        s = self._stream()
        nac = self._nac
        mom_ptr, blk = row.moments, row.blocks
        generic = getattr(self, "_nac_generic", None) is not None
        masked = self._kept is not None
        if masked and generic:
            raise NotImplementedError("position-dependent derivative couplings are not available once trajectories have been "
                                      "discarded (discard_nonsymplectic)")
        per_trajectory = per_trajectory or generic or blk is not None or masked or any(fam.needs_terms for fam, _ in families)
        in_kernel = mom_ptr is not None and not generic and not masked
        with self._timed("hk_correlate"):
            check(lib.sc_hk_correlate_m(self._state if state is None else state, self._ovl_t0, nac, ptr(self._vi), ptr(self.probi),
                                        ptr(self._nacq) if nac is not None else None, self._mc_norm(),
                                        ptr(self._cq) if per_trajectory else None,
                                        ptr(self._kq) if per_trajectory else None, ptr(self._cpart),
                                        ptr(self._mpart) if in_kernel else None, s))
        for fam, prepared in families:
            getattr(self, fam.launch)(prepared, None if fam.field is None else getattr(row, fam.row or fam.field), state=state,
                                      cursor=cursor)
        if masked:
            assert cursor is None
            self._masked_sums(nac is not None, row)
            return
        if blk is not None and not generic:
            self._term_blocks(nac is not None, blk, cursor)
        self._reduce_into(self._cpart, self._gcorr, row, cursor, self._gcorr if in_kernel else None)
        if generic:
            assert cursor is None
            self._generic_kic(row.slots[row.k])
            if blk is not None:
                self._term_blocks(True, blk)
            if mom_ptr is not None:
                # k_ic terms formed by torch (position-dependent couplings): the moments of the exported terms
                self._term_moments_into(True, mom_ptr)

    def _correlate_current(self, need_nac):
        if self._corr_step == self._nsteps and (self._corr_has_nac or not need_nac):
            return
        self._launch_correlate(self._rows.single(self._slot))
        self._corr_step, self._corr_has_nac = self._nsteps, (self._nac is not None or self._nac_generic is not None)
        self._slot_host = self._slot.cpu().numpy().copy()          # host sync
        self._check_energy_guard()

    def autocorrelation_qp(self):
        """per-trajectory terms of the autocorrelation function (reference propagators.py:784-807)"""
        self._correlate_current(False)
        return self._cq * (self._mc_norm() * self.probi)

    def autocorrelation(self, energy0_es=0.0):
        """C_auto(t) = e^{i t E0/hbar} <phi(0)|phi(t)> for the current step (reference propagators.py:809-843)"""
        self._correlate_current(False)
        c = complex(self._slot_host[0], self._slot_host[1])
        return c * np.exp(1j / hbar * self.t * energy0_es)

    def ic_correlation(self, potential, energy0_es=0.0):
        """k_ic(t) for the current step (reference propagators.py:845-911)"""
        self._remember_nac(potential)
        self._correlate_current(True)
        k = complex(self._slot_host[2], self._slot_host[3])
        return k * np.exp(1j / hbar * self.t * energy0_es)

    # ---- cross-correlation with target coherent states (not in the reference) ----
    def _cross_constants(self):
        """La = A^(1/2), Lb = B^(1/2) / hbar and C of the overlap <q_i, p_i, Gamma_t|q_k, p_k, Gamma_0> on the host and as sc_hk_cross
        takes them (diagonals for diagonal widths; else La, Lb and the transpose of C), plus the call's scratch -- once per state"""
        if self._cross is None:
            oc = hostmath.OverlapConstants(self._Gt, self._G0h)
            sym = lambda m: 0.5 * (m + m.T)
            La, Lb = hostmath.psd_sqrt_real(sym(oc.A)), hostmath.psd_sqrt_real(sym(oc.B)) / hbar
            dev, n, d = self.device, self.ntraj, self.dim
            if oc.diag:
                bufs = [torch.diagonal(m).contiguous().to(dev) for m in (La, Lb, oc.C)]
            else:
                bufs = [La.contiguous().to(dev), Lb.contiguous().to(dev), oc.C.T.contiguous().to(dev)]
            self._cross = {"La": La, "Lb": Lb, "C": oc.C, "diag": bool(oc.diag), "fac": float(oc.fac), "bufs": bufs,
                           "operands": None if oc.diag else torch.empty((n, 4 * d), dtype=F64, device=dev), "partials": None}
        return self._cross

    def _cross_targets(self, q_targets, p_targets):
        """validated targets and their operand rows [La q_k | Lb p_k | q_k | C p_k | p_k] on the device"""
        if not self._cross_ok:
            raise NotImplementedError(f"{type(self).__name__} has no cross-correlation with target coherent states: its Gaussians "
                                      "have per-trajectory widths and another prefactor")
        if getattr(self, "_thermal", None) is not None:
            raise NotImplementedError("a cross-correlation with target coherent states is not available with a thermal ensemble: "
                                      "sc_hk_cross takes the one centre (q0, p0)")
        try:
            Q, P = np.asarray(q_targets, dtype=np.float64), np.asarray(p_targets, dtype=np.float64)
        except (TypeError, ValueError) as err:
            raise ValueError(f"targets: real arrays of shape (K, {self.dim}) are expected ({err})")
        if Q.ndim != 2 or Q.shape != P.shape or Q.shape[1] != self.dim:
            raise ValueError(f"targets: q_targets and p_targets of shape (K, {self.dim}) are expected, got {Q.shape} and {P.shape}")
        if Q.shape[0] == 0:
            raise ValueError("targets: at least one target is expected (K = 0)")
        if not (np.isfinite(Q).all() and np.isfinite(P).all()):
            raise ValueError("targets: non-finite entry")
        cc = self._cross_constants()
        Qt, Pt = torch.from_numpy(Q.copy()), torch.from_numpy(P.copy())
        rows = torch.cat((Qt @ cc["La"].T, Pt @ cc["Lb"].T, Qt, Pt @ cc["C"].T, Pt), 1).contiguous().to(self.device)
        K = int(Q.shape[0])
        need = int(lib.sc_hk_cross_rows(self.ntraj, K)) * K * 5
        if cc["partials"] is None or cc["partials"].numel() < need:
            cc["partials"] = torch.empty(need, dtype=F64, device=self.device)
        return {"K": K, "rows": rows, "q": Q, "p": P}

    def _prepare_targets(self, targets):
        """run(targets=...): the caller's pair into the prepared dict of _cross_targets"""
        try:
            q_targets, p_targets = targets
        except (TypeError, ValueError):
            raise ValueError("targets: a pair (q_targets, p_targets) of arrays (K, D) is expected")
        return self._cross_targets(q_targets, p_targets)

    def _launch_cross(self, targets, out_ptr, state=None, cursor=None):
        """the (K, 5) cross-correlation sums of `state` (default: the current one) into the doubles at `out_ptr`, or into row *cursor
        of the (., K, 5) buffer there (the cursor is read, not advanced); honours the discard mask"""
        cc = self._cross_constants()
        b = cc["bufs"]
        with self._timed("hk_cross"):
            check(lib.sc_hk_cross(self._state if state is None else state, ptr(b[0]), ptr(b[1]), ptr(b[2]), int(cc["diag"]),
                                  cc["fac"], ptr(targets["rows"]), targets["K"], ptr(self._vi), ptr(self.probi), self._mc_norm(),
                                  ptr(self._kept), ptr(cc["operands"]), ptr(cc["partials"]), C_void(out_ptr),
                                  None if cursor is None else ptr(cursor), self._stream()))

    def cross_correlation(self, q_targets, p_targets, energy0_es=0.0, standard_errors=False):
        """C_k(t) = e^{i t E0/hbar} <phi_k|psi(t)> for the current step, phi_k = |q_k, p_k, Gamma_0> the coherent states at the rows
        of ``q_targets``, ``p_targets`` (K, D) (not in the reference): a complex ndarray (K,).  Linear in the
        ensemble like ``autocorrelation()``, which it equals for (q_k, p_k) = (q0, p0).  With ``standard_errors`` the result is
        ``(C, sigma)``, sigma = sigma_Re + i sigma_Im per target (``hostmath.standard_errors``).  Trajectories discarded by
        ``discard_nonsymplectic`` count as samples of value zero, N unchanged.  Synchronises; the state is not touched: the steps
        that follow give the bits they would have given without the call.  ``ValueError`` for targets of the wrong shape, with
        non-finite entries or K = 0."""
        targets = self._cross_targets(q_targets, p_targets)
        out = torch.zeros((1, targets["K"], 5), dtype=F64, device=self.device)
        self._launch_cross(targets, self._rows.single(cross=out).cross)
        return self._current_five_sums(out, energy0_es, standard_errors)

    def _current_five_sums(self, out, energy0_es, standard_errors):
        """X, or (X, sigma), of the current step from the one raw row (1, count, 5) a launch has just filled.  Synchronises."""
        self.synchronize()
        X, sigma = self.finalize_cross(out, self.t, 0.0, energy0_es, self._ntraj_norm)
        return (X[0], sigma[0]) if standard_errors else X[0]

    @staticmethod
    def phased_cross(cross, t0, dt, energy0_es):
        """(C, m3): the cross-correlation functions C_k(t), complex (nt, K), and the second-moment sums (S_rr, S_ii, S_ri) of the
        phased terms (nt, K, 3) from the raw rows (nt, K, 5) of run(..., cross=...): the dynamical phase of finalize_slots and the
        rotation of phased_moments"""
        raw = cross.detach().cpu().numpy() if isinstance(cross, torch.Tensor) else np.asarray(cross)
        times = t0 + hostmath.time_grid(raw.shape[0], dt)
        C = (raw[:, :, 0] + 1j * raw[:, :, 1]) * np.exp(1j / hbar * times * energy0_es)[:, None]
        return C, hostmath.rotate_second_moments(raw[:, :, 2:5], (times * energy0_es / hbar)[:, None])

    @staticmethod
    def finalize_cross(cross, t0, dt, energy0_es, ntraj_norm):
        """(C, sigma), complex (nt, K): the cross-correlation functions C_k(t) and their Monte-Carlo standard errors
        sigma_Re + i sigma_Im from the raw rows (nt, K, 5) of run(..., cross=...) (summed over ranks when sharded): phased_cross and
        the error algebra of finalize_moments"""
        C, m3 = HermanKlukPropagator.phased_cross(cross, t0, dt, energy0_es)
        return C, hostmath.standard_errors(C, m3, ntraj_norm)

    # ---- time-averaged spectra (not in the reference) ----
    def time_average(self, energies, dt, references=None, max_bytes=2 ** 32):
        """An accumulator of the time-averaged Herman-Kluk spectrum (Kaledin and Miller, separable prefactor; DESIGN.md section
        4.17) of the reference states |q_k, p_k, Gamma_0>, ``references`` = (Q, P), arrays (K, D), K <= 64; None: the one state
        (q0, p0).  ``energies``: the E_e (NE,), Hartree.  Over a window of ns steps of ``dt`` that starts at the current time t_a,

            I_k(E) = sum_i |dt sum_s e^{i E t_s/hbar} <chi_k|q_i(t_s) p_i(t_s)> e^{i S_i/hbar} c_i/|c_i| |^2 / (2 pi hbar T mc_norm P_i),

        t_s = t_a + s dt, T = ns dt: every trajectory adds a non-negative number, the peaks sit at the eigenvalues of the surface
        the trajectories run on with the weights |<chi_k|n>|^2.  Fill it with ``run(..., time_average=acc)`` or, step by step,
        ``acc.add()``; read it with ``acc.spectrum()``.  It owns 16 n K NE bytes on the device: ``ValueError`` (naming the size)
        above ``max_bytes``, for empty or non-finite energies, references of the wrong shape or K > 64."""
        if not self._cross_ok:
            raise NotImplementedError(f"{type(self).__name__} has no time-averaged spectra: its Gaussians have per-trajectory "
                                      "widths and another prefactor")
        self._refuse_thermal("a time-averaged spectrum", "its terms take fixed reference states, not per-trajectory centres")
        return TimeAverageAccumulator(self, energies, dt, references, max_bytes)

    def _launch_ta_terms(self, acc, out_ptr=None, state=None, cursor=None):
        """one column of the accumulator's terms from `state` (default: the current one); honours the discard mask"""
        assert cursor is None
        acc._append(state)

    @staticmethod
    def finalize_time_average(raw, T, ntraj_norm):
        """(I, sigma), real (K, NE): the time-averaged spectrum over a window of length T and its Monte-Carlo standard error from
        the raw sums (K, NE, 2) of ``TimeAverageAccumulator.raw_sums()`` (added over batches of one N and over ranks when
        sharded): I = raw[..., 0] / T, sigma = sqrt(max(N raw[..., 1] / T^2 - I^2, 0) / (N - 1)) (``hostmath.standard_errors``)"""
        raw = raw.detach().cpu().numpy() if isinstance(raw, torch.Tensor) else np.asarray(raw, dtype=np.float64)
        I = raw[..., 0] / T
        m3 = np.zeros(I.shape + (3,))
        m3[..., 0] = raw[..., 1] / T ** 2
        return I, hostmath.standard_errors(I, m3, ntraj_norm).real

    # ---- correlation functions with linear and quadratic operators (not in the reference; DESIGN.md sections 4.14, 4.16) ----
    @staticmethod
    def _is_operator_set(x):
        """(c, m) or (c, m, K) with c one-dimensional, m two-dimensional and K three-dimensional or None"""
        try:
            return (len(x) in (2, 3) and np.ndim(x[0]) == 1 and np.ndim(x[1]) == 2
                    and (len(x) == 2 or x[2] is None or np.ndim(x[2]) == 3))
        except (TypeError, ValueError):
            return False

    def _operator_set(self, name, ops):
        """validated (c (M,), m (M, D)) of one side as fp64 host tensors (its K: _operator_hessians)"""
        expected = (f"operators: {name} = (c, m) or (c, m, K) with c of shape (M,), m of shape (M, {self.dim}) and K of shape "
                    f"(M, {self.dim}, {self.dim}) or None is expected")
        if not self._is_operator_set(ops):
            raise ValueError(expected)
        try:
            c, m = np.asarray(ops[0], dtype=np.float64), np.asarray(ops[1], dtype=np.float64)
        except (TypeError, ValueError) as err:
            raise ValueError(f"operators: real arrays are expected for {name} ({err})")
        if m.shape != (c.shape[0], self.dim):
            raise ValueError(f"{expected}, got {c.shape} and {m.shape}")
        if c.shape[0] == 0:
            raise ValueError("operators: at least one operator is expected (M = 0)")
        if not (np.isfinite(c).all() and np.isfinite(m).all()):
            raise ValueError(f"operators: non-finite entry in {name}")
        return torch.from_numpy(c.copy()), torch.from_numpy(m.copy())

    @staticmethod
    def _operator_hessians(name, ops, M, D):
        """validated K (M, D, D) of one side's (c, m, K) as an fp64 host tensor; None when the set has no K, K is None or every entry
        is zero: the operators are linear then (the path of section 4.14)"""
        if len(ops) == 2 or ops[2] is None:
            return None
        try:
            K = np.asarray(ops[2], dtype=np.float64)
        except (TypeError, ValueError) as err:
            raise ValueError(f"operators: a real array is expected for K of {name} ({err})")
        if K.shape != (M, D, D):
            raise ValueError(f"operators: K of {name} of shape ({M}, {D}, {D}) is expected, got {K.shape}")
        if not np.isfinite(K).all():
            raise ValueError(f"operators: non-finite entry in K of {name}")
        for a in range(M):
            if abs(K[a] - K[a].T).max() > 1.0e-12 * abs(K[a]).max():
                raise ValueError(f"operators: K of operator {a} of {name} is not symmetric")
        return torch.from_numpy(K.copy()) if K.any() else None

    def _operator_side(self, name, ops):
        """(c, m, K or None) of one side"""
        c, m = self._operator_set(name, ops)
        return c, m, self._operator_hessians(name, ops, int(c.shape[0]), self.dim)

    @staticmethod
    def _operators_key(A, B):
        """what the prepared operators are cached by: the bytes of (c, m, K) of both sides, an absent (or all-zero) K as nothing"""
        return tuple(b"" if t is None else t.numpy().tobytes() for t in tuple(A) + tuple(B))

    def _operator_pair(self, cache, bra, ket, refused, refused_k, fold, rows):
        """The preparation of an operator pair, shared by both families: the class refusal, the family's refusal of the ensemble
        (``refused``: an exception or None), both sides validated (``ket`` None: the bra's, K included), its refusal of a K
        (``refused_k``), the count check; the prepared dict, cached in the attribute ``cache`` per set of operators until the initial
        conditions change (_finish_state).  ``fold(A, B, M, g)``: the family's folded buffers on the device and its *_initial launch
        into g, returns (bufs, further entries of the dict); ``rows``: its *_rows query."""
        if not self._opcorr_ok:
            raise NotImplementedError(f"{type(self).__name__} has no operator correlation functions: its Gaussians have "
                                      "per-trajectory widths and another prefactor")
        if refused is not None:
            raise refused
        A = self._operator_side("bra", bra)
        B = A if ket is None else self._operator_side("ket", ket)
        if refused_k is not None and (A[2] is not None or B[2] is not None):
            raise refused_k
        if B[0].shape != A[0].shape:
            raise ValueError(f"operators: bra and ket have to hold the same number of operators, got {A[0].shape[0]} and {B[0].shape[0]}")
        key = self._operators_key(A, B)
        hit = getattr(self, cache)
        if hit is not None and hit["key"] == key:
            return hit
        M = int(A[0].shape[0])
        g = torch.empty((self.ntraj, M), dtype=C128, device=self.device)
        bufs, more = fold(A, B, M, g)
        partials = torch.empty(max(int(rows(self.ntraj, M)) * M * 5, 1), dtype=F64, device=self.device)
        numpy_set = lambda c, m, K: (c.numpy(), m.numpy()) + (() if K is None else (K.numpy(),))
        setattr(self, cache, {"key": key, "M": M, "bra": numpy_set(*A), "ket": numpy_set(*B), "bufs": bufs, "g": g,
                              "partials": partials, **more})
        return getattr(self, cache)

    def _operators(self, bra, ket=None):
        """validated operators A_a = cA_a + mA_a.x + 1/2 x^T KA_a x (``bra``) and B_a (``ket``), their folded vectors and the
        ket-side factors g [n][M] of the initial points on the device (_operator_pair, _fold_operators)"""
        refused = None if getattr(self, "_thermal", None) is None else NotImplementedError(
            "an operator correlation function is not available with a thermal ensemble: the folded operators take the one centre "
            "(q0, p0); the trace over the ensemble is thermal_operator_correlation() / run(thermal_operators=...), with a K "
            "thermal_quadratic_correlation() / run(thermal_quadratic=...)")
        return self._operator_pair("_opcorr", bra, ket, refused, None, self._fold_operators, lib.sc_hk_opcorr_rows)

    def _fold_operators(self, A, B, M, g):
        """Without a K on either side: the affine forms of hostmath.fold_linear_operators and sc_hk_opcorr_initial (section 4.14);
        with one: the columns of hostmath.fold_quadratic_operators and sc_hk_opquad_initial (section 4.16), and the ranks"""
        dev, host = self.device, (self._G0h, self._q0h, self._p0h)
        if A[2] is None and B[2] is None:
            uA, wA, kA = hostmath.fold_linear_operators(*A[:2], self._Gt, *host, ket=False)
            uB, wB, kB = hostmath.fold_linear_operators(*B[:2], self._Gi, *host, ket=True)
            bufs = [t.to(dev) for t in (uA, wA, kA, uB, wB, kB)]
            check(lib.sc_hk_opcorr_initial(ptr(self._zi_t), self.ntraj, self.dim, ptr(bufs[3]), ptr(bufs[4]), ptr(bufs[5]), M, ptr(g),
                                           self._stream()))
            return bufs, {}
        *colsA, RA = hostmath.fold_quadratic_operators(*A, self._Gt, *host, ket=False)
        *colsB, RB = hostmath.fold_quadratic_operators(*B, self._Gi, *host, ket=True)
        bufs = [t.to(dev) for t in colsA + colsB]          # (u, w, kappa, lambda) of the bra, then of the ket
        check(lib.sc_hk_opquad_initial(ptr(self._zi_t), self.ntraj, self.dim, ptr(bufs[4]), ptr(bufs[5]), ptr(bufs[6]),
                                       ptr(bufs[7]), M, RB, ptr(g), self._stream()))
        return bufs, {"RA": RA, "RB": RB}

    def _parse_operator_pair(self, operators, sets):
        """the (bra, ket), or bra alone, of run() as (bra, ket or None); ``sets``: one side of the family, for the error text"""
        if self._is_operator_set(operators):
            operators = (operators, None)
        try:
            bra, ket = operators
        except (TypeError, ValueError):
            raise ValueError(f"operators: (bra, ket) or bra, each {sets}, is expected")
        return bra, ket

    def _prepare_operators(self, operators):
        """run(operators=...): the prepared dict of _operators"""
        return self._operators(*self._parse_operator_pair(operators, "(c, m) or (c, m, K) of arrays (M,), (M, D) and (M, D, D)"))

    def _launch_opcorr(self, operators, out_ptr, state=None, cursor=None):
        """the (M, 5) operator-correlation sums of `state` (default: the current one) from the terms _cq the correlate kernel has
        exported for it, into the doubles at `out_ptr`, or into row *cursor of the (., M, 5) buffer there (the cursor is read, not
        advanced); honours the discard mask.  sc_hk_opquad when the prepared operators carry columns ("RA"), else sc_hk_opcorr."""
        b = operators["bufs"]
        st, cur = self._state if state is None else state, None if cursor is None else ptr(cursor)
        if "RA" in operators:
            with self._timed("hk_opquad"):
                check(lib.sc_hk_opquad(st, ptr(self._cq), ptr(b[0]), ptr(b[1]), ptr(b[2]), ptr(b[3]), ptr(operators["g"]),
                                       operators["M"], operators["RA"], ptr(self._kept), ptr(operators["partials"]), C_void(out_ptr),
                                       cur, self._stream()))
            return
        with self._timed("hk_opcorr"):
            check(lib.sc_hk_opcorr(st, ptr(self._cq), ptr(b[0]), ptr(b[1]), ptr(b[2]), ptr(operators["g"]), operators["M"],
                                   ptr(self._kept), ptr(operators["partials"]), C_void(out_ptr), cur, self._stream()))

    def operator_correlation(self, bra, ket=None, energy0_es=0.0, standard_errors=False):
        """X_a(t) = e^{i t E0/hbar} <phi_0| A_a e^{-iHt/hbar} B_a |phi_0> for the current step with M pairs of linear or quadratic
        operators A_a = cA_a + mA_a.x + 1/2 x^T KA_a x, B_a likewise (not in the reference; DESIGN.md sections 4.14, 4.16): a complex
        ndarray (M,).  ``bra`` = (c, m) or (c, m, K), real arrays (M,), (M, D) and (M, D, D) in the coordinates of q0, every K_a the
        symmetric Hessian of its operator (x_j x_k with j != k is K_jk = K_kj = 1, x_j^2 is K_jj = 2); K = None or all zeros: linear
        operators, the same bits as (c, m).  ``ket`` likewise, None = the operators of the bra, K included.
        Every trajectory's C_auto term is multiplied by the closed-form Gaussian matrix elements of A at its current and of B at its
        initial phase-space point, the way ``ic_correlation`` treats the non-adiabatic coupling: linear in the ensemble like
        ``autocorrelation()``, which it equals for c = 1, m = 0.  With ``standard_errors`` the result is ``(X, sigma)``, sigma =
        sigma_Re + i sigma_Im per pair (``hostmath.standard_errors``).  Trajectories discarded by ``discard_nonsymplectic`` count as
        samples of value zero, N unchanged.  Synchronises; the state is not touched: the steps that follow give the bits they would
        have given without the call.  ``ValueError`` for operators of the wrong shape, with non-finite entries, M = 0, a K that is
        not symmetric, or a vector m or an eigenvector of K (eigenvalue above 1e-12 of the largest) outside the range of
        Gamma_0 + Gamma_t (bra) or Gamma_i + Gamma_0 (ket)."""
        return self._current_operator_rows(_OPERATOR_ROWS, self._operators(bra, ket), energy0_es, standard_errors)

    def _current_operator_rows(self, family, operators, energy0_es, standard_errors):
        """X, or (X, sigma), of the current step: the correlate kernel and the launch of ``family`` into one raw row.  Synchronises."""
        out = torch.zeros((1, operators["M"], 5), dtype=F64, device=self.device)
        slot = torch.zeros(8, dtype=F64, device=self.device)
        self._launch_correlate(self._rows.single(slot, opcorr=out), families=((family, operators),))
        return self._current_five_sums(out, energy0_es, standard_errors)

    # ---- operator correlation functions of a thermal ensemble, linear operators (not in the reference) ----
    def _thermal_operators(self, bra, ket=None):
        """``_operators`` for the active thermal ensemble: validated linear operators, their folded vectors and the ket-side factors
        g [n][M] on the device (_operator_pair, _fold_thermal_operators)"""
        refused = None if self._thermal is not None else ValueError(
            "thermal operators need a thermal ensemble (thermal_initial_conditions): the expectation value in the one state phi_0 "
            "is operator_correlation() / run(operators=...)")
        refused_k = NotImplementedError("quadratic operators (a K) are not taken by thermal_operator_correlation() / "
                                        "run(thermal_operators=...), whose operators are linear (c, m): "
                                        "thermal_quadratic_correlation() / run(thermal_quadratic=...) takes them")
        return self._operator_pair("_thermal_opcorr", bra, ket, refused, refused_k, self._fold_thermal_operators,
                                   lib.sc_hk_opcorr_thermal_rows)

    def _fold_thermal_operators(self, A, B, M, g):
        """the folded vectors of hostmath.fold_thermal_linear_operators -- (u, w, ut, wt, kappa) of the bra, then of the ket -- and
        sc_hk_opcorr_thermal_initial"""
        th = self._thermal
        tc = th["consts"]
        folded = (hostmath.fold_thermal_linear_operators(*A[:2], self._Gt, self._G0h, self._q0h, tc, ket=False)
                  + hostmath.fold_thermal_linear_operators(*B[:2], self._Gi, self._G0h, self._q0h, tc, ket=True))
        bufs = [folded[i].to(self.device) for i in (0, 1, 3, 4, 2, 5, 6, 8, 9, 7)]        # (u, w, ut, wt, kappa) twice
        check(lib.sc_hk_opcorr_thermal_initial(ptr(self._zi_t), ptr(th["centres"]), self.ntraj, self.dim, tc.dmodes, ptr(bufs[5]),
                                               ptr(bufs[6]), ptr(bufs[7]), ptr(bufs[8]), ptr(bufs[9]), M, ptr(g), self._stream()))
        return bufs, {}

    def _prepare_thermal_operators(self, operators):
        """run(thermal_operators=...): the prepared dict of _thermal_operators"""
        return self._thermal_operators(*self._parse_operator_pair(operators, "(c, m) of arrays (M,) and (M, D)"))

    def _launch_thermal_opcorr(self, operators, out_ptr, state=None, time=None, cursor=None):
        """the (M, 5) thermal operator-correlation sums of `state` (default: the current one), whose clock reads `time` (None:
        self.t), from the terms _cq sc_hk_correlate_thermal has exported for it, into the doubles at `out_ptr`; honours the
        discard mask"""
        assert cursor is None
        b, th = operators["bufs"], self._thermal
        with self._timed("hk_opcorr_thermal"):
            check(lib.sc_hk_opcorr_thermal(self._state if state is None else state, float(self.t if time is None else time),
                                           th["struct"], ptr(self._cq), ptr(b[0]), ptr(b[1]), ptr(b[2]), ptr(b[3]), ptr(b[4]),
                                           ptr(operators["g"]), operators["M"], ptr(self._kept), ptr(operators["partials"]),
                                           C_void(out_ptr), None, self._stream()))

    def thermal_operator_correlation(self, bra, ket=None, energy0_es=0.0, standard_errors=False):
        """X_a(t) = e^{i t E0/hbar} Tr[rho e^{i H_es t/hbar} A_a e^{-i H_gs t/hbar} B_a] for the current step of a thermal ensemble
        (``thermal_initial_conditions``) with M pairs of LINEAR operators A_a = cA_a + mA_a.x, B_a likewise (not in the reference;
        DESIGN.md section 4.20): a complex ndarray (M,) -- the Herzberg-Teller dipole correlation function at a temperature.
        ``bra`` = (c, m), real arrays (M,) and (M, D) in the coordinates of q0; ``ket`` likewise, None = the operators of the bra.
        Every trajectory's thermal C_auto term is multiplied by the Gaussian matrix elements of A between its own centre, rotated to
        the current time, and its current point, and of B between its initial point and its centre: ``operator_correlation`` with
        per-trajectory centres, which it equals at temperature 0, and ``autocorrelation()`` for c = 1, m = 0.  With
        ``standard_errors`` the result is ``(X, sigma)``.  Discarded trajectories count as samples of value zero, N unchanged.
        Synchronises; the state is not touched: the steps that follow give the bits they would have given without the call.
        ``ValueError`` without a thermal ensemble (the quantity is ``operator_correlation`` then), for operators of the wrong
        shape, with non-finite entries, M = 0, another M on the ket, or a vector m outside the range of Gamma_0 + Gamma_t (bra) or
        Gamma_i + Gamma_0 (ket); ``NotImplementedError`` for operators with a K."""
        return self._current_operator_rows(_THERMAL_OPERATOR_ROWS, self._thermal_operators(bra, ket), energy0_es, standard_errors)

    # ---- ... and quadratic operators (not in the reference) ----
    def _thermal_quadratic(self, bra, ket=None):
        """``_thermal_operators`` for operators that may carry a K: validated, folded into columns, and the ket-side factors g [n][M]
        on the device (_operator_pair, _fold_thermal_quadratic)"""
        refused = None if self._thermal is not None else ValueError(
            "thermal quadratic operators need a thermal ensemble (thermal_initial_conditions): the expectation value in the one "
            "state phi_0 is operator_correlation() / run(operators=...)")
        return self._operator_pair("_thermal_opquad", bra, ket, refused, None, self._fold_thermal_quadratic,
                                   lib.sc_hk_opquad_thermal_rows)

    def _fold_thermal_quadratic(self, A, B, M, g):
        """Without a K on either side: exactly _fold_thermal_operators (section 4.20); with one: the columns of hostmath.
        fold_thermal_quadratic_operators -- (u, w, ut, wt, kappa, lambda) of the bra, then of the ket --, sc_hk_opquad_thermal_initial
        and the ranks"""
        if A[2] is None and B[2] is None:
            return self._fold_thermal_operators(A, B, M, g)
        th = self._thermal
        tc = th["consts"]
        *colsA, RA = hostmath.fold_thermal_quadratic_operators(*A, self._Gt, self._G0h, self._q0h, tc, ket=False)
        *colsB, RB = hostmath.fold_thermal_quadratic_operators(*B, self._Gi, self._G0h, self._q0h, tc, ket=True)
        order = (0, 1, 4, 5, 2, 3)                         # (u, w, kappa, lambda, ut, wt) -> (u, w, ut, wt, kappa, lambda)
        bufs = [cols[i].to(self.device) for cols in (colsA, colsB) for i in order]
        check(lib.sc_hk_opquad_thermal_initial(ptr(self._zi_t), ptr(th["centres"]), self.ntraj, self.dim, tc.dmodes, *map(ptr, bufs[6:]),
                                               M, RB, ptr(g), self._stream()))
        return bufs, {"RA": RA, "RB": RB}

    def _prepare_thermal_quadratic(self, operators):
        """run(thermal_quadratic=...): the prepared dict of _thermal_quadratic"""
        return self._thermal_quadratic(*self._parse_operator_pair(operators, "(c, m) or (c, m, K) of arrays (M,), (M, D) and (M, D, D)"))

    def _launch_thermal_opquad(self, operators, out_ptr, state=None, time=None, cursor=None):
        """_launch_thermal_opcorr for the prepared dict of _thermal_quadratic: sc_hk_opquad_thermal when it carries columns ("RA"),
        else that very launch, sc_hk_opcorr_thermal"""
        if "RA" not in operators:
            return self._launch_thermal_opcorr(operators, out_ptr, state=state, time=time, cursor=cursor)
        assert cursor is None
        b, th = operators["bufs"], self._thermal
        with self._timed("hk_opquad_thermal"):
            check(lib.sc_hk_opquad_thermal(self._state if state is None else state, float(self.t if time is None else time),
                                           th["struct"], ptr(self._cq), *map(ptr, b[:6]), ptr(operators["g"]), operators["M"],
                                           operators["RA"], ptr(self._kept), ptr(operators["partials"]), C_void(out_ptr), None,
                                           self._stream()))

    def thermal_quadratic_correlation(self, bra, ket=None, energy0_es=0.0, standard_errors=False):
        """X_a(t) = e^{i t E0/hbar} Tr[rho e^{i H_es t/hbar} A_a e^{-i H_gs t/hbar} B_a] for the current step of a thermal ensemble
        with M pairs of linear or QUADRATIC operators A_a = cA_a + mA_a.x + 1/2 x^T KA_a x, B_a likewise (not in the reference;
        DESIGN.md section 4.22): a complex ndarray (M,) -- the energy-gap correlation function between two harmonic surfaces,
        second-order Herzberg-Teller terms and thermal second moments <x_j x_k>, each with an error bar.  ``bra`` = (c, m) or
        (c, m, K) as for ``operator_correlation`` (K_a the symmetric Hessian), ``ket`` likewise, None = the operators of the bra, K
        included.  ``thermal_operator_correlation`` with the matrix elements of ``operator_correlation``: every trajectory's thermal
        C_auto term times the Gaussian matrix element of A between its own centre, rotated to the current time, and its current
        point, and of B between its initial point and its centre.  A K that is None or all zeros on both sides takes the path of
        ``thermal_operator_correlation`` and gives its bits.  With ``standard_errors`` the result is ``(X, sigma)``.  Discarded
        trajectories count as samples of value zero, N unchanged.  Synchronises; the state is not touched.
        ``ValueError`` without a thermal ensemble, for operators of the wrong shape, with non-finite entries, M = 0, another M on
        the ket, a K that is not symmetric, or a vector m or an eigenvector of K (eigenvalue above 1e-12 of the largest) outside the
        range of Gamma_0 + Gamma_t (bra) or Gamma_i + Gamma_0 (ket)."""
        return self._current_operator_rows(_THERMAL_QUADRATIC_ROWS, self._thermal_quadratic(bra, ket), energy0_es, standard_errors)

    def run(self, potential, dt, nt, energy0_es=0.0, slots=None, use_graph=False, moments=None, standard_errors=False, blocks=None,
            targets=None, cross=None, operators=None, opcorr=None, time_average=None, thermal_quadratic=None, thermal_opquad=None,
            thermal_operators=None, thermal_opcorr=None):
        """The caller loop of cli.py:401-436 on the device: ``nt`` times (C_auto, k_ic, step), no host sync.

        Returns ``(autocorrelation[nt], ic_correlation[nt])`` as complex NumPy arrays.  With ``slots`` (a
        device tensor (nt, 5)) the raw sums are left on the device for a later flush (see distributed.py)
        and ``None`` is returned.  Columns 0..3 of row k are Re C, Im C, Re k, Im k of the state before step k.
        Column 4 belongs to the engine: the whole-loop kernel (``sc_hk_run``) leaves the mean <T+V> of step k there,
        the step-at-a-time paths do not touch it -- do not keep data of your own in it across ``run()``.

        ``use_graph``: for small batches the loop is bound by the ~6 kernel launches per step, not by the kernels.
        The first iteration then runs as usual and the launch sequence of the second one is captured in a HIP graph
        that is replayed for the remaining steps (the row of ``slots`` a step writes is a device-resident cursor, so
        no kernel argument changes between steps).  Only for the fused kernels (device potential descriptor, D <= 64).

        Separable potentials with diagonal width matrices and 16 < D <= 64 advance TWO time steps per launch while the monodromy
        blocks are known to be diagonal (``sc_hk_step_multi``: the second step's reads come from the memory-side cache; results
        bit-identical to one launch per step; ``pair_steps = False`` switches it off).  For 32 < D <= 64 and an ensemble whose
        blocks exceed the memory-side cache (``visit_min_bytes``) a visit takes up to ``visit_steps`` (three; at most four) time steps
        (``sc_hk_step_visit``: one read and one write of the blocks per visit), the last ``nt mod visit_steps`` steps a shorter
        visit or a single step; ``visit_steps = 2`` is the launch sequence of pairs.  Same bits either way.

        Standard errors: ``moments`` (a contiguous float64 device tensor (>= nt, 6), parallel to ``slots``) receives per step the
        sums over the trajectories of (Re c_i)^2, (Im c_i)^2, Re c_i Im c_i of the C_auto terms, then the same of the k_ic terms,
        without the dynamical phase (``finalize_moments`` applies it and forms the errors).  With ``slots=None`` and
        ``standard_errors=True`` the return value is ``(C, k, sigma_C, sigma_k)``, sigma = sigma_Re + i sigma_Im of each step.
        C and k are the same bit for bit with or without moments.

        Error bars of the rate: ``blocks`` (a contiguous float64 device tensor (>= nt, B, 4), B a power of two in 2 ... 64) receives
        per step the sums Re C, Im C, Re k, Im k over each of the B blocks of trajectories (``hostmath.error_block``; row k = the
        state before step k, without the dynamical phase: ``finalize_blocks`` applies it), on every route.  Their sum over the
        blocks is the slot row; any linear functional of C(t) or k(t) evaluated per block gives its standard error
        (``hostmath.block_standard_error``, ``rates.rate_standard_error``).  Independent of ``moments``; slots and moments are the
        same bit for bit with or without blocks.

        After ``discard_nonsymplectic`` (a discard mask exists): slots, moments and blocks are the sums over the kept trajectories
        (``sc_term_masked_sums`` after every correlate launch, the intermediate states of pairs and visits included).  The loop
        then never runs as the one-launch kernel (it exports no terms) and ``use_graph=True`` raises ``ValueError``.

        Cross-correlation functions: ``targets`` = (Q, P), arrays (K, D) of target coherent states (``cross_correlation``): a
        ``sc_hk_cross`` launch follows every correlate launch, the intermediate states of pairs and visits included.  With
        ``slots=None`` the returned tuple gains ``X`` (nt, K) complex at its end, and ``sigma_X`` after it with ``standard_errors=True``.
        With ``slots`` given ``cross`` is required: a contiguous float64 device tensor (>= nt, K, 5) that receives the raw rows
        (Re X, Im X, S_rr, S_ii, S_ri per target, no phase; plain sums with the global N in the weight, so the buffers of ranks add)
        for ``finalize_cross``.  With targets the loop never runs as the one-launch kernel (it exports no per-step state): on those
        shapes C and k are the step-at-a-time loop's; everywhere else C, k, moments, blocks and the final state are the same bit for
        bit with or without targets.  ``use_graph=True`` with targets raises ``ValueError``.

        Operator correlation functions: ``operators`` = (bra, ket) or bra alone, each (c (M,), m (M, D)) or (c, m, K (M, D, D)) of
        operators c_a + m_a.x + 1/2 x^T K_a x, K_a the symmetric Hessian, None or zeros for linear operators
        (``operator_correlation``): a ``sc_hk_opcorr`` launch (``sc_hk_opquad`` with a K) follows every correlate launch, which
        then exports its per-trajectory terms as it does for blocks.  Everything said of targets holds with ``opcorr`` (>= nt, M, 5) in the place of
        ``cross``; ``X`` (nt, M) and ``sigma_X`` come after the cross outputs.

        Thermal operator correlation functions: ``thermal_operators`` = (bra, ket) or bra alone, each (c (M,), m (M, D)), on a
        thermal ensemble (``thermal_operator_correlation``): a ``sc_hk_opcorr_thermal`` launch with the state's own time follows
        every ``sc_hk_correlate_thermal`` launch, the intermediate states of pairs and visits included.  Everything said of
        operators holds with ``thermal_opcorr`` (>= nt, M, 5) in the place of ``opcorr``; ``ValueError`` without a thermal ensemble.

        Thermal correlation functions with quadratic operators: ``thermal_quadratic`` = (bra, ket) or bra alone, each (c, m) or
        (c, m, K) (``thermal_quadratic_correlation``): a ``sc_hk_opquad_thermal`` launch (``sc_hk_opcorr_thermal`` without a K) with
        the state's own time follows every ``sc_hk_correlate_thermal`` launch.  Everything said of the thermal operators holds with
        ``thermal_opquad`` (>= nt, M, 5) in the place of ``thermal_opcorr``.  Together with ``thermal_operators`` in one call:
        ``ValueError`` -- linear operators go into the same set with K None.

        Time-averaged spectra: ``time_average`` = an accumulator of ``time_average()``: a ``sc_hk_ta_terms`` launch follows every
        correlate launch, the intermediate states of pairs and visits included, and every TB-th column one ``sc_hk_ta_accumulate``
        launch.  Columns that do not fill a block stay pending in the accumulator across calls (``spectrum()`` / ``raw_sums()``
        flush them): a loop cut into several ``run()`` calls leaves the bits of the uncut loop.  The return value does not change.
        As with targets the loop never runs as the one-launch kernel; everywhere else every output and the final state are the
        same bit for bit with or without the accumulator.  ``ValueError`` for a ``dt`` other than the accumulator's and for
        ``use_graph=True``.
        """
        assert self.dim == potential.dimensions(), "potential has wrong dimensions"
        if use_graph and self._kept is not None:
            raise ValueError("use_graph=True is not available once trajectories have been discarded (discard_nonsymplectic): the "
                             "graph replay has no masked reduction")
        if self._thermal is not None:
            # (the whole-loop kernels are never taken either: _whole_loop_applies)
            if use_graph:
                raise ValueError("use_graph=True is not available with a thermal ensemble: the time of the state is an argument of "
                                 "the correlate kernel, which a graph replay cannot change")
            for name, arg in (("targets", targets), ("operators", operators), ("time_average", time_average)):
                if arg is not None:
                    self._refuse_thermal(f"run({name}=...)", "its kernel takes the one centre (q0, p0)")
        given = {"targets": targets, "cross": cross, "operators": operators, "opcorr": opcorr,
                 "thermal_operators": thermal_operators, "thermal_opcorr": thermal_opcorr,
                 "thermal_quadratic": thermal_quadratic, "thermal_opquad": thermal_opquad}
        if thermal_operators is not None and thermal_quadratic is not None:
            raise ValueError("run(thermal_operators=..., thermal_quadratic=...): one set of thermal operators per call -- linear "
                             "operators go into thermal_quadratic with K None")
        families, bufs, counts = [], {}, {}
        for fam in _RUN_ROW_FAMILIES:
            arg, buf = given[fam.arg], given[fam.field]
            if arg is None:
                if buf is not None:
                    raise ValueError(f"{fam.field}= receives the sums of run({fam.arg}=...): pass the {fam.arg} as well")
                continue
            if use_graph:
                raise ValueError(f"use_graph=True is not available with {fam.arg}: the graph replay has no {fam.what} launch")
            if slots is not None and buf is None:
                raise ValueError(f"run(slots=..., {fam.arg}=...) leaves the raw sums on the device: pass {fam.field}=, a float64 device "
                                 f"tensor (>= nt, {fam.letter}, 5), to receive those of the {fam.arg}")
            prepared = getattr(self, fam.prepare)(arg)
            counts[fam.letter] = prepared[fam.letter]
            if buf is not None and fam.row is not None:        # validated under the caller's name, then a buffer of the row's field
                self._rows._check(fam.field, buf, nt, (counts[fam.letter], 5), self.device)
            bufs[fam.row or fam.field] = torch.zeros((nt, counts[fam.letter], 5), dtype=F64, device=self.device) if buf is None else buf
            families.append((fam, prepared))
        dt = float(dt)
        hooks = list(families)                                     # what follows every correlate launch
        if time_average is not None:
            if use_graph:
                raise ValueError("use_graph=True is not available with time_average: the graph replay has no time-average terms launch")
            if not isinstance(time_average, TimeAverageAccumulator):
                raise ValueError("time_average: an accumulator of HermanKlukPropagator.time_average() is expected")
            time_average._check_run(self, dt)
            hooks.append((_TIME_AVERAGE, time_average))
        self._remember_nac(potential)
        own = slots is None
        if standard_errors and not own:
            raise ValueError("standard_errors=True returns the errors of run()'s own slots: pass moments= together with slots")
        if own:
            slots = torch.zeros((nt, 5), dtype=F64, device=self.device)
            if standard_errors and moments is None:
                moments = torch.zeros((nt, 6), dtype=F64, device=self.device)
        rows = self._rows(self.device, nt, slots, moments, blocks, **bufs, **counts)
        t0 = self.t
        fused = (hasattr(potential, "_descriptor") and not hasattr(potential, "_gdml_model")
                 and not hasattr(potential, "_qff_model") and self.dim <= 64
                 and self._nac_generic is None)
        desc = self._potential_descriptor(potential, dt) if fused else None
        if fused and not hooks and self._whole_loop_applies(desc):
            # separable potential, diagonal widths, D <= 12: the whole loop as ONE launch (sc_hk_run; it exports no per-step state
            # for the targets of a cross-correlation, for operators or for a time-average accumulator)
            self._run_whole_loop(desc, dt, nt, rows, potential)
        elif (use_graph and fused and nt > 2 and not getattr(self, "profile_step_kernel", False) and not self.kernel_timing
              and self._modal_step_constants(potential, desc, dt) is None):
            # (the normal-mode step runs the plain loop: its first step may change the basis of the blocks)
            self._run_graph(potential, dt, nt, desc, rows)
        else:
            pairs = fused and nt >= 2 and self._multi_applies(desc)
            kmax = self._visit_steps_for(desc) if pairs else 1
            k = 0
            while k < nt:
                self._launch_correlate(rows.row(k), per_trajectory=False, families=hooks)
                ks = min(kmax, nt - k) if pairs else 1       # never a visit longer than the steps left
                if ks == 2:
                    # TWO time steps per visit of a trajectory (sc_hk_step_multi): the second step's loads of the monodromy blocks
                    # hit the memory-side cache instead of HBM; its correlation terms come from the state between the two steps
                    self._launch_step_pair(desc, dt)
                    self._launch_correlate(rows.row(k + 1), self._multi["state_mid"], per_trajectory=False, families=hooks,
                                           time=self.t + dt)
                    self.t += dt
                    self.t += dt
                    k += 2
                elif ks > 2:
                    # three or four (sc_hk_step_visit): the blocks leave and reach HBM once per visit; row k + j of the slots, moments
                    # and blocks comes from the j-th intermediate state
                    self._launch_step_visit(desc, dt, ks)
                    t_mid = self.t
                    for j in range(1, ks):
                        t_mid += dt                          # the clock of the j-th intermediate state, accumulated as self.t is
                        self._launch_correlate(rows.row(k + j), self._multi["states_mid"][j - 1], per_trajectory=False,
                                               families=hooks, time=t_mid)
                    for _ in range(ks):
                        self.t += dt
                    k += ks
                else:
                    self._launch_step(potential, dt, desc=desc, remembered=True)
                    self.t += dt
                    k += 1
        self._corr_step = -1
        if not own:
            return None
        self.synchronize()
        tail = ()
        for fam, _ in families:
            X, sigma_X = self.finalize_cross(bufs[fam.row or fam.field][:nt], t0, dt, energy0_es, self._ntraj_norm)
            tail = tail + ((X, sigma_X) if standard_errors else (X,))
        if standard_errors:
            return (self.finalize_slots(slots, t0, dt, energy0_es)
                    + self.finalize_moments(slots, moments, t0, dt, energy0_es, self._ntraj_norm) + tail)
        return self.finalize_slots(slots, t0, dt, energy0_es) + tail

    def standard_errors(self, energy0_es=0.0):
        """(sigma_C, sigma_k) of the current step: the Monte-Carlo standard errors sigma_Re + i sigma_Im of autocorrelation() and
        ic_correlation() at this time (the step-by-step counterpart of run(..., standard_errors=True)).  sigma_k is 0 until the
        coupling is known (call ic_correlation(potential) first).  Synchronises."""
        slot = torch.zeros((1, 5), dtype=F64, device=self.device)
        mom = torch.zeros((1, 6), dtype=F64, device=self.device)
        self._launch_correlate(self._rows.single(slot, mom))
        self.synchronize()
        sc, sk = self.finalize_moments(slot, mom, self.t, 0.0, energy0_es, self._ntraj_norm)
        return complex(sc[0]), complex(sk[0])

    _rows = _StepRows               # widths, strides and validation of the output buffers of run()
    _whole_loop_ok = True           # WM needs its own per-step kernel between the steps
    _cross_ok = True                # WM has per-trajectory widths and another prefactor: no cross-correlation
    _opcorr_ok = True               # ... and no operator correlation functions

    def _whole_loop_applies(self, desc):
        # (under a discard mask the sums come from the exported terms, which the whole-loop kernels do not write)
        # (nor with a thermal ensemble: the whole-loop kernels know the one centre (q0, p0); the step loop is taken silently)
        return (self._whole_loop_ok and self._kept is None and self._thermal is None and not self.kernel_timing
                and not getattr(self, "profile_step_kernel", False) and not self._shortcut_applies(desc)
                and bool(lib.sc_hk_run_supported(desc, self._hk, self._ovl_t0)))

    # run() with a constant dense Hessian: from this many steps on the loop runs in normal-mode coordinates (sc_hk_run_modal; the two
    # changes of basis of the monodromy blocks cost about as much as four steps of the product with Phi)
    normal_modes_from = 16

    def _modal_constants(self, potential, desc, dt):
        """transformed prefactor constants and per-mode step matrices for sc_hk_run_modal, or None where it does not apply"""
        if (desc.kind != _lib.SC_POT_HARMONIC_DENSE or self._pre.diag or not hasattr(potential, "_normal_modes")
                or not self._hk.real_lr or not lib.sc_hk_run_modal_supported(desc, self._hk, self._ovl_t0)):
            return None
        cache = self.__dict__.setdefault("_modal_cache", {})
        key = (float(dt), potential.hess0.numpy().tobytes(), potential._masses.numpy().tobytes())      # the VALUES: edited in place = new key
        hit = cache.get(key)
        if hit is not None:
            return hit
        A, B, Ainv, Binv, phi = potential._normal_modes(dt)
        dev = self.device
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        L1, L2, R1, R2 = (m.real.numpy() for m in (self._pre.L1, self._pre.L2, self._pre.R1, self._pre.R2))
        consts = [t((L1 @ A).astype(np.complex128)), t((L2 @ B).astype(np.complex128)),
                  t((Ainv @ R1).astype(np.complex128)), t((Binv @ R2).astype(np.complex128))]
        hk = sc_hk_consts(dim=self.dim, dprime=self._pre.dprime, diag=0, real_lr=1,
                          L1=ptr(consts[0]), L2=ptr(consts[1]), R1=ptr(consts[2]), R2=ptr(consts[3]))
        hit = {"hk": hk, "consts": consts, "phi": t(phi), "A": t(A), "B": t(B), "Ainv": t(Ainv), "Binv": t(Binv)}
        cache.clear()
        cache[key] = hit
        return hit

    def _to_normal_modes(self, modal, forward, state=None):
        """monodromy blocks <-> normal-mode coordinates, in place: Mqq~ = A^-1 Mqq A, Mqp~ = A^-1 Mqp B, Mpq~ = B^-1 Mpq A, Mpp~ = B^-1 Mpp B
        (``state``: a copy of the engine state whose ``mono`` points elsewhere; default the state itself)"""
        if "stacks" not in modal:
            A, B, Ai, Bi = modal["A"], modal["B"], modal["Ainv"], modal["Binv"]
            modal["stacks"] = {True: (torch.stack((Ai, Ai, Bi, Bi)).contiguous(), torch.stack((A, B, A, B)).contiguous()),
                               False: (torch.stack((A, A, B, B)).contiguous(), torch.stack((Ai, Bi, Ai, Bi)).contiguous())}
        left, right = modal["stacks"][forward]
        check(lib.sc_mono_similarity(self._state if state is None else state, ptr(left), ptr(right), self._stream()))

    # step() / run() with a constant dense Hessian and these D take the normal-mode step kernel (sc_hk_step_modal)
    modal_step_dims = (17, 64)

    def _modal_step_constants(self, potential, desc, dt):
        """transformed prefactor constants, per-mode step matrices and the change of basis for sc_hk_step_modal, or None where it
        does not apply.  Diagonal widths enter as dense diagonal L, R (L1 = diag st, L2 = diag 1/st, R1 = diag 1/si, R2 = diag si)."""
        lo, hi = self.modal_step_dims
        if (desc.kind != _lib.SC_POT_HARMONIC_DENSE or not lo <= self.dim <= hi or not hasattr(potential, "_normal_modes")
                or not (self._pre.diag or self._hk.real_lr)):
            return None
        key = (float(dt), potential.hess0.numpy().tobytes(), potential._masses.numpy().tobytes())      # the VALUES: edited in place = new key
        hit = self._modal_step_cache.get(key)
        if hit is None:
            A, B, Ainv, Binv, phi = potential._normal_modes(dt)
            if self._pre.diag:
                st, si = self._pre.st.numpy(), self._pre.si.numpy()
                L1, L2, R1, R2, dprime = np.diag(st), np.diag(1.0 / st), np.diag(1.0 / si), np.diag(si), self.dim
            else:
                L1, L2, R1, R2 = (m.real.numpy() for m in (self._pre.L1, self._pre.L2, self._pre.R1, self._pre.R2))
                dprime = self._pre.dprime
            dev = self.device
            t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
            consts = [t((L1 @ A).astype(np.complex128)), t((L2 @ B).astype(np.complex128)),
                      t((Ainv @ R1).astype(np.complex128)), t((Binv @ R2).astype(np.complex128))]
            hk = sc_hk_consts(dim=self.dim, dprime=dprime, diag=0, real_lr=1,
                              L1=ptr(consts[0]), L2=ptr(consts[1]), R1=ptr(consts[2]), R2=ptr(consts[3]))
            probe = sc_state.from_buffer_copy(self._state)
            probe.mono_layout = _lib.SC_MONO_ROWMAJOR
            ok = bool(lib.sc_hk_step_modal_supported(desc, probe, hk))
            hit = {"ok": ok, "hk": hk, "consts": consts, "phi": t(phi), "A": t(A), "B": t(B), "Ainv": t(Ainv), "Binv": t(Binv),
                   "basis": key[1:]}
            self._modal_step_cache.clear()             # the basis the blocks are in stays alive in _modal_basis
            self._modal_step_cache[key] = hit
        return hit if hit["ok"] else None

    def _enter_modal(self, modal):
        """bring the monodromy blocks into the normal-mode coordinates of `modal` (from Cartesian or from another basis)"""
        cur = self._modal_basis
        if cur is not None and cur["basis"] == modal["basis"]:
            self._modal_basis = modal
            return
        self._leave_modal()
        self._to_normal_modes(modal, forward=True)
        self._modal_basis = modal

    def _leave_modal(self):
        """monodromy blocks back to Cartesian coordinates (everything but sc_hk_step_modal reads and writes them there)"""
        if self._modal_basis is not None:
            self._to_normal_modes(self._modal_basis, forward=False)
            self._modal_basis = None

    def _run_whole_loop(self, desc, dt, nt, rows, potential=None):
        self._leave_modal()
        if desc.kind not in _lib.SEPARABLE_KINDS:
            self._blocks_structurally_diagonal = False
        self._sync_dense_mono(leave_diagonal=True)
        self._set_mono_layout(_lib.SC_MONO_ROWMAJOR)
        # per-step partial sums of every wavefront: 40 sc_hk_run_slots bytes per step; long runs go in launches of <= 512 steps
        # (<= 84 MB of partials at 4096 slots, reused: the launches are ordered on the stream), the state stays on the device
        # in between and is read / written once per launch (<= 1 KB per trajectory at D <= 12: negligible against 512 steps)
        chunk = min(nt, 512)
        mom = rows.moments is not None
        partials = torch.empty(lib.sc_hk_run_scratch_doubles(self.ntraj, self.dim, chunk, int(mom)), dtype=F64, device=self.device)
        nac = self._nac
        modal = self._modal_constants(potential, desc, dt) if nt >= self.normal_modes_from else None
        if modal is not None:
            self._to_normal_modes(modal, forward=True)
        for k0 in range(0, nt, chunk):
            k = min(chunk, nt - k0)
            first = rows.row(k0)              # this launch fills the piece of the buffers from step k0 on
            tail = (ptr(partials), first.slot, ptr(self._elog), self._stream())
            head = (self._ovl_t0, nac, ptr(self._vi), ptr(self.probi), ptr(self._nacq) if nac is not None else None, self._mc_norm(), dt, k)
            if mom:
                tail = tail[:3] + (C_void(first.moments), tail[3])
            if modal is not None:
                run = lib.sc_hk_run_modal_m if mom else lib.sc_hk_run_modal
                check(run(desc, self._state, modal["hk"], *head, ptr(modal["phi"]), *tail))
            else:
                run = lib.sc_hk_run_m if mom else lib.sc_hk_run
                check(run(desc, self._state, self._hk, *head, *tail))
            if first.blocks is not None:
                # block sums of this launch's per-wavefront partials, before the next launch reuses the scratch
                out, nblocks = first.blocks
                check(lib.sc_hk_run_blocks(ptr(partials), self.ntraj, self.dim, k, nblocks, C_void(out), self._stream()))
        if modal is not None:
            self._to_normal_modes(modal, forward=False)
        self._run_scratch = partials          # alive until the stream has consumed it
        self._nsteps += nt
        for _ in range(nt):
            self.t += dt                      # accumulated as the reference's loop does (propagators.py:655)

    _multi_ok = True                # WM needs its own kernel after every single step
    pair_steps = True               # run(): two time steps per visit where sc_hk_step_multi applies (False: one launch per step)
    # run(): the MAXIMUM number of time steps per visit (sc_hk_step_visit; 2 = pairs only, the behaviour before visits; at most 4).
    # Three is what was measured to be fastest at n = 1e5 for every 32 < D <= 64 (four is slower than three: every further sub-step
    # redoes one more rotation and the kernel is bound by FP64 issue; docs/NOTEBOOK.md section 9.3); D <= 32 has no kernel for more
    # than two.  Longer visits are taken only where the monodromy blocks of the ensemble are larger than the 256 MB memory-side
    # cache: the gain is HBM traffic, and a smaller state never leaves the cache between two steps
    visit_steps = 3
    visit_min_bytes = 256 << 20

    def _multi_applies(self, desc):
        """two time steps per visit (sc_hk_step_multi): separable potential, diagonal widths, 16 < D <= 64 (the tiled fast path),
        and blocks that are still diagonal -- an intermediate determinant with a weak pivot could not be repaired"""
        if not (self._multi_ok and self.pair_steps and self._blocks_structurally_diagonal and self._nac_generic is None
                and not self._shortcut_applies(desc) and self._fast_path_layout(desc) == _lib.SC_MONO_TILED16):
            return False
        probe = sc_state.from_buffer_copy(self._state)
        probe.mono_layout = _lib.SC_MONO_TILED16
        return bool(lib.sc_hk_step_multi_supported(desc, probe, self._hk))

    def _visit_steps_for(self, desc):
        """largest number of time steps per visit run() may take: ``visit_steps``, capped by the size of the state
        (``visit_min_bytes``) and by what the library has for this D"""
        ks = int(self.visit_steps) if 32 * self.dim * self.dim * self.ntraj >= self.visit_min_bytes else 2
        probe = sc_state.from_buffer_copy(self._state)
        probe.mono_layout = _lib.SC_MONO_TILED16
        while ks > 2 and not lib.sc_hk_step_visit_supported(desc, probe, self._hk, ks):
            ks -= 1
        return max(ks, 2)

    def _visit_scratch(self, ks):
        """scratch of sc_hk_step_multi / sc_hk_step_visit for up to `ks` steps per visit: work [ks], epart [ks], and the ks - 1
        intermediate states qp / act / c2 / sgn with one sc_state view each (``states_mid``; ``state_mid`` is the first)"""
        n, d, dev = self.ntraj, self.dim, self.device
        m = self._multi
        if m is not None and m["ks"] >= ks:
            return m
        grid = self._gstep
        bufs = {"ks": ks, "work": torch.empty((ks, n, 4, d), dtype=F64, device=dev),
                "qp": torch.empty(((ks - 1) * n, 2 * d), dtype=F64, device=dev),
                "act": torch.empty((ks - 1) * n, dtype=F64, device=dev), "c2": torch.empty((ks - 1) * n, dtype=C128, device=dev),
                "sgn": torch.empty((ks - 1) * n, dtype=F64, device=dev),
                "bad": m["bad"] if m is not None else torch.zeros(1, dtype=torch.int32, device=dev),
                "epart": torch.zeros((ks, grid), dtype=F64, device=dev)}
        bufs["ms"] = sc_multi_scratch(work=ptr(bufs["work"]), qp_mid=ptr(bufs["qp"]), act_mid=ptr(bufs["act"]), c2_mid=ptr(bufs["c2"]),
                                      sgn_mid=ptr(bufs["sgn"]), unrepaired=ptr(bufs["bad"]))
        mids = []
        for j in range(ks - 1):
            mid = sc_state.from_buffer_copy(self._state)
            mid.qp, mid.act = ptr(bufs["qp"][j * n:]), ptr(bufs["act"][j * n:])
            mid.c2, mid.sgn = ptr(bufs["c2"][j * n:]), ptr(bufs["sgn"][j * n:])
            mids.append(mid)
        bufs["states_mid"], bufs["state_mid"] = mids, mids[0]
        if m is not None:
            bufs["retired"] = m              # launches on the stream may still use the smaller scratch
        self._multi = bufs
        return bufs

    def _launch_step_pair(self, desc, dt):
        self._launch_step_visit(desc, dt, 2)

    def _launch_step_visit(self, desc, dt, ks):
        """`ks` time steps in one visit of every trajectory: 2 = sc_hk_step_multi, 3 and 4 = sc_hk_step_visit"""
        n = self.ntraj
        m = self._visit_scratch(ks)
        s = self._stream()
        self._leave_modal()
        self._sync_dense_mono(leave_diagonal=True)
        self._set_mono_layout(_lib.SC_MONO_TILED16)
        for mid in m["states_mid"]:
            mid.mono_layout = _lib.SC_MONO_TILED16
        timed = getattr(self, "profile_step_kernel", False)
        if timed:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        if ks == 2:
            with self._timed("hk_step_pair"):
                check(lib.sc_hk_step_multi(desc, self._state, self._hk, m["ms"], dt, ptr(m["epart"]), s))
        else:
            with self._timed("hk_step_visit"):
                check(lib.sc_hk_step_visit(desc, self._state, self._hk, m["ms"], dt, ptr(m["epart"]), ks, s))
        if timed:
            e1.record()
            self.__dict__.setdefault("_step_events", []).append((e0, e1, ks))
        for sub in range(ks):
            check(lib.sc_energy_guard(C_void(m["epart"].data_ptr() + 8 * sub * self._gstep), self._gstep, float(n), ptr(self._elog), s))
        self._nsteps += ks

    def _run_graph(self, potential, dt, nt, desc, rows):
        """first iteration eagerly (lazy set-up, layout conversion), then one captured iteration replayed nt - 1 times"""
        base = rows.row(0)
        cursor = torch.zeros(1, dtype=torch.int64, device=self.device)

        def iteration():
            self._launch_correlate(base, cursor=cursor, per_trajectory=False)
            self._launch_step(potential, dt, desc=desc, remembered=True)
        iteration()
        graph = torch.cuda.CUDAGraph()
        steps_before = self._nsteps
        with torch.cuda.graph(graph):
            iteration()                      # recorded, not executed
        self._nsteps = steps_before + 1      # the host-side bookkeeping of a captured iteration ran once ...
        graph.replay()
        for _ in range(nt - 2):
            graph.replay()
            self._nsteps += 1                # ... and is repeated here for every further replay
        for _ in range(nt):
            self.t += dt                      # accumulated as the reference's loop does (propagators.py:655)
        if hasattr(self, "_wm_step"):
            self._wm_step = self._nsteps      # the WM terms of the current state were produced by the last replay
        self._graph = graph                  # keeps the captured launch parameters alive until the work has run

    @staticmethod
    def block_counts(n, B):
        """trajectories per block of a rank that holds ``n`` trajectories (hostmath.block_counts; sharded: add over the ranks)"""
        return hostmath.block_counts(n, B)

    @staticmethod
    def finalize_blocks(blocks, t0, dt, energy0_es):
        """(C_blocks, k_blocks), complex (nt, B): the block sums of run(..., blocks=...) with the dynamical phase of finalize_slots
        applied; their sums over the blocks are the C and k of finalize_slots"""
        raw = blocks.detach().cpu().numpy() if isinstance(blocks, torch.Tensor) else np.asarray(blocks)
        times = t0 + hostmath.time_grid(raw.shape[0], dt)
        phase = np.exp(1j / hbar * times * energy0_es)[:, None]
        return (raw[:, :, 0] + 1j * raw[:, :, 1]) * phase, (raw[:, :, 2] + 1j * raw[:, :, 3]) * phase

    @staticmethod
    def finalize_slots(slots, t0, dt, energy0_es):
        """apply the dynamical phase e^{i t E0/hbar} (reference propagators.py:841, 906) on the host"""
        raw = slots.detach().cpu().numpy()
        times = t0 + hostmath.time_grid(raw.shape[0], dt)
        phase = np.exp(1j / hbar * times * energy0_es)
        return (raw[:, 0] + 1j * raw[:, 1]) * phase, (raw[:, 2] + 1j * raw[:, 3]) * phase

    @staticmethod
    def phased_moments(slots, moments, t0, dt, energy0_es):
        """(C', k', M_C', M_k'): the phased means of finalize_slots and the second-moment sums (S_rr, S_ii, S_ri) of the phased
        terms, rows (nt, 3) -- the rotation is exact because the phase is the same for every trajectory"""
        C, k = HermanKlukPropagator.finalize_slots(slots, t0, dt, energy0_es)
        m = moments.detach().cpu().numpy() if isinstance(moments, torch.Tensor) else np.asarray(moments)
        m = m[:C.shape[0]]
        theta = (t0 + hostmath.time_grid(C.shape[0], dt)) * energy0_es / hbar
        return C, k, hostmath.rotate_second_moments(m[:, 0:3], theta), hostmath.rotate_second_moments(m[:, 3:6], theta)

    @staticmethod
    def finalize_moments(slots, moments, t0, dt, energy0_es, ntraj_norm):
        """standard errors (sigma_C, sigma_k) of the phased means, sigma_Re + i sigma_Im per step, from the raw slot sums and the
        moment sums of run(..., moments=...) (summed over ranks when sharded); ntraj_norm = N of the Monte-Carlo weight 1/N"""
        C, k, mC, mk = HermanKlukPropagator.phased_moments(slots, moments, t0, dt, energy0_es)
        return hostmath.standard_errors(C, mC, ntraj_norm), hostmath.standard_errors(k, mk, ntraj_norm)

    # ------------------------------------------------------------------ data access (reference :914-948)
    @property
    def y(self):
        """state in the reference's layout: rows (q, p, Mqq, Mqp, Mpq, Mpp, S), trajectories fastest"""
        d, n = self.dim, self.ntraj
        out = torch.empty((2 * d + 4 * d * d + 1, n), dtype=F64, device=self.device)
        self._sync_dense_mono()
        self._set_mono_layout(_lib.SC_MONO_ROWMAJOR)
        self._leave_modal()
        check(lib.sc_state_to_reference(self._state, ptr(out), self._stream()))
        return out

    @y.setter
    def y(self, value):
        value = torch.as_tensor(value, dtype=F64).to(self.device).contiguous()
        d, n = self.dim, self.ntraj
        assert value.shape == (2 * d + 4 * d * d + 1, n)
        self._state.mono_layout = _lib.SC_MONO_ROWMAJOR          # everything in mono is overwritten ...
        self._modal_basis = None                                 # ... with Cartesian blocks
        check(lib.sc_state_from_reference(ptr(value), self._state, self._stream()))
        torch.cuda.current_stream(self.device).synchronize()     # `value` may be a temporary
        self._corr_step = -1
        self._wm_export_step = -1
        # the new monodromy blocks may or may not be diagonal: keep the shortcut only if they are
        diag = torch.diagonal(self._mono, dim1=2, dim2=3)
        self._mono_stale = False
        self._mono_is_diag = bool(torch.count_nonzero(self._mono) == torch.count_nonzero(diag))
        self._blocks_structurally_diagonal = self._mono_is_diag
        if self._mono_is_diag:
            self._mdiag.copy_(diag)

    @property
    def c(self):
        """unsigned prefactor sqrt(c2) (principal branch), as the reference's attribute"""
        return torch.sqrt(self._c2)

    def initial_positions_and_momenta(self):
        return torch.split(self.zi, [self.dim, self.dim])

    def current_positions_and_momenta(self):
        qp = self._qp.t()
        return qp[:self.dim], qp[self.dim:]

    def classical_action(self):
        return self._act

    def monodromy_matrices(self):
        # (n, D, D) -> (D, D, n) views
        self._sync_dense_mono()
        self._set_mono_layout(_lib.SC_MONO_ROWMAJOR)
        self._leave_modal()
        return tuple(self._mono[:, k].permute(1, 2, 0) for k in range(4))

    def symplectic_deviation(self, scale=None, per_block=False):
        """Distance of every trajectory's monodromy matrix from the symplectic condition M^T J M = J (not in the reference;
        DESIGN.md section 4.10): the integration error of the fixed RK4 step, trajectory by trajectory.

        Returns a device tensor (n,), the largest element of the three blocks E1 = Mqq^T Mpq - Mpq^T Mqq,
        E2 = Mqq^T Mpp - Mpq^T Mqp - 1, E3 = Mqp^T Mpp - Mpp^T Mqp in the scaled coordinates q_a sigma_a, p_a / sigma_a -- or, with
        ``per_block``, the three maxima (n, 3).  ``scale`` = sigma, a positive vector of length D; the default sqrt(diag Gamma_t),
        the width of the propagated Gaussians, makes all three blocks of a harmonic mode O(1).  A trajectory with a non-finite
        monodromy element reports +inf.  No host synchronisation; the state (storage order and basis of the blocks included) is not
        changed: the steps that follow give the bits they would have given without the check."""
        default = scale is None
        scale = self.__dict__.get("_width_scale") if default else torch.as_tensor(scale, dtype=F64)
        if scale is None:
            scale = torch.sqrt(torch.diagonal(self._Gt))
        if scale.shape != (self.dim,):
            raise ValueError(f"scale should have shape ({self.dim},), got {tuple(scale.shape)}")
        if scale.device.type == "cpu" and not bool(((scale > 0) & torch.isfinite(scale)).all()):
            raise ValueError("scale has to be positive and finite (a mode of zero width needs an explicit scale)")
        scale = scale.to(self.device).contiguous()
        if default:
            self._width_scale = scale     # Gamma_t is fixed at construction: uploaded once
        self._sync_dense_mono()           # fold in the diagonals the separable shortcut advanced
        state = self._state               # the storage order stays what it is: the kernels read either
        if self._modal_basis is not None:
            # Blocks in normal-mode coordinates (constant dense Hessian): the check needs the Cartesian ones, but transforming the
            # state back and forth would change the last bits of every later step.  It looks at a Cartesian COPY (4 D^2 doubles
            # per trajectory for the duration of the call) and leaves the state in its basis.
            cartesian = self._mono.clone()
            state = sc_state.from_buffer_copy(self._state)
            state.mono = cartesian.data_ptr()
            self._to_normal_modes(self._modal_basis, forward=False, state=state)
        dev = torch.empty((self.ntraj, 3), dtype=F64, device=self.device)
        with self._timed("symplectic_deviation"):
            check(lib.sc_symplectic_deviation(state, ptr(scale), ptr(dev), self._stream()))
        return dev if per_block else dev.max(dim=1).values

    def discard_nonsymplectic(self, tolerance, scale=None):
        """Discard every trajectory whose monodromy matrix has left the symplectic condition (not in the reference; DESIGN.md
        section 4.11): runs ``symplectic_deviation(scale)`` and clears the bit of every still-kept trajectory whose deviation
        eps_i is not <= ``tolerance`` (+inf and NaN included).  Returns the eps tensor (n,) it judged.  No host synchronisation.

        The mask is sticky -- only new initial conditions bring a trajectory back -- and the state kernels do not know it: a
        discarded trajectory is still propagated, ``y``, ``c2`` and the branch trackers are what they would have been.

        The estimator: a discarded trajectory is a sample of value ZERO, N does not change.  From the mark on ``autocorrelation()``,
        ``ic_correlation()``, ``standard_errors()`` and ``run()`` (slots, moments, blocks) sum the per-trajectory terms over
        ``kept`` with the unchanged weights 1/(N prob_i), so the standard errors and the batch-means errors, with their unchanged
        N and block counts, are the errors of exactly this estimator.  Who prefers the self-normalised estimate multiplies C and k
        by N / kept_count() of that time; its error is NOT what the moments and blocks estimate, which is why it is not the
        default.  Until the first call no mask exists and every route runs the launches it always ran; afterwards ``run()`` goes
        step by step (pairs and visits included, never the one-launch loop) and refuses ``use_graph=True``.

        Works wherever ``symplectic_deviation`` works (row-major and tiled blocks, the normal-mode basis).  Position-dependent
        derivative couplings are not supported under a mask: ``NotImplementedError``."""
        tol = float(tolerance)
        if not tol > 0.0:
            raise ValueError(f"tolerance has to be positive, got {tolerance!r}")
        if self._nac_generic is not None:
            raise NotImplementedError("discard_nonsymplectic is not available with position-dependent derivative couplings: their "
                                      "k_ic terms are formed outside the masked reduction")
        dev = self.symplectic_deviation(scale, per_block=True)
        if self._kept is None:
            self._kept = torch.ones(self.ntraj, dtype=torch.uint8, device=self.device)
            self._discarded_at = torch.full((self.ntraj,), -1, dtype=torch.int32, device=self.device)
            self._kept_count = torch.zeros(1, dtype=torch.int64, device=self.device)
        check(lib.sc_discard_mark(ptr(dev), self.ntraj, tol, self._nsteps, ptr(self._kept), ptr(self._discarded_at),
                                  ptr(self._kept_count), self._stream()))
        self._corr_step = -1                  # the sums of the current step were formed under the old mask
        return dev.max(dim=1).values

    @property
    def kept(self):
        """bool tensor (n,): False for the trajectories discard_nonsymplectic has discarded; all True before any mark"""
        if self._kept is None:
            return torch.ones(self.ntraj, dtype=torch.bool, device=self.device)
        return self._kept.bool()

    @property
    def discarded_at(self):
        """int32 tensor (n,): the step count of the mark that discarded the trajectory, -1 = kept"""
        if self._discarded_at is None:
            return torch.full((self.ntraj,), -1, dtype=torch.int32, device=self.device)
        return self._discarded_at.clone()

    def kept_count(self):
        """number of trajectories still kept (a Python int; synchronises)"""
        return self.ntraj if self._kept_count is None else int(self._kept_count.item())

    def semiclassical_prefactor(self):
        return self._sgn * torch.sqrt(self._c2)

    def coefficients(self):
        """expansion coefficients v_i of the wavefunction in the coherent states (reference propagators.py:657-686).
        The discard mask (discard_nonsymplectic) is ignored: discarded trajectories keep their coefficients."""
        v = self.semiclassical_prefactor() * torch.exp(1j / hbar * self._act) * self._vi
        return v / (self._mc_norm() * self.probi)

    def _norm_group(self, across_ranks, group):
        """process group of a cross-rank norm(), or the LOCAL sentinel.  Cross-rank is OPT-IN: a process group that merely
        exists (ranks propagating independent ensembles, rank-0-only logging) must not turn norm() into a collective."""
        from . import distributed as Dm
        if not across_ranks and group is None:
            return Dm.LOCAL
        if Dm._active(group):
            # every rank has to hold one shard of ONE ensemble weighted with the global N (initial_conditions(ntraj_total=...))
            count = torch.tensor([float(self.ntraj)], dtype=F64, device=self.device)
            Dm.all_reduce_sum(count, group)
            if int(round(float(count.item()))) != int(self._ntraj_norm):
                raise ValueError(f"norm(across_ranks=True): the ranks hold {int(count.item())} trajectories together but the "
                                 f"Monte-Carlo weight is 1/{self._ntraj_norm}: the ranks do not share one ensemble "
                                 "(pass ntraj_total = the global count to initial_conditions, or take the rank-local norm())")
        return group

    def norm(self, across_ranks=False, group=None):
        """|psi| = sqrt(sum_ij v_i^* <q_i,p_i,Gamma_t|q_j,p_j,Gamma_t> v_j), O(n^2) (reference propagators.py:734-782).

        The pair sum runs in ``sc_pair_sum_rect``; the host only packs the operands: positions are centred (the overlaps
        depend on differences) so that the per-trajectory and the cross terms of the exponent stay small.

        By default the norm of THIS rank's trajectories with this rank's weights (no communication).
        ``across_ranks=True`` (or an explicit ``group``) -- every rank of the group holds one shard of one ensemble with
        the global N as ``ntraj_total`` and every rank makes the call: the ket operands of all ranks are all-gathered,
        every rank sums ITS bras against ALL kets and one all-reduce adds the partial sums -- every rank returns the norm
        of the whole wavefunction.

        The discard mask (discard_nonsymplectic) is ignored: discarded trajectories contribute as ever.
        """
        from . import distributed as Dm
        self._refuse_thermal("norm()", "it describes one pure state, the trajectories belong to a mixture")
        group = self._norm_group(across_ranks, group)
        dev, d, n = self.device, self.dim, self.ntraj
        oc = hostmath.OverlapConstants(self._Gt, self._Gt)
        A, B, Cm = (m.to(dev) for m in (oc.A, oc.B, oc.C))
        # a centre all ranks agree on: the mean position of the whole ensemble
        qsum = torch.cat((self._qp[:, :d].sum(0), torch.tensor([float(n)], dtype=F64, device=dev)))
        Dm.all_reduce_sum(qsum, group)
        q = self._qp[:, :d] - (qsum[:d] / qsum[d]).unsqueeze(0)
        p = self._qp[:, d:]
        Aq, Bp, Cp = q @ A.T, p @ B.T / hbar ** 2, p @ Cm.T / hbar
        # exponent_ij = rs_i + rs_j + X1_i.Y1_j + i (ib_i + ik_j + X2_i.Y2_j)   (propagators.py:232-237 expanded)
        X1 = torch.cat((q, p), 1).contiguous()
        Y1 = torch.cat((Aq, Bp), 1).contiguous()
        X2 = torch.cat((q, Cp, q), 1).contiguous()
        Y2 = torch.cat((p / hbar, -q, -Cp), 1).contiguous()
        rs = (-0.5 * (q * Aq).sum(1) - 0.5 * (p * Bp).sum(1)).contiguous()
        cc = (q * Cp).sum(1)
        ib = cc.contiguous()
        ik = (cc - (p * q).sum(1) / hbar).contiguous()
        v = self.coefficients()
        wb, wk = (oc.fac * v.conj()).contiguous(), v.contiguous()
        # kets of the whole ensemble (this rank's own when there is one rank)
        ket = torch.cat((Y1, Y2, rs.unsqueeze(1), ik.unsqueeze(1), torch.view_as_real(wk)), 1)
        ket = Dm.all_gather_rows(ket, group)
        nj = ket.shape[0]
        Y1j, Y2j = ket[:, :2 * d].contiguous(), ket[:, 2 * d:5 * d].contiguous()
        rsj, ikj = ket[:, 5 * d].contiguous(), ket[:, 5 * d + 1].contiguous()
        wkj = ket[:, 5 * d + 2:5 * d + 4].contiguous()
        tiles = lib.sc_pair_sum_rect_tiles(n, nj)
        partials = torch.empty((tiles, 4), dtype=F64, device=dev)
        slot = torch.zeros(8, dtype=F64, device=dev)
        s = self._stream()
        check(lib.sc_pair_sum_rect(ptr(X1), ptr(Y1j), 2 * d, ptr(X2), ptr(Y2j), 3 * d, ptr(rs), ptr(rsj), ptr(ib), ptr(ikj),
                                   ptr(wb), ptr(wkj), n, nj, ptr(partials), s))
        check(lib.sc_reduce_slot(ptr(partials), int(tiles), None, 0, 1.0, ptr(slot), s))
        Dm.all_reduce_sum(slot, group)
        return float(torch.sqrt(slot[0]).item())

    def _density_directions(self, directions):
        """(M, D) fp64 host tensor of the directions of reduced_density: mode indices -> unit vectors, or the vectors given"""
        d = self.dim
        arr = np.asarray(directions)
        if arr.dtype == bool or arr.size == 0:
            raise ValueError("directions: mode indices or vectors of length D are expected")
        if np.issubdtype(arr.dtype, np.integer) and arr.ndim <= 1:
            idx = arr.reshape(-1)
            if ((idx < 0) | (idx >= d)).any():
                raise ValueError(f"directions: mode index outside 0 ... {d - 1}: {idx.tolist()}")
            U = torch.zeros((idx.shape[0], d), dtype=F64)
            U[torch.arange(idx.shape[0]), torch.from_numpy(idx.astype(np.int64))] = 1.0
            return U
        U = torch.as_tensor(arr, dtype=F64)
        if U.dim() == 1:
            U = U.unsqueeze(0)
        if U.dim() != 2 or U.shape[1] != d:
            raise ValueError(f"directions: vectors of length {d} are expected, got shape {tuple(arr.shape)}")
        if not bool(torch.isfinite(U).all()):
            raise ValueError("directions: non-finite component")
        return U.contiguous()

    def reduced_density(self, directions, s):
        """Marginal density of the wavepacket along chosen directions (not in the reference):

            rho_u(s) = int |psi(x)|^2 delta(s - u.x) dx
                     = Re sum_ij v_i^* v_j O_ij (2 pi sigma^2)^-1/2 exp(-(s - mu_ij)^2 / (2 sigma^2)),
            sigma^2 = u^T B u,  mu_ij = u.(q_i + q_j) / 2 + i u^T B (p_j - p_i) / hbar,  B = (2 Gamma_t)^+,

        O_ij the overlaps and v the coefficients of ``norm()``: the integral of rho_u over s is ``norm()**2``.

        ``directions``: an int or a sequence of ints (mode indices k -> unit vectors e_k), or an array (D,) or (M, D) of real
        vectors u, not necessarily normalised (integers in a flat sequence are always mode indices).  ``s``: 1-D array of grid
        values, in any order.  Returns a real ndarray (M, ns).

        A direction has to lie in the range of Gamma_t (the marginal along a null direction of a singular Gamma_t does not
        exist): ``ValueError`` otherwise, as for a direction of the wrong length, a zero direction, a mode index out of range and
        an empty or non-finite grid.  For a singular Gamma_t the result is the real part of the formula with the
        pseudo-inverse and pseudo-determinant conventions of the overlaps.

        The pair sum runs in ``sc_density_pair_sum`` on the operands ``norm()`` packs (positions centred on the ensemble mean,
        the grid shifted by u.centre).  Rank-local: this rank's trajectories with this rank's weights, no communication.  The
        discard mask (discard_nonsymplectic) is ignored: discarded trajectories contribute as ever.  The state is not touched."""
        self._refuse_thermal("reduced_density()", "it describes one pure state, the trajectories belong to a mixture")
        dev, d, n = self.device, self.dim, self.ntraj
        U = self._density_directions(directions)
        sg = torch.as_tensor(np.asarray(s, dtype=np.float64))
        if sg.dim() != 1 or sg.shape[0] == 0:
            raise ValueError(f"s: a non-empty 1-D grid is expected, got shape {tuple(sg.shape)}")
        if not bool(torch.isfinite(sg).all()):
            raise ValueError("s: non-finite grid value")
        oc = hostmath.OverlapConstants(self._Gt, self._Gt)
        unorm = torch.linalg.norm(U, dim=1)
        if bool((unorm == 0).any()):
            raise ValueError("directions: zero vector")
        # Gamma_t Gamma_t^+ = 2 Gamma_t (2 Gamma_t)^+ = 2 C projects onto the range of Gamma_t
        outside = torch.linalg.norm(U - 2.0 * (U @ oc.C.T), dim=1) > 1.0e-8 * unorm
        if bool(outside.any()):
            raise ValueError(f"directions: direction(s) {torch.nonzero(outside).flatten().tolist()} outside the range of Gamma_t: "
                             "the marginal along a null direction does not exist")
        UB = U @ oc.B                                       # rows u^T B (B symmetric)
        sigma2 = (UB * U).sum(1)
        M, ns = U.shape[0], sg.shape[0]
        A, B, Cm = (m.to(dev) for m in (oc.A, oc.B, oc.C))
        # the operands of norm() (rank-local), packed the same way
        centre = self._qp[:, :d].sum(0) / float(n)
        q = self._qp[:, :d] - centre.unsqueeze(0)
        p = self._qp[:, d:]
        Aq, Bp, Cp = q @ A.T, p @ B.T / hbar ** 2, p @ Cm.T / hbar
        X1 = torch.cat((q, p), 1).contiguous()
        Y1 = torch.cat((Aq, Bp), 1).contiguous()
        X2 = torch.cat((q, Cp, q), 1).contiguous()
        Y2 = torch.cat((p / hbar, -q, -Cp), 1).contiguous()
        rs = (-0.5 * (q * Aq).sum(1) - 0.5 * (p * Bp).sum(1)).contiguous()
        cc = (q * Cp).sum(1)
        ib = cc.contiguous()
        ik = (cc - (p * q).sum(1) / hbar).contiguous()
        v = self.coefficients()
        wb, wk = (oc.fac * v.conj()).contiguous(), v.contiguous()
        # per direction: a = u.q / 2, b = u^T B p / hbar (rows [M][n]), 1 / (2 sigma^2) and the grid's origin u.centre
        Ud = U.to(dev)
        a = (0.5 * (Ud @ q.T)).contiguous()
        b = (UB.to(dev) @ p.T / hbar).contiguous()
        h = (0.5 / sigma2).to(dev).contiguous()
        origin = (Ud @ centre).contiguous()
        sd = sg.to(dev).contiguous()
        rows = lib.sc_density_pair_sum_rows(n, n)
        partials = torch.empty((rows, M * ns, 2), dtype=F64, device=dev)
        rho = torch.empty((M, ns, 2), dtype=F64, device=dev)
        with self._timed("reduced_density"):
            check(lib.sc_density_pair_sum(ptr(X1), ptr(Y1), 2 * d, ptr(X2), ptr(Y2), 3 * d, ptr(rs), ptr(rs), ptr(ib), ptr(ik),
                                          ptr(wb), ptr(wk), n, n, ptr(a), ptr(b), ptr(a), ptr(b), ptr(h), M, ptr(sd), ptr(origin),
                                          ns, ptr(partials), ptr(rho), self._stream()))
        return rho[:, :, 0].cpu().numpy()

    def _pair_operands(self):
        """the rank-local operands of the pair exponent as ``norm()`` packs them (positions centred on the ensemble mean):
        (X1, Y1, X2, Y2, rs, ib, ik, wb, wk) on the device"""
        dev, d, n = self.device, self.dim, self.ntraj
        oc = hostmath.OverlapConstants(self._Gt, self._Gt)
        A, B, Cm = (m.to(dev) for m in (oc.A, oc.B, oc.C))
        q = self._qp[:, :d] - (self._qp[:, :d].sum(0) / float(n)).unsqueeze(0)
        p = self._qp[:, d:]
        Aq, Bp, Cp = q @ A.T, p @ B.T / hbar ** 2, p @ Cm.T / hbar
        # exponent_ij = rs_i + rs_j + X1_i.Y1_j + i (ib_i + ik_j + X2_i.Y2_j)
        X1 = torch.cat((q, p), 1).contiguous()
        Y1 = torch.cat((Aq, Bp), 1).contiguous()
        X2 = torch.cat((q, Cp, q), 1).contiguous()
        Y2 = torch.cat((p / hbar, -q, -Cp), 1).contiguous()
        rs = (-0.5 * (q * Aq).sum(1) - 0.5 * (p * Bp).sum(1)).contiguous()
        cc = (q * Cp).sum(1)
        ib = cc.contiguous()
        ik = (cc - (p * q).sum(1) / hbar).contiguous()
        v = self.coefficients()
        return X1, Y1, X2, Y2, rs, ib, ik, (oc.fac * v.conj()).contiguous(), v.contiguous()

    def expectation(self, c=None, x=None, xx=None, p=None, pp=None, normalise=True, ex=None):
        """Expectation values of M quadratic operators in the wavepacket (not in the reference):

            A_a = c_a + x_a.x + 1/2 x^T xx_a x + p_a.p + 1/2 p^T pp_a p        (p = -i hbar d/dx; no x-p cross terms),
            E_a = <psi|A_a|psi> = sum_ij v_i^* v_j O_ij F_a,ij,      N2 = sum_ij v_i^* v_j O_ij = norm()**2,

        O_ij the overlaps and v the coefficients of ``norm()``, F_a,ij the Gaussian matrix element of A_a divided by the overlap
        (``hostmath.fold_expectation_operators``).  ``c`` (M,), ``x``, ``p`` (M, D), ``xx``, ``pp`` (M, D, D) real symmetric; any
        of them may be None (= zeros), M is taken from the ones given.  Returns ``(values, norm2)``: the complex ndarray (M,) of
        E_a / N2 -- of E_a with ``normalise=False`` -- and the float N2.  The imaginary part of the value of a Hermitian operator is
        rounding.

        For a singular Gamma_t every x_a, p_a and eigenvector of xx_a, pp_a (eigenvalues above 1e-12 of the largest) has to lie
        in the range of Gamma_t: ``ValueError`` naming the operator otherwise, as for parts whose shapes do not agree, a
        non-symmetric xx or pp and non-finite entries.  The value is then the formula with the pseudo-inverse conventions of the
        overlaps.

        ``ex=(w, a)`` adds  sum_e w_a,e exp(-a_a,e . x)  to operator a: ``w`` (M, P) real or complex, ``a``
        (M, P, D) real, M as in the other parts (which may then all be None); an operator with fewer terms has w = 0 in the others.
        Every a with w != 0 has to lie in the range of Gamma_t (``ValueError`` naming operator and term).  The exponentials of the
        trajectories' own positions are formed on the device; one that is not finite -- a trajectory far out on the repulsive wall
        -- is a ``ValueError`` naming the term.  The pair sum then runs in ``sc_pair_expect_exp``; without ``ex`` nothing changes.

        The pair sum runs in ``sc_pair_expect`` on the operands ``norm()`` packs.  Rank-local: this rank's trajectories with
        this rank's weights, no communication.  The discard mask (discard_nonsymplectic) is ignored: discarded trajectories
        contribute as ever.  No step is taken and the state is not touched.  The value is quadratic in the ensemble, not
        additive over batches: there is no hook in ``run()``."""
        self._refuse_thermal("expectation()", "it describes one pure state, the trajectories belong to a mixture")
        dev, d, n = self.device, self.dim, self.ntraj
        if ex is not None:
            if not isinstance(ex, (tuple, list)) or len(ex) != 2:
                raise ValueError("operators: ex = (w, a) with w of shape (M, P) and a of shape (M, P, D) is expected")
            euq, eup, mu = hostmath.fold_exponential_operators(ex[0], ex[1], self._Gt)
            if all(t is None for t in (c, x, xx, p, pp)):
                c = torch.zeros(mu.shape[0], dtype=F64)
        uq, up, lam, kap, R = hostmath.fold_expectation_operators(c, x, xx, p, pp, self._Gt)
        M = int(kap.shape[0])
        if ex is not None and int(mu.shape[0]) != M:
            raise ValueError(f"operators: the parts have to hold the same number M >= 1 of operators, got {M} and {int(mu.shape[0])} in ex")
        X1, Y1, X2, Y2, rs, ib, ik, wb, wk = self._pair_operands()
        # the columns a_i = uq.q_i + up.p_i from the actual positions, [M (1 + R)][n]; the kets take the conjugates
        qT, pT = self._qp[:, :d].T, self._qp[:, d:].T
        uq, up = uq.reshape(-1, d).to(dev), up.reshape(-1, d).to(dev)
        zre, zim = uq.real @ qT + up.real @ pT, uq.imag @ qT + up.imag @ pT
        za, zb = torch.complex(zre, zim).contiguous(), torch.complex(zre, -zim).contiguous()
        lam_d, kap_d = lam.reshape(-1).to(dev).contiguous(), kap.to(dev).contiguous()
        tiles = lib.sc_pair_expect_tiles(n, n)
        partials = torch.empty((max(int(tiles), 1), M + 1, 2), dtype=F64, device=dev)
        out = torch.empty(M + 1, dtype=C128, device=dev)
        if ex is not None:
            ea, eb, P = self._exponential_columns(euq, eup, mu)
        with self._timed("expectation"):
            if ex is None:
                check(lib.sc_pair_expect(ptr(X1), ptr(Y1), 2 * d, ptr(X2), ptr(Y2), 3 * d, ptr(rs), ptr(rs), ptr(ib), ptr(ik), ptr(wb),
                                         ptr(wk), n, n, ptr(za), ptr(zb), ptr(lam_d), ptr(kap_d), M, R, ptr(partials), ptr(out),
                                         self._stream()))
            else:
                check(lib.sc_pair_expect_exp(ptr(X1), ptr(Y1), 2 * d, ptr(X2), ptr(Y2), 3 * d, ptr(rs), ptr(rs), ptr(ib), ptr(ik),
                                             ptr(wb), ptr(wk), n, n, ptr(za), ptr(zb), ptr(lam_d), ptr(kap_d), M, R, ptr(ea), ptr(eb),
                                             P, ptr(partials), ptr(out), self._stream()))
        res = out.cpu().numpy()
        norm2 = float(res[M].real)
        return (res[:M] / norm2 if normalise else res[:M].copy()), norm2

    def _width_has_full_rank(self):
        """no eigenvalue of Gamma_t below the threshold of the pseudo-inverses"""
        return bool((abs(torch.linalg.eigvalsh(hostmath.as_f64(self._Gt))) > hostmath.ZERO).all())

    def wavepacket_moments(self, directions=None):
        """Centre and widths of the wavepacket along chosen directions u: a dict with ``x`` = <u.x>, ``p`` = <u.p>, ``var_x`` =
        <(u.x)^2> - <u.x>^2, ``var_p`` = <(u.p)^2> - <u.p>^2, real ndarrays (M,) of the values normalised with ``norm2`` = norm()**2,
        which comes along.  ``directions`` as in ``reduced_density``: mode indices or vectors of length D; None means the D axes,
        for a Gamma_t of full rank only (``ValueError`` otherwise: give directions in its range).  One ``expectation`` call with
        four operators per direction; what is said there about ranks, the discard mask and the state holds here."""
        self._refuse_thermal("wavepacket_moments()", "it describes one pure state, the trajectories belong to a mixture")
        d = self.dim
        if directions is None:
            if not self._width_has_full_rank():
                raise ValueError("wavepacket_moments: Gamma_t is singular, the moments along its null directions do not exist: give "
                                 "directions in the range of Gamma_t")
            U = torch.eye(d, dtype=F64)
        else:
            U = self._density_directions(directions)
            if bool((torch.linalg.norm(U, dim=1) == 0).any()):
                raise ValueError("directions: zero vector")
        Md = U.shape[0]
        zv, zm = torch.zeros((Md, d), dtype=F64), torch.zeros((Md, d, d), dtype=F64)
        uu = 2.0 * U.unsqueeze(2) * U.unsqueeze(1)          # 1/2 x^T (2 u u^T) x = (u.x)^2
        vals, norm2 = self.expectation(x=torch.cat((U, zv, zv, zv)), xx=torch.cat((zm, uu, zm, zm)),
                                       p=torch.cat((zv, zv, U, zv)), pp=torch.cat((zm, zm, zm, uu)))
        ex, exx, ep, epp = (vals[k * Md:(k + 1) * Md].real for k in range(4))
        return {"x": ex, "p": ep, "var_x": exx - ex ** 2, "var_p": epp - ep ** 2, "norm2": norm2}

    def energy_expectation(self, potential):
        """<psi| p^T m^-1 p / 2 + V(x) |psi> / norm()**2 for a potential whose Hessian is constant: ``MolecularHarmonicPotential``
        and ``MorsePotential`` with all chi = 0 (``NotImplementedError`` for every other: V is not a quadratic operator).  A float:
        the real part of one ``expectation`` value.  A singular Gamma_t is refused with ``ValueError``: the kinetic energy along
        its null directions does not exist, and projecting it is the caller's decision (``expectation`` with a projected pp)."""
        self._refuse_thermal("energy_expectation()", "it describes one pure state, the trajectories belong to a mixture")
        d = self.dim
        quad = _constant_hessian_parts(potential)
        if quad is None:
            raise NotImplementedError(f"energy_expectation: {type(potential).__name__} is not a potential with a constant Hessian "
                                      "(MolecularHarmonicPotential, MorsePotential with chi = 0): <V> is not a quadratic operator's")
        if potential.dimensions() != d:
            raise ValueError(f"energy_expectation: the potential has {potential.dimensions()} dimensions, the propagator {d}")
        if not self._width_has_full_rank():
            raise ValueError("energy_expectation: Gamma_t is singular, the kinetic energy along its null directions does not exist; "
                             "projecting it is the caller's decision (expectation() with a projected pp)")
        vals, _ = self.expectation(**_hamiltonian_operator(potential, "energy_expectation"))
        return float(vals[0].real)

    def _exponential_columns(self, uq, up, mu):
        """(ea, eb, P): the product columns of ``hostmath.fold_exponential_operators`` from the actual positions, [M P][n] complex on
        the device: ea_i = mu exp(-alpha_i), eb_j = conj(exp(-alpha_j)), alpha_i = uq.q_i + up.p_i -- n M P exponentials, not n^2"""
        dev, d = self.device, self.dim
        M, P = int(mu.shape[0]), int(mu.shape[1])
        if P == 0:
            return None, None, 0
        qT, pT = self._qp[:, :d].T, self._qp[:, d:].T
        uq, up = uq.reshape(-1, d).to(dev), up.reshape(-1, d).to(dev)
        alpha = torch.complex(uq.real @ qT + up.real @ pT, uq.imag @ qT + up.imag @ pT)
        e = torch.exp(-alpha)
        ea, eb = (mu.reshape(-1, 1).to(dev) * e).contiguous(), e.conj().resolve_conj().contiguous()
        bad = ~torch.isfinite(torch.view_as_real(ea)).all(2).all(1)
        if bool(bad.any()):
            col = int(torch.nonzero(bad)[0])
            raise ValueError(f"operators: term {col % P} of operator {col // P} of ex: exp(-a.x) is not finite at a trajectory's "
                             "position (it has run far out on the repulsive wall)")
        return ea, eb, P

    def anharmonic_energy_expectation(self, potential):
        """<psi| p^T m^-1 p / 2 + V(x) |psi> / norm()**2 on the separable anharmonic surfaces: a float, the
        real part of one ``expectation`` value with ``ex``.  ``MorsePotential`` with chi != 0: V = sum_k D_k (1 - 2 exp(-a_k x_k) +
        exp(-2 a_k x_k)) with the object's own a and D (modes with the 1e-4 fix-up included) -- D squared p-columns and 2 D
        exponentials in one operator; ``NonHarmonicPotential``: the eps Morse part as two exponentials and a constant per
        dimension, (1 - eps) x^2 / 2 as ``xx``.  For the potentials of ``energy_expectation`` its value.  sGDML and quartic force
        fields: ``NotImplementedError``.  A singular Gamma_t is refused with ``ValueError`` as there.

        V is a sum of terms of alternating sign that are each about D_k = omega / (4 chi): rounding is relative to the sum of the
        absolute terms, about 50 <V> at chi = 0.02 and 1e4 <V> at the 1e-4 fix-up."""
        from . import potentials as P
        self._refuse_thermal("anharmonic_energy_expectation()", "it describes one pure state, the trajectories belong to a mixture")
        d = self.dim
        if isinstance(potential, P.MolecularHarmonicPotential) or (isinstance(potential, P.MorsePotential) and potential._is_harmonic()):
            return self.energy_expectation(potential)
        if _morse_parts(potential) is None:
            raise NotImplementedError(f"anharmonic_energy_expectation: {type(potential).__name__} is neither a Morse-type potential "
                                      "(MorsePotential, NonHarmonicPotential) nor one with a constant Hessian: <V> has no closed form")
        if potential.dimensions() != d:
            raise ValueError(f"anharmonic_energy_expectation: the potential has {potential.dimensions()} dimensions, the propagator {d}")
        if not self._width_has_full_rank():
            raise ValueError("anharmonic_energy_expectation: Gamma_t is singular, the kinetic energy along its null directions does "
                             "not exist; projecting it is the caller's decision (expectation() with a projected pp)")
        vals, _ = self.expectation(**_hamiltonian_operator(potential, "anharmonic_energy_expectation"))
        return float(vals[0].real)

    def wavefunction(self, x):
        """frozen-Gaussian wavefunction psi(x,t) on a spatial grid x (dim,nx) -> complex ndarray (nx,)
        (reference propagators.py:688-732 with CoherentStatesWavefunction :243-292).  The discard mask (discard_nonsymplectic) is
        ignored: discarded trajectories contribute as ever."""
        self._refuse_thermal("wavefunction()", "it describes one pure state, the trajectories belong to a mixture")
        x = torch.as_tensor(x, dtype=F64)
        d, nx = x.shape
        assert d == self.dim, "spatial grid has wrong dimensions"
        dev, n = self.device, self.ntraj
        L = hostmath.psd_sqrt_real(self._Gt)                  # (x-q)^T Gt (x-q) = |L (x-q)|^2
        fac = hostmath.wavepacket_norm_factor(self._Gt)
        Ld = L.to(dev)
        q, p = self._qp[:, :d], self._qp[:, d:]
        LqT = (Ld @ q.T).contiguous()
        PT = p.T.contiguous()
        pq = ((p * q).sum(1) / hbar).contiguous()
        if hbar != 1.0:
            PT = PT / hbar
        X = x.T.contiguous().to(dev)
        Lx = (X @ Ld.T).contiguous()
        v = self.coefficients().contiguous()
        phi = torch.zeros(nx, dtype=C128, device=dev)
        check(lib.sc_grid_sum(ptr(LqT), ptr(PT), ptr(pq), ptr(v), n, d, ptr(Lx), ptr(X), nx, fac, ptr(phi),
                              self._stream()))
        return phi.cpu().numpy()

    def _get_signs_of_sqrt(self, key):
        if key != "prefactorC":
            logger.error(f"Apparently the sign of the square root of the quantity '{key}' is not being tracked.")
            raise KeyError(key)
        return self._sgn.type(C128)

    _TRACKED = {"prefactorC": ("_sgn", "_c2")}

    @property
    def sign_trackers(self):
        """the reference's bookkeeping dict (propagators.py:1006-1066): name -> {'signs': +-1 per trajectory,
        'previous': value at the last tracked step}, built from the device-resident tracker state (read-only views)"""
        return {name: {"signs": getattr(self, s).type(C128), "previous": getattr(self, z)}
                for name, (s, z) in self._TRACKED.items()}


class TimeAverageAccumulator(object):
    """What ``HermanKlukPropagator.time_average()`` returns: A [n K][NE], the pending columns G [TB][n K] of the terms, their count
    and the step counter s of the grid t_s = t_a + s dt.  Bound to the propagator and its ensemble."""

    def __init__(self, prop, energies, dt, references, max_bytes):
        try:
            E = np.array(energies, dtype=np.float64)
        except (TypeError, ValueError) as err:
            raise ValueError(f"energies: a real array (NE,) is expected ({err})")
        if E.ndim != 1 or E.shape[0] == 0:
            raise ValueError(f"energies: a non-empty one-dimensional array is expected, got shape {E.shape}")
        if not np.isfinite(E).all():
            raise ValueError("energies: non-finite entry")
        if E.shape[0] > 65535:
            raise ValueError(f"energies: NE = {E.shape[0]} outside NE <= 65535")
        dt = float(dt)
        if not (np.isfinite(dt) and dt != 0.0):
            raise ValueError(f"dt: a finite non-zero time step is expected, got {dt}")
        D = prop.dim
        if references is None:
            Q, P = prop._q0h.numpy()[None, :].copy(), prop._p0h.numpy()[None, :].copy()
        else:
            try:
                Q, P = (np.array(a, dtype=np.float64) for a in references)
            except (TypeError, ValueError) as err:
                raise ValueError(f"references: a pair (Q, P) of real arrays of shape (K, {D}) is expected ({err})")
            if Q.ndim != 2 or Q.shape != P.shape or Q.shape[1] != D or Q.shape[0] == 0:
                raise ValueError(f"references: Q and P of shape (K, {D}) with K > 0 are expected, got {Q.shape} and {P.shape}")
            if not (np.isfinite(Q).all() and np.isfinite(P).all()):
                raise ValueError("references: non-finite entry")
        K, NE, n = int(Q.shape[0]), int(E.shape[0]), prop.ntraj
        if K > 64:
            raise ValueError(f"references: K = {K} outside K <= 64 (one tile column of the terms kernel)")
        need = 16 * n * K * NE
        if need > max_bytes:
            raise ValueError(f"the accumulator A (n K, NE) = ({n} x {K}, {NE}) complex takes {need} bytes, more than max_bytes = "
                             f"{int(max_bytes)}: fewer energies or reference states, or a smaller batch")
        dev = prop.device
        cc = prop._cross_constants()
        Qt, Pt = torch.from_numpy(Q), torch.from_numpy(P)
        self._refs = torch.cat((Qt @ cc["La"].T, Pt @ cc["Lb"].T, Qt, Pt @ cc["C"].T, Pt), 1).contiguous().to(dev)
        self.TB = int(lib.sc_hk_ta_block())
        self._prop, self._qp = prop, prop._qp                      # (the ensemble: another one has other buffers)
        self.energies, self.references, self.dt, self.t_start = E, (Q, P), dt, float(prop.t)
        self.K, self.NE = K, NE
        self._E = torch.from_numpy(E).to(dev)
        self._A = torch.zeros((n * K, NE), dtype=C128, device=dev)
        self._G = torch.empty((self.TB, n * K), dtype=C128, device=dev)
        self._W = torch.empty((self.TB, NE), dtype=C128, device=dev)
        self._partials = torch.empty(max(int(lib.sc_hk_ta_finish_rows(n)) * K * NE * 2, 1), dtype=F64, device=dev)
        self.pending, self.steps = 0, 0

    @property
    def window(self):
        """T = ns dt of the steps taken so far"""
        return self.steps * self.dt

    def _check_owner(self, prop):
        if prop is not self._prop or prop._qp is not self._qp:
            raise ValueError("this time-average accumulator belongs to another propagator or to an earlier set of initial conditions")

    def _check_run(self, prop, dt):
        """run(time_average=self): refused before anything is launched"""
        self._check_owner(prop)
        if dt != self.dt:
            raise ValueError(f"time_average: the accumulator's grid has dt = {self.dt}, this run has dt = {dt}")

    def _append(self, state=None):
        """the terms of `state` (default: the propagator's current one) as column `pending`; a full block goes into A"""
        prop = self._prop
        cc = prop._cross_constants()
        b = cc["bufs"]
        with prop._timed("hk_ta_terms"):
            check(lib.sc_hk_ta_terms(prop._state if state is None else state, ptr(b[0]), ptr(b[1]), ptr(b[2]), int(cc["diag"]),
                                     cc["fac"], ptr(self._refs), self.K, ptr(prop._kept), ptr(cc["operands"]), ptr(self._G),
                                     self.pending, prop._stream()))
        self.pending += 1
        self.steps += 1
        if self.pending == self.TB:
            self._flush()

    def _flush(self):
        """the pending columns into A"""
        if self.pending == 0:
            return
        prop = self._prop
        with prop._timed("hk_ta_accumulate"):
            check(lib.sc_hk_ta_accumulate(ptr(self._G), prop.ntraj, self.K, self.pending, ptr(self._E), self.NE, self.t_start, self.dt,
                                          self.steps - self.pending, ptr(self._W), ptr(self._A), prop._stream()))
        self.pending = 0

    def add(self):
        """append the propagator's current state as the next step of the window (for callers of ``step()``: once per step, before
        it, as ``run()`` does)"""
        self._check_owner(self._prop)
        self._append()

    def raw_sums(self):
        """the sums (K, NE, 2) over this batch's trajectories of y T and (y T)^2, y_ik(e) = |A_ik(E_e)|^2 / (2 pi hbar T mc_norm
        P_i), as a NumPy array: plain sums with the global N in the weight, so the buffers of batches of one N and of ranks add;
        ``finalize_time_average`` finishes them.  Flushes the pending columns; trajectories discarded by now count as y = 0, N
        unchanged.  Synchronises; the accumulator goes on afterwards."""
        prop = self._prop
        self._check_owner(prop)
        self._flush()
        out = torch.empty((self.K, self.NE, 2), dtype=F64, device=prop.device)
        check(lib.sc_hk_ta_finish(ptr(self._A), prop.ntraj, self.K, self.NE, ptr(prop.probi), prop._mc_norm(), ptr(prop._kept),
                                  ptr(self._partials), ptr(out), prop._stream()))
        prop.synchronize()
        return out.cpu().numpy()

    def spectrum(self, standard_errors=False):
        """I (K, NE) over the window so far, or (I, sigma) with its Monte-Carlo standard errors"""
        if self.steps == 0:
            raise ValueError("the window is empty: no step has been added to the accumulator")
        I, sigma = HermanKlukPropagator.finalize_time_average(self.raw_sums(), self.window, self._prop._ntraj_norm)
        return (I, sigma) if standard_errors else I


class _KernelTimer(object):
    def __init__(self, prop, label):
        self.prop, self.label = prop, label

    def __enter__(self):
        self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.e0.record()

    def __exit__(self, *exc):
        self.e1.record()
        self.prop.__dict__.setdefault("_kernel_events", {}).setdefault(self.label, []).append((self.e0, self.e1))
        return False


class _NoTimer(object):
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NO_TIMER = _NoTimer()


def C_void(address):
    import ctypes
    return ctypes.c_void_p(int(address))


def _NULL_POT(dim):
    """descriptor for prefactor-only launches (the potential is not touched in mode 1)"""
    return _lib.sc_potential(kind=_lib.SC_POT_HARMONIC_SEP, dim=dim)


def _constant_hessian_parts(potential):
    """(const, lin, H) of V = const + lin.x + 1/2 x^T H x for a potential whose Hessian is constant (``MolecularHarmonicPotential``,
    ``MorsePotential`` with all chi = 0), None for every other"""
    from . import potentials as P
    if isinstance(potential, P.MolecularHarmonicPotential):
        H, x0, g = (hostmath.as_f64(t) for t in (potential.hess0, potential.pos0, potential.grad0))
        H = 0.5 * (H + H.T)
        const = float(potential.energy0) - potential._origin - float(g @ x0) + 0.5 * float(x0 @ H @ x0)
        return const, g - H @ x0, H
    if isinstance(potential, P.MorsePotential) and potential._is_harmonic():
        return 0.0, torch.zeros(potential.dimensions(), dtype=F64), torch.diag(hostmath.as_f64(potential.omega) ** 2)
    return None


def _morse_parts(potential):
    """(depth, rate, H) of V = sum_k depth_k (1 - exp(-rate_k x_k))^2 + 1/2 x^T H[0] x on the separable anharmonic surfaces
    (``MorsePotential`` with its own D and a, H None; ``NonHarmonicPotential``: the eps Morse part, (1 - eps) x^2 / 2 as H), None for
    every other"""
    from . import potentials as P
    if isinstance(potential, P.MorsePotential):
        return hostmath.as_f64(potential.D), hostmath.as_f64(potential.a), None
    if isinstance(potential, P.NonHarmonicPotential):
        eps, rate = hostmath.as_f64(potential.eps), hostmath.as_f64(potential.b)
        return 0.5 * eps / rate ** 2, rate, torch.diag(1.0 - eps).unsqueeze(0)
    return None


def _hamiltonian_operator(potential, who):
    """the one operator p^T m^-1 p / 2 + V(x) as the keyword arguments c, x, xx, pp, ex of ``expectation`` /
    ``wm_operator_expectation``, from ``_constant_hessian_parts`` or ``_morse_parts``; NotImplementedError for every other potential"""
    W = lambda: torch.diag(1.0 / hostmath.as_f64(potential.masses())).unsqueeze(0)
    quad = _constant_hessian_parts(potential)
    if quad is not None:
        const, lin, H = quad
        return dict(c=torch.tensor([const], dtype=F64), x=lin.unsqueeze(0), xx=H.unsqueeze(0), pp=W())
    morse = _morse_parts(potential)
    if morse is None:
        raise NotImplementedError(f"{who}: {type(potential).__name__} is neither a Morse-type potential (MorsePotential, "
                                  "NonHarmonicPotential) nor one with a constant Hessian: <V> has no closed form")
    depth, rate, H = morse
    # D_k (1 - exp(-a_k x_k))^2 = D_k - 2 D_k exp(-a_k x_k) + D_k exp(-2 a_k x_k)
    w = torch.cat((-2.0 * depth, depth)).unsqueeze(0)
    a = torch.cat((torch.diag(rate), torch.diag(2.0 * rate))).unsqueeze(0)
    return dict(c=depth.sum().reshape(1), xx=H, pp=W(), ex=(w, a))


def wm_pair_expect(bra, ket, U, za, zb, g, sfix, sket, lam, kap, stream=None):
    """sum_ij T_ij F_a,ij of M operators and sum_ij T_ij through ``sc_wm_pair_expect`` (include/semiclassical_hip.h), in as many calls
    as the columns need: one call holds ``sc_wm_pair_expect_capacity(D, d')`` columns (``hostmath.wm_expectation_launches``), the
    pieces of an operator are added on the host in the order of the calls.  ``bra`` = (qp, coef, cqqp, dvecp), ``ket`` = (qp, coef,
    cqq, dvec, cqqp, dvecp), U (D, d'), za (C, ni), zb (C, nj), g, sfix (C, d') complex, sket (M, nj, d') complex or None, lam
    (M, 1 + R) real, kap (M,) complex: contiguous tensors on one device.  Returns the complex ndarray (M + 1,), entry M = sum T."""
    dev = U.device
    D, dp = U.shape
    ni, nj = int(bra[0].shape[0]), int(ket[0].shape[0])
    M, C1 = lam.shape
    cap = int(lib.sc_wm_pair_expect_capacity(D, dp))
    tiles = max(int(lib.sc_wm_pair_expect_tiles(ni, nj)), 1)
    rows = [ptr(t) for t in bra] + [ni] + [ptr(t) for t in ket] + [nj, ptr(U), D, dp]

    def call(za, zb, g, sfix, sket, lam, kap, m, r):
        partials = torch.empty((tiles, m + 1, 2), dtype=F64, device=dev)
        out = torch.empty(m + 1, dtype=C128, device=dev)
        check(lib.sc_wm_pair_expect(*rows, ptr(za), ptr(zb), ptr(g), ptr(sfix), ptr(sket), ptr(lam), ptr(kap), m, r, ptr(partials),
                                    ptr(out), stream))
        return out.cpu().numpy()

    if M * C1 <= cap or cap < 2:            # (a shape outside the limits has capacity 0: the library names the limits)
        return call(za, zb, g, sfix, sket, lam.contiguous(), kap, M, C1 - 1)
    Rl, calls = hostmath.wm_expectation_launches(lam.cpu(), cap)
    # one more column and one more operator of zeros, for the padding and for column 0 of an operator's later pieces
    pad = lambda t: torch.cat((t, torch.zeros((1,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev)))
    za, zb, g, sfix, lam_f = pad(za), pad(zb), pad(g), pad(sfix), pad(lam.reshape(-1))
    kap_p = pad(kap)
    sket = pad(sket) if sket is not None else None
    res = np.zeros(M + 1, dtype=np.complex128)
    for k, pieces in enumerate(calls):
        cols, ops = [], []
        for a, first, sq in pieces:
            cols += [a * C1 if first else M * C1] + [a * C1 + r for r in sq] + [M * C1] * (Rl - len(sq))
            ops.append(a if first else M)
        ci, oi = torch.tensor(cols, device=dev), torch.tensor(ops, device=dev)
        out = call(za[ci].contiguous(), zb[ci].contiguous(), g[ci].contiguous(), sfix[ci].contiguous(),
                   sket[oi].contiguous() if sket is not None else None, lam_f[ci].contiguous(), kap_p[oi].contiguous(), len(pieces), Rl)
        for e, (a, _, _) in enumerate(pieces):
            res[a] += out[e]
        if k == 0:
            res[M] = out[len(pieces)]
    return res


def wm_pair_expect_cols(bra, ket, U, za, zb, g, sfix, sket, ketcol, kind, lam, kap, stream=None):
    """``wm_pair_expect`` through ``sc_wm_pair_expect_cols``: columns of the kinds 0, 1, 2 with per-ket border vectors on any of them
    (DESIGN.md section 4.25), cut into calls by ``hostmath.wm_operator_launches``; a call takes along the slots of sket its columns
    name.  Operands as ``wm_pair_expect``, and sket (S, nj, d') complex or None, ketcol, kind (C,) int32 on the device, lam (M, cols)
    real.  Returns the complex ndarray (M + 1,), entry M = sum T."""
    dev = U.device
    D, dp = U.shape
    ni, nj = int(bra[0].shape[0]), int(ket[0].shape[0])
    M, C1 = lam.shape
    cap = int(lib.sc_wm_pair_expect_capacity(D, dp))
    tiles = max(int(lib.sc_wm_pair_expect_tiles(ni, nj)), 1)
    rows = [ptr(t) for t in bra] + [ni] + [ptr(t) for t in ket] + [nj, ptr(U), D, dp]

    def call(za, zb, g, sfix, sket, ketcol, kind, lam, kap, m, cols):
        partials = torch.empty((tiles, m + 1, 2), dtype=F64, device=dev)
        out = torch.empty(m + 1, dtype=C128, device=dev)
        S = 0 if sket is None else int(sket.shape[0])
        check(lib.sc_wm_pair_expect_cols(*rows, ptr(za), ptr(zb), ptr(g), ptr(sfix), ptr(sket), S, ptr(ketcol), ptr(kind), ptr(lam),
                                         ptr(kap), m, cols, ptr(partials), ptr(out), stream))
        return out.cpu().numpy()

    if M * C1 <= cap or cap < 2:            # (a shape outside the limits has capacity 0: the library names the limits)
        return call(za, zb, g, sfix, sket, ketcol, kind, lam.contiguous(), kap, M, C1)
    cols, calls = hostmath.wm_operator_launches(lam.cpu(), kind.cpu().reshape(M, C1), cap)
    # one more column and one more operator of zeros, for the padding and for column 0 of an operator's later pieces
    pad = lambda t, fill=0: torch.cat((t, torch.full((1,) + tuple(t.shape[1:]), fill, dtype=t.dtype, device=dev)))
    za, zb, g, sfix, lam_f, kind, ketcol = pad(za), pad(zb), pad(g), pad(sfix), pad(lam.reshape(-1)), pad(kind), pad(ketcol, -1)
    kap_p = pad(kap)
    res = np.zeros(M + 1, dtype=np.complex128)
    for k, (ops, owners, columns) in enumerate(calls):
        ci, oi = torch.tensor(columns, device=dev), torch.tensor(ops, device=dev)
        kc = ketcol[ci].clone()
        used = kc >= 0
        slots = kc[used].long()                             # every slot belongs to one column: no duplicates
        kc[used] = torch.arange(int(slots.numel()), dtype=torch.int32, device=dev)
        out = call(za[ci].contiguous(), zb[ci].contiguous(), g[ci].contiguous(), sfix[ci].contiguous(),
                   sket[slots].contiguous() if slots.numel() else None, kc, kind[ci].contiguous(), lam_f[ci].contiguous(),
                   kap_p[oi].contiguous(), len(ops), cols)
        for e, a in enumerate(owners):
            res[a] += out[e]
        if k == 0:
            res[M] = out[len(ops)]
    return res


class WaltonManolopoulosPropagator(HermanKlukPropagator):
    """Walton-Manolopoulos (Filinov-smoothed) propagator, reference propagators.py:1077-1719.

    ``alpha``, ``beta``: widths of the phase-space cell over which the HK integrand is integrated out.
    The Filinov matrix, its inverse / determinant, the second inverse / determinant and the terms of
    eqns (85) and (100) are evaluated per trajectory by ``sc_wm_correlate`` right after the HK step kernel
    (registers for small matrices, LDS for medium ones, an L2-resident scratch block beyond that: no size limit).
    """

    _tiled_fast_path = False        # the Filinov matrix is built from the row-major blocks after every step
    _whole_loop_ok = False          # ... by its own kernel, between the steps
    _multi_ok = False
    _cross_ok = False               # cross_correlation() and run(targets=...) raise NotImplementedError
    _opcorr_ok = False              # operator_correlation() and run(operators=...) raise NotImplementedError
    _thermal_ok = False             # (set_)thermal_initial_conditions raise NotImplementedError

    def __init__(self, Gamma_i, Gamma_t, alpha, beta, device='cuda'):
        super().__init__(Gamma_i, Gamma_t, device=device)      # the Filinov matrix needs the dense monodromy blocks
        self.alpha = torch.tensor(float(alpha))
        self.beta = torch.tensor(float(beta))

    def _prepare(self):
        super()._prepare()
        dev, n = self.device, self.ntraj
        wm = hostmath.WMConstants(self._G0h, self._Gi, self._Gt, self._iGi0h, self.U.cpu(),
                                  float(self.alpha), float(self.beta))
        self._wm_host = wm
        up = lambda x: x.contiguous().to(dev)
        self._wm_bufs = {k: up(getattr(wm, k)) for k in ("U", "Gt", "G0", "iGi0", "S", "Cqq", "Cst", "Bq")}
        self._detA = torch.ones(n, dtype=C128, device=dev)
        self._detM = torch.ones(n, dtype=C128, device=dev)
        self._sgnA = torch.ones(n, dtype=F64, device=dev)
        self._sgnM = torch.ones(n, dtype=F64, device=dev)
        self._wm_flags = torch.zeros(n + 1, dtype=torch.int32, device=dev)      # fixed-order pivots handed to the pivoted kernel
        self._gwm = lib.sc_wm_grid(n, self.dim)
        self._wpart = torch.zeros((self._gwm, 4), dtype=F64, device=dev)
        self._wm_step, self._wm_has_nac = -1, False
        self._wm_export_step = -1
        self._wm_nac_bufs, self._wm_nac_traj = None, None
        need = lib.sc_wm_scratch_bytes(n, self.dim, wm.dprime)      # 0 while the matrices of a trajectory fit on chip
        assert need >= 0
        self._wm_scratch = torch.empty(need // 8, dtype=F64, device=dev) if need > 0 else None
        self._build_wm_struct()

    def _build_wm_struct(self):
        b, wm, nb = self._wm_bufs, self._wm_host, self._wm_nac_bufs
        self._wm = sc_wm_consts(
            dim=self.dim, dprime=wm.dprime, U=ptr(b["U"]), Gt=ptr(b["Gt"]), G0=ptr(b["G0"]), iGi0=ptr(b["iGi0"]),
            S=ptr(b["S"]), Cqq=ptr(b["Cqq"]), Cst=ptr(b["Cst"]), Bq=ptr(b["Bq"]), q0=ptr(self.q0), p0=ptr(self.p0),
            n1=ptr(nb[0]) if nb else None, s_n1=ptr(nb[1]) if nb else None, w_n1=ptr(nb[2]) if nb else None,
            inv_scale_a=wm.inv_scale_a, inv_two_pi=wm.inv_two_pi, pre=wm.pre,
            p0n1=self._wm_p0n1 if nb else 0.0, n2=self._wm_n2 if nb else 0.0,
            detA=ptr(self._detA), detM=ptr(self._detM), sgnA=ptr(self._sgnA), sgnM=ptr(self._sgnM),
            pre_coef=wm.pre_coef, scratch=ptr(self._wm_scratch),
            scratch_bytes=0 if self._wm_scratch is None else self._wm_scratch.numel() * 8, flags=ptr(self._wm_flags),
            nac_traj=ptr(getattr(self, "_wm_nac_traj", None)))

    def _remember_nac(self, potential):
        current, fp = self._nac_is_current(potential)
        if current:
            return
        super()._remember_nac(potential)
        masses, tau1, tau2, varies = fp
        wm = self._wm_host
        dev = self.device
        if bool(varies.item()):
            # position-dependent couplings: per trajectory n1(q_i), S n1(q_i), G0 n1(Q), p0.n1(Q), n2(q_i), n2(Q)
            # (sc_wm_consts.nac_traj); the q_i part is filled once, the Q part before every launch (_refresh_nac_traj)
            d, n = self.dim, self.ntraj
            self._wm_S, self._wm_G0 = wm.S.to(dev), wm.G0.to(dev)
            blk = torch.zeros((n, 3 * d + 3), dtype=F64, device=dev)
            n1q, n2q = self._coupling_vectors(potential, self.zi[:d])
            blk[:, :d] = n1q.t()
            blk[:, d:2 * d] = (self._wm_S @ n1q).t()
            blk[:, 3 * d + 1] = n2q
            self._wm_nac_traj = blk
            self._wm_nac_bufs = None
            self._build_wm_struct()
            return
        self._wm_nac_traj = None
        n1 = -hbar ** 2 * tau1 / masses
        self._wm_nac_bufs = [n1.to(dev), (wm.S @ n1).to(dev), (wm.G0 @ n1).to(dev)]
        self._wm_p0n1 = float(torch.dot(self._p0h, n1))
        self._wm_n2 = float(-hbar ** 2 * 0.5 * torch.sum(tau2 / masses))
        self._build_wm_struct()

    def _refresh_nac_traj(self):
        """the current-point half of sc_wm_consts.nac_traj: G0 n1(Q), p0.n1(Q), n2(Q) (reference propagators.py:1689-1697)"""
        d = self.dim
        n1Q, n2Q = self._coupling_vectors(self._nac_pot, self._qp.t()[:d])
        blk = self._wm_nac_traj
        blk[:, 2 * d:3 * d] = (self._wm_G0 @ n1Q).t()
        blk[:, 3 * d] = self.p0 @ n1Q
        blk[:, 3 * d + 2] = n2Q

    def _wm_launch(self, track):
        traj = getattr(self, "_wm_nac_traj", None)
        has_nac = self._wm_nac_bufs is not None or traj is not None
        if traj is not None:
            self._refresh_nac_traj()
        with self._timed("wm"):
            check(lib.sc_wm_correlate(self._state, self._wm, ptr(self._zi_t), ptr(self.probi), self._mc_norm(),
                                      track, int(has_nac), ptr(self._cq), ptr(self._kq), ptr(self._wpart),
                                      self._stream()))
        self._wm_step, self._wm_has_nac = self._nsteps, has_nac

    def _after_prefactor(self, track):
        self._leave_modal()                 # sc_wm_correlate reads Cartesian blocks; the next modal step converts forward again
        self._wm_launch(track)

    def _export(self):
        """per-trajectory v_n, C_QQ and d-vector of the current step (no tracking), reference :1391-1432, 1513"""
        if getattr(self, "_wm_export_step", -1) == self._nsteps:
            return self._wm_export
        dev, n, d = self.device, self.ntraj, self.dim
        coef = torch.zeros(n, dtype=C128, device=dev)
        cqq = torch.zeros((n, d, d), dtype=C128, device=dev)
        dvec = torch.zeros((n, d), dtype=C128, device=dev)
        self._wm.coef_out, self._wm.cqq_out, self._wm.dvec_out = ptr(coef), ptr(cqq), ptr(dvec)
        try:
            self._wm_launch(0)
        finally:
            self._wm.coef_out, self._wm.cqq_out, self._wm.dvec_out = None, None, None
        self._wm_export, self._wm_export_step = (coef, cqq, dvec), self._nsteps
        return self._wm_export

    def coefficients(self):
        """coefficients v_n of the Gaussians in the WM wavefunction, eqn (75) (reference propagators.py:1391-1432); the discard
        mask is ignored, as in HermanKlukPropagator.coefficients"""
        return self._export()[0]

    def wavefunction(self, x):
        """WM wavefunction psi(x,t) on a spatial grid x (dim,nx) -> complex ndarray (nx,) (reference :1434-1482); the discard
        mask is ignored"""
        x = torch.as_tensor(x, dtype=F64)
        d, nx = x.shape
        assert d == self.dim, "spatial grid has wrong dimensions"
        coef, cqq, dvec = self._export()
        X = x.T.contiguous().to(self.device)
        phi = torch.zeros(nx, dtype=C128, device=self.device)
        check(lib.sc_wm_grid_sum(ptr(self._qp), ptr(coef), ptr(cqq), ptr(dvec), self.ntraj, d, ptr(X), nx, ptr(phi),
                                 self._stream()))
        return phi.cpu().numpy()

    def norm(self, across_ranks=False, group=None):
        """norm |psi| of the WM wavefunction, O(n^2) with a d' x d' inverse per pair (reference :1484-1575); rank-local by
        default, across ranks (opt-in) as HermanKlukPropagator.norm: every rank sums its bras against the all-gathered
        kets, one all-reduce.  The discard mask is ignored."""
        from . import distributed as Dm
        group = self._norm_group(across_ranks, group)
        dev, n, d = self.device, self.ntraj, self.dim
        coef, cqq, dvec, cqqp, dvecp, U = self._wm_pair_operands()
        dp = U.shape[1]
        flat = lambda t: torch.view_as_real(t.contiguous()).reshape(t.shape[0], -1)
        ket = torch.cat((self._qp, flat(coef.unsqueeze(1)), flat(cqq), flat(dvec), flat(cqqp), flat(dvecp)), 1)
        ket = Dm.all_gather_rows(ket, group)
        nj = ket.shape[0]
        widths = [2 * d, 2, 2 * d * d, 2 * d, 2 * dp * dp, 2 * dp]
        qpj, coefj, cqqj, dvecj, cqqpj, dvecpj = (c.contiguous() for c in torch.split(ket, widths, dim=1))
        tiles = lib.sc_wm_pair_sum_rect_tiles(n, nj)
        partials = torch.empty((tiles, 4), dtype=F64, device=dev)
        slot = torch.zeros(8, dtype=F64, device=dev)
        s = self._stream()
        check(lib.sc_wm_pair_sum_rect(ptr(self._qp), ptr(coef), ptr(cqqp), ptr(dvecp), n, ptr(qpj), ptr(coefj), ptr(cqqj),
                                      ptr(dvecj), ptr(cqqpj), ptr(dvecpj), nj, ptr(U), d, dp, ptr(partials), s))
        check(lib.sc_reduce_slot(ptr(partials), int(tiles), None, 0, 1.0, ptr(slot), s))
        Dm.all_reduce_sum(slot, group)
        return float(torch.sqrt(slot[0]).item())

    def _wm_pair_operands(self):
        """(coef, cqq, dvec, cqqp, dvecp, U): the export of the current step and its projections U^T CQQ U, U^T dvec per trajectory,
        the operands of the pair sums; U (D, d') real"""
        coef, cqq, dvec = self._export()
        U = self._wm_bufs["U"]
        Uc = U.type(C128)
        cqqp = torch.einsum('ak,nab,bl->nkl', Uc, cqq, Uc).contiguous()
        dvecp = (dvec @ Uc).contiguous()
        return coef, cqq, dvec, cqqp, dvecp, U

    def reduced_density(self, directions, s):
        raise NotImplementedError("reduced_density is not available for the Walton-Manolopoulos propagator: its Gaussians carry "
                                  "per-trajectory widths, the closed form behind it needs one width Gamma_t for all of them")

    def expectation(self, c=None, x=None, xx=None, p=None, pp=None, normalise=True, ex=None):
        raise NotImplementedError("expectation is not available for the Walton-Manolopoulos propagator: its Gaussians carry "
                                  "per-trajectory widths, the closed form behind it needs one width Gamma_t for all of them "
                                  "(wm_expectation, wm_operator_expectation and their moments solve a d' x d' system per pair instead)")

    def wm_expectation(self, c=None, x=None, xx=None, p=None, normalise=True):
        """Expectation values of M operators in the WM wavepacket (not in the reference):

            A_a = c_a + x_a.x + 1/2 x^T xx_a x + p_a.p          (p = -i hbar d/dx; no quadratic momentum part),
            E_a = <psi|A_a|psi> = sum_ij conj(v_i) O_ij v_j F_a,ij,      N2 = sum_ij conj(v_i) O_ij v_j = norm()**2,

        O_ij the overlaps and v the coefficients of ``norm()``, F_a,ij the matrix element of A_a between the Gaussians of the
        trajectories i and j divided by their overlap: with D' and b' of the pair, the mean of x is Q_i + U D'^-1 b' and its
        covariance U D'^-1 U^T (``hostmath.fold_wm_expectation_operators``).  ``c`` (M,), ``x``, ``p`` (M, D), ``xx`` (M, D, D) real
        symmetric; any of them may be None (= zeros), M is taken from the ones given.  Returns ``(values, norm2)``: the complex
        ndarray (M,) of E_a / N2 -- of E_a with ``normalise=False`` -- and the float N2.  The imaginary part of the value of a
        Hermitian operator is rounding.

        Every x_a, p_a and eigenvector of xx_a (eigenvalues above 1e-12 of the largest) has to lie in the span of the non-zero
        width modes: ``ValueError`` naming the operator otherwise, as for parts whose shapes do not agree, a non-symmetric xx and
        non-finite entries.

        The pair sum runs in ``sc_wm_pair_expect`` on the operands ``norm()`` packs, in as many calls as the operators' columns
        need (``wm_pair_expect``).  Rank-local: this rank's trajectories with this rank's weights, no communication.  The discard
        mask (discard_nonsymplectic) is ignored: discarded trajectories contribute as ever.  No step is taken and the state is
        not touched.  The value is quadratic in the ensemble, not additive over batches: there is no hook in ``run()``."""
        d = self.dim
        vx, nvec, lam, kap, R = hostmath.fold_wm_expectation_operators(c, x, xx, p, self._wm_host.U)
        coef, cqq, dvec, cqqp, dvecp, U = self._wm_pair_operands()
        Q = self._qp[:, :d]
        za, zb, g, sfix, sket = hostmath.wm_expectation_columns(vx, nvec, Q, dvecp, Q, cqq, dvec, dvecp, U)
        with self._timed("wm_expectation"):
            res = wm_pair_expect((self._qp, coef, cqqp, dvecp), (self._qp, coef, cqq, dvec, cqqp, dvecp), U, za, zb, g, sfix, sket,
                                 lam.to(self.device), kap.to(self.device), self._stream())
        M = int(kap.shape[0])
        norm2 = float(res[M].real)
        return (res[:M] / norm2 if normalise else res[:M].copy()), norm2

    def wm_wavepacket_moments(self, directions=None):
        """Centre and width of the WM wavepacket along chosen directions u: a dict with ``x`` = <u.x>, ``p`` = <u.p>, ``var_x`` =
        <(u.x)^2> - <u.x>^2, real ndarrays (M,) of the values normalised with ``norm2`` = norm()**2, which comes along (no ``var_p``:
        ``wm_expectation`` has no quadratic momentum part).  ``directions`` as in ``HermanKlukPropagator.reduced_density``: mode
        indices or vectors of length D; None means the D axes, for widths of full rank only (``ValueError`` otherwise: give
        directions in the span of the non-zero width modes).  One ``wm_expectation`` call with three operators per direction;
        what is said there about ranks, the discard mask and the state holds here."""
        d = self.dim
        if directions is None:
            if self._wm_host.dprime != d:
                raise ValueError("wm_wavepacket_moments: the widths are singular, the moments along their null directions do not "
                                 "exist: give directions in the span of the non-zero width modes")
            U = torch.eye(d, dtype=F64)
        else:
            U = self._density_directions(directions)
            if bool((torch.linalg.norm(U, dim=1) == 0).any()):
                raise ValueError("directions: zero vector")
        Md = U.shape[0]
        zv, zm = torch.zeros((Md, d), dtype=F64), torch.zeros((Md, d, d), dtype=F64)
        uu = 2.0 * U.unsqueeze(2) * U.unsqueeze(1)          # 1/2 x^T (2 u u^T) x = (u.x)^2
        vals, norm2 = self.wm_expectation(x=torch.cat((U, zv, zv)), xx=torch.cat((zm, uu, zm)), p=torch.cat((zv, zv, U)))
        ex, exx, ep = (vals[k * Md:(k + 1) * Md].real for k in range(3))
        return {"x": ex, "p": ep, "var_x": exx - ex ** 2, "norm2": norm2}

    def wm_operator_expectation(self, c=None, x=None, xx=None, p=None, pp=None, ex=None, normalise=True):
        """``wm_expectation`` with a quadratic momentum part and exponentials (not in the reference):

            A_a = c_a + x_a.x + 1/2 x^T xx_a x + p_a.p + 1/2 p^T pp_a p + sum_e w_a,e exp(-a_a,e . x)        (no x-p cross terms),

        shapes and conventions of ``wm_expectation`` and of ``HermanKlukPropagator.expectation``: ``pp`` (M, D, D) real symmetric,
        ``ex = (w, a)`` with w (M, P) and a (M, P, D) real, an operator with fewer terms has w = 0 in the others.  Returns
        ``(values, norm2)`` as there.  1/2 p^T pp p acts on the ket alone: with L_j(x) = d_j - C_j (x - Q_j) its element is
        -hbar^2 / 2 [L_j^T pp L_j - tr(pp C_j)] under the pair's Gaussian, one squared column with a per-ket border vector per
        eigenpair of pp; an exponential is exp(-a.xbar + 1/2 a^T B a), one column (``hostmath.fold_wm_operator_columns``).  A single
        pair's momentum term is not Hermitian-symmetric, the sum over the pairs is.

        Every x_a, p_a, a_e with w_e != 0 and eigenvector of xx_a, pp_a has to lie in the span of the non-zero width modes
        (``ValueError`` naming the operator and the part).  A value that is not finite -- an exponential out of range: a trajectory
        far out on the repulsive wall -- is a ``ValueError`` naming the operator; nothing is rescaled.  Sums of exponentials of
        alternating sign (a Morse V) round relative to the sum of the absolute terms, as in section 4.23.

        Without ``pp`` and ``ex`` this is ``wm_expectation``, bit for bit.  Otherwise the pair sum runs in
        ``sc_wm_pair_expect_cols`` (``wm_pair_expect_cols``).  Rank-local, the discard mask ignored, no step taken and no state
        touched, no hook in ``run()``: what ``wm_expectation`` says."""
        if pp is None and ex is None:
            return self.wm_expectation(c, x, xx, p, normalise)
        d = self.dim
        vx, vp, kind, lam, kap, _ = hostmath.fold_wm_operator_columns(c, x, xx, p, pp, ex, self._wm_host.U)
        coef, cqq, dvec, cqqp, dvecp, U = self._wm_pair_operands()
        Q = self._qp[:, :d]
        za, zb, g, sfix, sket, ketcol, kind_d = hostmath.wm_operator_columns(vx, vp, kind, lam, Q, dvecp, Q, cqq, dvec, dvecp, U)
        with self._timed("wm_operator_expectation"):
            res = wm_pair_expect_cols((self._qp, coef, cqqp, dvecp), (self._qp, coef, cqq, dvec, cqqp, dvecp), U, za, zb, g, sfix,
                                      sket, ketcol, kind_d, lam.to(self.device), kap.to(self.device), self._stream())
        M = int(kap.shape[0])
        bad = ~np.isfinite(res[:M])
        if bad.any():
            raise ValueError(f"operators: the value of operator {int(np.nonzero(bad)[0][0])} is not finite: an exponential is out of "
                             "range at a pair of trajectories (one has run far out on the repulsive wall)")
        norm2 = float(res[M].real)
        return (res[:M] / norm2 if normalise else res[:M].copy()), norm2

    def wm_phase_space_moments(self, directions=None):
        """``wm_wavepacket_moments`` with the momentum variance: a dict with ``x``, ``p``, ``var_x``, ``var_p`` = <(u.p)^2> - <u.p>^2
        and ``norm2``.  ``directions`` and the refusals as there.  One ``wm_operator_expectation`` call with four operators per
        direction."""
        d = self.dim
        if directions is None:
            if self._wm_host.dprime != d:
                raise ValueError("wm_phase_space_moments: the widths are singular, the moments along their null directions do not "
                                 "exist: give directions in the span of the non-zero width modes")
            U = torch.eye(d, dtype=F64)
        else:
            U = self._density_directions(directions)
            if bool((torch.linalg.norm(U, dim=1) == 0).any()):
                raise ValueError("directions: zero vector")
        Md = U.shape[0]
        zv, zm = torch.zeros((Md, d), dtype=F64), torch.zeros((Md, d, d), dtype=F64)
        uu = 2.0 * U.unsqueeze(2) * U.unsqueeze(1)          # 1/2 x^T (2 u u^T) x = (u.x)^2
        vals, norm2 = self.wm_operator_expectation(x=torch.cat((U, zv, zv, zv)), xx=torch.cat((zm, uu, zm, zm)),
                                                   p=torch.cat((zv, zv, U, zv)), pp=torch.cat((zm, zm, zm, uu)))
        ex, exx, ep, epp = (vals[k * Md:(k + 1) * Md].real for k in range(4))
        return {"x": ex, "p": ep, "var_x": exx - ex ** 2, "var_p": epp - ep ** 2, "norm2": norm2}

    def wm_energy_expectation(self, potential):
        """<psi| p^T m^-1 p / 2 + V(x) |psi> / norm()**2 of the WM wavepacket: a float, the real part of one
        ``wm_operator_expectation`` value.  V as ``HermanKlukPropagator.energy_expectation`` and ``anharmonic_energy_expectation``
        build it (``_hamiltonian_operator``): ``MolecularHarmonicPotential``; ``MorsePotential`` with its own D and a -- D squared
        momentum columns and 2 D exponentials in one operator, or omega^2 as ``xx`` when every chi = 0 --; ``NonHarmonicPotential``.
        sGDML and quartic force fields: ``NotImplementedError``.  Singular widths (d' < D) are refused with ``ValueError``: the
        kinetic energy along their null directions does not exist.  On the Morse-type surfaces V is a sum of terms of alternating
        sign that are each about D_k: rounding is relative to the sum of the absolute terms, as in section 4.23 (there is no
        cancellation-free fold)."""
        parts = _hamiltonian_operator(potential, "wm_energy_expectation")
        if potential.dimensions() != self.dim:
            raise ValueError(f"wm_energy_expectation: the potential has {potential.dimensions()} dimensions, the propagator {self.dim}")
        if self._wm_host.dprime != self.dim:
            raise ValueError("wm_energy_expectation: the widths are singular, the kinetic energy along their null directions does "
                             "not exist; projecting it is the caller's decision (wm_operator_expectation() with a projected pp)")
        vals, _ = self.wm_operator_expectation(**parts)
        return float(vals[0].real)

    def _launch_correlate(self, row, state=None, cursor=None, per_trajectory=True, families=()):
        # no pairs or visits; run(targets=...) and run(operators=...) are refused before the loop starts
        assert state is None and not families
        # the per-trajectory terms were produced together with the prefactor; recompute (with the stored branch
        # signs, no tracking) only if the coupling vector was not known at that time
        knows_nac = self._wm_nac_bufs is not None or self._wm_nac_traj is not None
        if self._wm_step != self._nsteps or (knows_nac and not self._wm_has_nac):
            self._wm_launch(0)
        if self._kept is not None:
            # discard mask: every sum from the exported terms, over the kept trajectories (sc_term_masked_sums)
            assert cursor is None
            self._masked_sums(self._wm_has_nac, row)
            return
        # sc_wm_correlate exports every trajectory's terms exactly once (register kernel or its pivoted re-run): their moments,
        # in a pass of its own (not fused into the WM kernels)
        mom_rows = self._term_moments(self._wm_has_nac) if row.moments is not None else None
        if row.blocks is not None:
            self._term_blocks(self._wm_has_nac, row.blocks, cursor)         # the same exported terms; before the cursor advances
        self._reduce_into(self._wpart, self._gwm, row, cursor, mom_rows)

    def _correlate_current(self, need_nac):
        if self._corr_step == self._nsteps and (self._corr_has_nac or not need_nac):
            return
        self._launch_correlate(self._rows.single(self._slot))
        self._corr_step, self._corr_has_nac = self._nsteps, self._wm_has_nac
        self._slot_host = self._slot.cpu().numpy().copy()
        self._check_energy_guard()

    _TRACKED = {"prefactorC": ("_sgn", "_c2"), "detA": ("_sgnA", "_detA"), "detM": ("_sgnM", "_detM")}

    def _get_signs_of_sqrt(self, key):
        if key == "detA":
            return self._sgnA.type(C128)
        if key == "detM":
            return self._sgnM.type(C128)
        return super()._get_signs_of_sqrt(key)
