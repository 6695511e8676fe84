"""`semi dynamics` / `semi rates` tasks on the HIP engine.

Drop-in for the JSON task lists of the reference (README.rst:90-102; semiclassical/cli.py:171-476
``run_semiclassical_dynamics``, :519-570 ``calculate_rates``): the same task keys with the same defaults, the same
``correlations.npz`` keys, the same accumulate / overwrite semantics and the same error texts -- those are the
contract.  The code around the contract is organised differently from the reference:

    ProblemSetup       what a potential section resolves to (one builder per potential type, registered by name)
    CorrelationStore   the npz file as a running, trajectory-weighted mean over repetitions and over separate runs
    propagate_batch    one repetition on the device; the time loop is ``propagator.run`` (no host sync inside)

    python -m semiclassical_amd.driver dynamics input.json [--cuda ID]
    python -m semiclassical_amd.driver rates input.json

Not carried over: extxyz export and plotting (outside the hot path).
"""
import argparse
import json
import logging
import os
from collections import namedtuple

import numpy as np
import torch

from . import broadening, hostmath, potentials, propagators, rates, readers, units
from .units import hbar

logger = logging.getLogger(__name__)


class ConfigurationError(Exception):
    pass


# ---------------------------------------------------------------------------------------------------------------------
# the 'potential' section of a task
# ---------------------------------------------------------------------------------------------------------------------

ProblemSetup = namedtuple("ProblemSetup", "potential q0 p0 Gamma_0 zero_point_energy adiabatic_gap")

_SETUPS = {}


def _potential_type(name):
    def register(builder):
        _SETUPS[name] = builder
        return builder
    return register


def _fchk(path):
    with open(path) as handle:
        return readers.FormattedCheckpointFile(handle)


def _molecular_setup(surface, excited_state):
    """Final-state surface + initial wavepacket of a molecule: the wavepacket is the vibrational ground state of the
    excited-state fchk file; the surface is relaxed from there and its minimum becomes the energy origin, which fixes
    the adiabatic gap (cli.py:187-197, 293-300)."""
    centre, widths, zero_point = excited_state.vibrational_groundstate()
    q0 = torch.from_numpy(centre)
    surface.minimize(q0)
    gap = excited_state.total_energy() - surface.total_energy()
    logger.info(f"  adiabatic excitation energy               : {gap * units.hartree_to_ev:.4f} eV")
    return ProblemSetup(surface, q0, torch.zeros_like(q0), torch.from_numpy(widths), zero_point, gap)


@_potential_type("harmonic")
def _setup_harmonic(section):
    surface = potentials.MolecularHarmonicPotential(_fchk(section['ground']), _fchk(section['coupling']))
    return _molecular_setup(surface, _fchk(section['excited']))


@_potential_type("gdml")
def _setup_gdml(section):
    from .gdml import MolecularGDMLPotential
    model = np.load(section['ground'], allow_pickle=True)
    surface = MolecularGDMLPotential(model, _fchk(section['coupling']))
    return _molecular_setup(surface, _fchk(section['excited']))     # minimize() may raise, as the reference's does


@_potential_type("anharmonic AS")
def _setup_adiabatic_shift(section):
    """model file with one row per mode: frequency / cm^-1, Huang-Rhys factor (its sign is the direction of the
    displacement), coupling, anharmonicity (README.rst:367-373, cli.py:229-285)"""
    table = torch.from_numpy(np.atleast_2d(np.loadtxt(section['model_file'])))
    logger.info("vibrational modes (cm^-1):")
    logger.info(table[:, 0])
    omega = table[:, 0] / units.hartree_to_wavenumbers
    huang_rhys, coupling, chi = table[:, 1], table[:, 2], table[:, 3]
    shift = torch.sign(huang_rhys) * torch.sqrt(2.0 * abs(huang_rhys) / omega)       # S = 1/2 dQ^2 omega
    shift[omega == 0.0] = 0.0                                                        # zero modes are not displaced
    zero_point = torch.sum(hbar / 2.0 * omega).item()
    return ProblemSetup(potentials.MorsePotential(omega, chi, coupling), shift, 0.0 * shift, torch.diag(omega),
                        zero_point, np.nan)


@_potential_type("quartic force field")
def _setup_quartic_force_field(section):
    """npz model file.  Surface: pos0 (D,), energy0 (), grad0 (D,), hess0 (D, D), masses (D,), coupling (D,) and the optional
    cubic (D, D, D), quartic_iijj (D, D), quartic_iiij (D, D), origin (); all derivatives at pos0 in atomic units
    (potentials.QuarticForceFieldPotential).  Wavepacket: q0 (D,), Gamma_0 (D, D), zero_point_energy (), optional p0 (D,)
    (default 0) and adiabatic_gap (default NaN, as the AS type).  No minimisation: the file says where the origin is."""
    path = section['model_file']
    try:
        with np.load(path) as npz:
            data = {k: np.asarray(npz[k], dtype=np.float64) for k in npz.files}
    except Exception as err:
        raise ConfigurationError(f"'quartic force field': {path} should be an npz file ({err})")
    required = ("pos0", "energy0", "grad0", "hess0", "masses", "coupling", "q0", "Gamma_0", "zero_point_energy")
    missing = [k for k in required if k not in data]
    if missing:
        raise ConfigurationError(f"'quartic force field': {path} lacks the array(s) {', '.join(missing)}")
    dim = data["pos0"].size
    shapes = {"q0": (dim,), "p0": (dim,), "Gamma_0": (dim, dim), "zero_point_energy": (), "adiabatic_gap": (), "origin": ()}
    for key, shape in shapes.items():
        if key in data and (data[key].shape != shape or not np.all(np.isfinite(data[key])) and key != "adiabatic_gap"):
            raise ConfigurationError(f"'quartic force field': {key} of shape {shape}, finite, is expected in {path}, got "
                                     f"{data[key].shape}")
    try:
        surface = potentials.QuarticForceFieldPotential.from_arrays(
            data["pos0"], data["energy0"], data["grad0"], data["hess0"], cubic=data.get("cubic"),
            quartic_iijj=data.get("quartic_iijj"), quartic_iiij=data.get("quartic_iiij"), masses=data["masses"],
            nac0=data["coupling"], origin=float(data.get("origin", 0.0)))
    except ValueError as err:
        raise ConfigurationError(f"'quartic force field': {path}: {err}")
    q0 = torch.from_numpy(data["q0"])
    p0 = torch.from_numpy(data["p0"]) if "p0" in data else torch.zeros_like(q0)
    return ProblemSetup(surface, q0, p0, torch.from_numpy(data["Gamma_0"]), float(data["zero_point_energy"]),
                        float(data.get("adiabatic_gap", np.nan)))


def build_problem(task):
    section = task['potential']
    builder = _SETUPS.get(section['type'])
    if builder is None:
        raise ConfigurationError(f"Unknown potential type in {task['potential']}")
    return builder(section)


# ---------------------------------------------------------------------------------------------------------------------
# correlations.npz
# ---------------------------------------------------------------------------------------------------------------------

# The two families of five-sum rows as the driver carries them from the task to the result file.
#   task_key  the task's key, an npz file (_load_targets / _load_operators)
#   noun      the propagate_batch argument and the run() argument, and the noun of the messages; buffer: run()'s buffer argument
#   idents    the arrays that say which estimator it is: the keys of the record, stored as prefix + key; as_run: the same arrays as
#             run() takes them
#   stored    the key of the pooled correlation functions; + "_second_moment" and + "_error" by the keep-or-drop rule
#   what, rows  the nouns of the messages; ndim, expected: the shape check of the first array
#   stale     derived keys that go stale when the correlation functions change
#   optional  further identifying arrays that a task may leave out: absent means zeros (the Hessians K of the operators, DESIGN.md
#             section 4.16); carried behind idents, stored only when the task gave them
RowFamily = namedtuple("RowFamily", "task_key noun buffer idents prefix as_run stored what rows ndim expected stale optional",
                       defaults=((),))
ROW_FAMILIES = (
    RowFamily("cross_correlation_targets", "targets", "cross", ("q", "p"), "cross_targets_", tuple, "cross_correlation",
              "cross-correlation functions", "cross-correlation", 2, "arrays of shape (K, D) with K > 0 are", ()),
    RowFamily("operator_correlation", "operators", "opcorr", ("bra_c", "bra_m", "ket_c", "ket_m"), "operator_",
              lambda a: (tuple(a[:2]) + tuple(a[4:5]), tuple(a[2:4]) + tuple(a[5:6])), "operator_correlation",
              "operator correlation functions", "operator-correlation", 1, "c of shape (M,) with M > 0 is",
              ("operator_lineshape", "radiative_rate"), ("bra_k", "ket_k")),
)


class CorrelationStore(object):
    """The result file: ``propagator, times, autocorrelation, ic_correlation, adiabatic_gap, zero_point_energy,
    trajectories`` (cli.py:346-353), re-read and re-written after every batch so that an interrupted run keeps what it
    has (cli.py:453-476)."""

    def __init__(self, path):
        self.path = path

    def _check_temperature(self, stored, kelvin):
        """the stored correlation functions belong to the ensemble of this temperature (``temperature``, Kelvin; no key and None:
        the one pure state of a task without "temperature")"""
        have = float(stored['temperature']) if 'temperature' in stored else None
        if have != (None if kelvin is None else float(kelvin)):
            say = lambda T: "without a temperature" if T is None else f"at {T:g} K"
            raise ConfigurationError(
                f"{self.path} holds correlation functions computed {say(have)}, this task runs {say(kelvin)} "
                "(\"temperature\"): they are different ensembles and cannot be pooled")

    def start(self, task, propagator_name, times, setup, cross_targets=None, operators=None, time_average=None, temperature=None):
        """``cross_targets``: (q, p) of the task's "cross_correlation_targets", or None: a file that is added to has to hold
        exactly these (ConfigurationError otherwise, before any trajectory runs).  ``operators``: (bra_c, bra_m, ket_c, ket_m) of
        the task's "operator_correlation", or None: the same rule; (..., bra_k, ket_k) with Hessians (M, D, D), which a file
        without them holds as zeros.  ``time_average``: (energies, q, p, window) of the task's "time_averaged_spectrum", or None:
        the same rule for the stored ``ta_energies``, ``ta_references_q``, ``ta_references_p`` and ``ta_window``.  ``temperature``:
        the task's "temperature" in Kelvin, or None: the same rule for the stored ``temperature``."""
        fresh = task['results'].get('overwrite', True) is True or not os.path.exists(self.path)
        if fresh:
            nt = len(times)
            np.savez(self.path, propagator=propagator_name, times=times,
                     autocorrelation=np.zeros((nt,), dtype=complex), ic_correlation=np.zeros((nt,), dtype=complex),
                     adiabatic_gap=setup.adiabatic_gap, zero_point_energy=setup.zero_point_energy, trajectories=0)
            return
        # adding to the results of an earlier run
        assert task.get('manual_seed', None) is None, \
            "Multiple runs with the same sequence of random numbers make no sense! Do not use `manual_seed` and `overwrite=False` at the same time"
        previous = np.load(self.path)
        assert np.array_equal(previous['times'], times.numpy()), \
            f"Time steps in {self.path} differ. Delete the old file or change the grid for time propagation."
        assert previous['propagator'] == propagator_name, "Data produced with different propagators cannot be added."
        if previous['trajectories'] > 0:
            for fam, idents in zip(ROW_FAMILIES, (cross_targets, operators)):
                self._check_family(fam, previous, idents)
            self._check_time_average(previous, time_average)
            self._check_temperature(previous, temperature)

    CROSS_KEYS, OPERATOR_KEYS = (tuple(fam.prefix + key for key in fam.idents) + (fam.stored,) for fam in ROW_FAMILIES)

    CROSS_ERROR_KEYS, OPERATOR_ERROR_KEYS = ((fam.stored + '_second_moment', fam.stored + '_error') for fam in ROW_FAMILIES)

    def _check_family(self, fam, stored, idents):
        """the stored correlation functions of the family belong to exactly the identifying arrays of the task or batch (the targets
        (q, p), the operators (bra_c, bra_m, ket_c, ket_m); None: it has none)"""
        have = fam.prefix + fam.idents[0] in stored
        if have != (idents is not None):
            raise ConfigurationError(
                f"{self.path} holds {fam.what if have else 'no ' + fam.what}, this task "
                f"{'has no' if have else 'has'} \"{fam.task_key}\": they cannot be pooled")
        same = have and all(np.array_equal(stored[fam.prefix + key], new) for key, new in zip(fam.idents, idents))
        for at, key in enumerate(fam.optional, len(fam.idents)):         # absent on either side: zeros
            old, new = stored.get(fam.prefix + key), idents[at] if have and at < len(idents) else None
            if old is not None and new is not None:
                same = same and np.array_equal(old, new)
            else:
                same = same and not any(np.any(a) for a in (old, new) if a is not None)
        if have and not same:
            raise ConfigurationError(
                f"{self.path} holds {fam.what} with other {fam.noun} than this task's "
                f"(\"{fam.task_key}\"): they are different estimators and cannot be pooled")

    TA_IDENT_KEYS = ('ta_energies', 'ta_references_q', 'ta_references_p', 'ta_window')
    TA_ERROR_KEYS = ('ta_spectrum_second_moment', 'ta_spectrum_error')

    def _check_time_average(self, stored, idents):
        """the stored time-averaged spectrum belongs to exactly the energies, reference states and window (energies, q, p, T) of
        the task or batch (None: it has none)"""
        have = 'ta_energies' in stored
        if have != (idents is not None):
            raise ConfigurationError(
                f"{self.path} holds {'a' if have else 'no'} time-averaged spectrum, this task "
                f"{'has no' if have else 'has'} \"time_averaged_spectrum\": they cannot be pooled")
        if have and not all(np.array_equal(stored[key], np.asarray(new, dtype=np.float64)) for key, new in zip(self.TA_IDENT_KEYS, idents)):
            raise ConfigurationError(
                f"{self.path} holds a time-averaged spectrum with other energies, reference states or another window than this "
                "task's (\"time_averaged_spectrum\", \"num_steps\", \"time_step_fs\"): they are different estimators and cannot "
                "be pooled")

    ERROR_KEYS = ('autocorrelation_error', 'ic_correlation_error', 'autocorrelation_second_moment', 'ic_correlation_second_moment')

    BLOCK_KEYS = ('autocorrelation_blocks', 'ic_correlation_blocks', 'block_trajectories')

    SYMPLECTICITY_KEYS = ('symplecticity_steps', 'symplecticity_max', 'symplecticity_mean', 'symplecticity_exceeding',
                          'symplecticity_tolerance', 'symplecticity_kept', 'symplecticity_discard')

    def add_batch(self, autocorrelation, ic_correlation, ntraj, second_moments=None, blocks=None, symplecticity=None, cross=None,
                  operators=None, time_average=None, temperature=None):
        """fold the means over ``ntraj`` new trajectories into the stored means.  ``second_moments``: (M_C, M_k), the
        per-sample second moments (rows (S_rr, S_ii, S_ri) times the batch size, phase applied) of the batch, folded the same
        way; the standard errors of the pooled means follow from them.  Files and batches that do not both carry them lose
        the error keys (with a warning): errors over only part of the stored trajectories would be wrong.
        ``blocks``: (C_blocks, k_blocks, counts) -- the block sums (nt, B) of the batch (phase applied; their sum over the blocks is
        the batch mean) and the trajectories per block (B,).  The sums are folded with the same weights as the means, so that the
        stored blocks keep adding up to the stored means, and the counts add: block b of the file is block b of every batch,
        pooled.  The same rule as for the second moments drops the block keys.
        ``symplecticity``: the record of propagate_batch's symplecticity checks ('steps', 'max', 'mean' per check and, with a
        tolerance, 'exceeding' and 'tolerance').  Over batches the maxima pool as maxima, the means with the weights of the
        correlation functions, the counts add.  Files and batches that do not both carry the keys, or that differ in the steps
        checked or in the tolerance, lose them (same rule again).
        With 'discard' set in the record (the task discards the trajectories that fail the check) the
        record also carries 'kept', the trajectories still kept after every check; the file then holds ``symplecticity_kept``
        (counts add) and ``symplecticity_discard``.  Correlation functions with and without discarding, or discarded against
        another tolerance or at other steps, are different estimators: pooling them is refused (ConfigurationError), never
        resolved by dropping keys.
        ``cross``: the record of the batch's cross-correlation functions: 'q', 'p' (K, D) the targets,
        'correlation' (nt, K) and, with standard errors, 'second_moment' (nt, K, 3) as for the autocorrelation.  The file then holds
        ``cross_targets_q``, ``cross_targets_p``, ``cross_correlation`` (pooled with the weights of ``autocorrelation``) and, by the
        keep-or-drop rule of the second moments, ``cross_correlation_second_moment`` and ``cross_correlation_error``.  Stored
        targets that differ from the batch's (or exist on one side only) are refused (ConfigurationError).
        ``operators``: the record of the batch's operator correlation functions: 'bra_c', 'ket_c' (M,),
        'bra_m', 'ket_m' (M, D), optionally the Hessians 'bra_k', 'ket_k' (M, D, D) of quadratic operators (section 4.16; stored as
        ``operator_bra_k``, ``operator_ket_k`` only when given, absent = zeros), 'correlation' (nt, M) and, with standard errors,
        'second_moment' (nt, M, 3).  The file then holds
        ``operator_bra_c``, ``operator_bra_m``, ``operator_ket_c``, ``operator_ket_m``, ``operator_correlation`` and, by the same
        keep-or-drop rule, ``operator_correlation_second_moment`` and ``operator_correlation_error``; everything as for ``cross``.
        ``time_average``: the record of the batch's time-averaged spectrum: 'energies' (NE,), 'q', 'p'
        (K, D) the reference states, 'window' T, 'spectrum' (K, NE) and, with standard errors, 'second_moment' (K, NE), the
        per-sample second moment N sum_i y_i^2.  The file then holds ``ta_energies``, ``ta_references_q``, ``ta_references_p``,
        ``ta_window``, ``ta_spectrum`` (pooled with the weights of ``autocorrelation``) and, by the same keep-or-drop rule,
        ``ta_spectrum_second_moment`` and ``ta_spectrum_error``.  Other stored energies, reference states or window (or a
        spectrum on one side only) are refused (ConfigurationError).
        ``temperature``: the temperature in Kelvin of the batch's thermal ensemble, None for the one pure
        state; the file then holds ``temperature``.  A file of another temperature (or of none) is refused (ConfigurationError)."""
        stored = dict(np.load(self.path))
        done = stored['trajectories']
        total = done + ntraj
        if done > 0:
            self._check_temperature(stored, temperature)
        if temperature is not None:
            stored['temperature'] = float(temperature)
        records = list(zip(ROW_FAMILIES, (cross, operators)))
        if done > 0:
            for fam, record in records:
                self._check_family(fam, stored, None if record is None else
                                   tuple(record[key] for key in fam.idents + fam.optional if key in record))
            self._check_time_average(stored, None if time_average is None else
                                     tuple(time_average[key] for key in ('energies', 'q', 'p', 'window')))
        discarding = symplecticity is not None and bool(symplecticity.get('discard', False))
        if done > 0:
            was_discarding = bool(stored.get('symplecticity_discard', False))
            if was_discarding != discarding:
                raise ConfigurationError(
                    f"{self.path} holds correlation functions computed {'with' if was_discarding else 'without'} "
                    f"\"discard_nonsymplectic\", this batch was computed {'with' if discarding else 'without'} it: they are "
                    "different estimators and cannot be pooled")
            if discarding and not self._same_checks(stored, symplecticity):
                raise ConfigurationError(
                    f"{self.path} holds correlation functions whose trajectories were discarded at other steps or against "
                    "another tolerance than this batch's (\"check_symplecticity_every\", \"symplecticity_tolerance\"): they "
                    "are different estimators and cannot be pooled")
        stored['autocorrelation'] = (ntraj * autocorrelation + done * stored['autocorrelation']) / total
        stored['ic_correlation'] = (ntraj * ic_correlation + done * stored['ic_correlation']) / total
        stored['trajectories'] = total
        have = 'autocorrelation_second_moment' in stored
        if second_moments is not None and (have or done == 0):
            for name, new in zip(('autocorrelation', 'ic_correlation'), second_moments):
                key = name + '_second_moment'
                pooled = (ntraj * new + done * stored[key]) / total if have else np.asarray(new, dtype=np.float64)
                stored[key] = pooled
                stored[name + '_error'] = hostmath.standard_errors(stored[name], pooled / total, total)
        elif have or second_moments is not None:
            logger.warning("standard errors dropped from %s: %s", self.path,
                           "the stored trajectories have no second moments" if second_moments is not None else
                           "this task does not compute them (\"standard_errors\": true)")
            for key in self.ERROR_KEYS:
                stored.pop(key, None)
        have_blocks = 'autocorrelation_blocks' in stored
        fits = blocks is not None and (done == 0 or (have_blocks and stored['autocorrelation_blocks'].shape == np.shape(blocks[0])))
        if fits:
            pool = have_blocks and done > 0
            for key, new in zip(self.BLOCK_KEYS[:2], blocks[:2]):
                stored[key] = (ntraj * np.asarray(new) + done * stored[key]) / total if pool else np.asarray(new, dtype=complex)
            counts = np.asarray(blocks[2], dtype=np.int64)
            stored['block_trajectories'] = stored['block_trajectories'] + counts if pool else counts
        elif have_blocks or blocks is not None:
            logger.warning("error blocks dropped from %s: %s", self.path,
                           "this task does not compute them (\"error_blocks\": B)" if blocks is None else
                           "the stored trajectories have no blocks, or another number of them")
            for key in self.BLOCK_KEYS:
                stored.pop(key, None)
        have_checks = 'symplecticity_steps' in stored
        if symplecticity is not None and (done == 0 or (have_checks and self._same_checks(stored, symplecticity))):
            pool = have_checks and done > 0
            if not pool:
                for key in self.SYMPLECTICITY_KEYS:
                    stored.pop(key, None)
            new_max, new_mean = (np.asarray(symplecticity[key], dtype=np.float64) for key in ('max', 'mean'))
            stored['symplecticity_steps'] = np.asarray(symplecticity['steps'], dtype=np.int64)
            stored['symplecticity_max'] = np.maximum(stored['symplecticity_max'], new_max) if pool else new_max
            stored['symplecticity_mean'] = (ntraj * new_mean + done * stored['symplecticity_mean']) / total if pool else new_mean
            if 'tolerance' in symplecticity:
                counts = np.asarray(symplecticity['exceeding'], dtype=np.int64)
                stored['symplecticity_exceeding'] = stored['symplecticity_exceeding'] + counts if pool else counts
                stored['symplecticity_tolerance'] = float(symplecticity['tolerance'])
            if discarding:
                kept = np.asarray(symplecticity['kept'], dtype=np.int64)
                stored['symplecticity_kept'] = stored['symplecticity_kept'] + kept if pool else kept
                stored['symplecticity_discard'] = True
        elif have_checks or symplecticity is not None:
            logger.warning("symplecticity checks dropped from %s: %s", self.path,
                           "this task does not make them (\"check_symplecticity_every\": k)" if symplecticity is None else
                           "the stored trajectories have none, or were checked at other steps or against another tolerance")
            for key in self.SYMPLECTICITY_KEYS:
                stored.pop(key, None)
        for fam, record in records:
            if record is None:
                continue
            pool = done > 0
            new = np.asarray(record['correlation'], dtype=complex)
            for key in fam.idents + tuple(key for key in fam.optional if key in record):
                stored[fam.prefix + key] = np.asarray(record[key], dtype=np.float64)
            stored[fam.stored] = (ntraj * new + done * stored[fam.stored]) / total if pool else new
            moment = record.get('second_moment', None)
            key = fam.stored + '_second_moment'
            have_moment = key in stored
            if moment is not None and (have_moment or not pool):
                stored[key] = (ntraj * moment + done * stored[key]) / total if pool else np.asarray(moment, dtype=np.float64)
                stored[fam.stored + '_error'] = hostmath.standard_errors(stored[fam.stored], stored[key] / total, total)
            elif have_moment or moment is not None:
                logger.warning(f"standard errors of the {fam.what} dropped from %s: %s", self.path,
                               "the stored trajectories have no second moments" if moment is not None else
                               "this task does not compute them (\"standard_errors\": true)")
                for drop in (key, fam.stored + '_error'):
                    stored.pop(drop, None)
            for key in fam.stale:            # computed from the old correlation functions: stale now
                stored.pop(key, None)
        if time_average is not None:
            pool = done > 0
            new = np.asarray(time_average['spectrum'], dtype=np.float64)
            for key, name in zip(self.TA_IDENT_KEYS, ('energies', 'q', 'p', 'window')):
                stored[key] = np.asarray(time_average[name], dtype=np.float64)
            stored['ta_spectrum'] = (ntraj * new + done * stored['ta_spectrum']) / total if pool else new
            moment = time_average.get('second_moment', None)
            key = 'ta_spectrum_second_moment'
            have_moment = key in stored
            if moment is not None and (have_moment or not pool):
                stored[key] = (ntraj * moment + done * stored[key]) / total if pool else np.asarray(moment, dtype=np.float64)
                m3 = np.zeros(stored[key].shape + (3,))
                m3[..., 0] = stored[key] / total
                stored['ta_spectrum_error'] = hostmath.standard_errors(stored['ta_spectrum'], m3, total).real
            elif have_moment or moment is not None:
                logger.warning("standard errors of the time-averaged spectrum dropped from %s: %s", self.path,
                               "the stored trajectories have no second moments" if moment is not None else
                               "this task does not compute them (\"standard_errors\": true)")
                for drop in self.TA_ERROR_KEYS:
                    stored.pop(drop, None)
        stored.pop('ic_rate', None)          # a rate computed from the old correlation function is stale now
        stored.pop('ic_rate_error', None)
        logger.info(f"<phi(0)|phi(0)>= {stored['autocorrelation'][0]}")
        assert abs(stored['autocorrelation'][0] - 1.0) < 1.0e-3
        np.savez(self.path, **stored)

    @staticmethod
    def _same_checks(stored, symplecticity):
        """the stored symplecticity checks were made at the same steps and against the same tolerance (or none) as the new ones"""
        if not np.array_equal(stored['symplecticity_steps'], np.asarray(symplecticity['steps'])):
            return False
        if ('symplecticity_tolerance' in stored) != ('tolerance' in symplecticity):
            return False
        return 'tolerance' not in symplecticity or float(stored['symplecticity_tolerance']) == float(symplecticity['tolerance'])


# ---------------------------------------------------------------------------------------------------------------------
# dynamics
# ---------------------------------------------------------------------------------------------------------------------

def make_propagator(task, Gamma_0, device):
    """frozen Gaussians of the width of the initial wavepacket: Gamma_i = Gamma_t = Gamma_0 (cli.py:305-306, 376-383)"""
    if task.get('propagator', 'HK') == "WM":
        cell = task.get('cell_width', 10000.0)
        return propagators.WaltonManolopoulosPropagator(Gamma_0, Gamma_0, cell, cell, device=device)
    return propagators.HermanKlukPropagator(Gamma_0, Gamma_0, device=device)


def _check_symplecticity(propagator, step, time, tolerance, log, discard=False):
    """one symplecticity check of the batch: (step, max, mean, trajectories above the tolerance, trajectories kept) -- one host
    transfer.  ``discard``: the check also discards the trajectories above the tolerance (propagator.discard_nonsymplectic); max
    and mean are then taken over the trajectories that were still kept BEFORE this mark (one dead trajectory would otherwise make
    them +inf for the rest of the run; NaN once nobody is left), the last element is the number kept after it (else None)."""
    if discard:
        alive = propagator.kept
        eps = propagator.discard_nonsymplectic(tolerance)
        count = alive.sum().to(eps.dtype)
        lowest = torch.full_like(eps, -float("inf"))
        stats = [torch.where(alive, eps, lowest).max(), torch.where(alive, eps, torch.zeros_like(eps)).sum() / count,
                 (eps > tolerance).sum().to(eps.dtype), count, propagator.kept.sum().to(eps.dtype)]
        largest, mean, above, before, kept = torch.stack(stats).tolist()
        if before == 0:
            largest = mean = float("nan")
        exceeding, kept = int(above), int(kept)
    else:
        eps = propagator.symplectic_deviation()
        stats = [eps.max(), eps.mean()] + ([(eps > tolerance).sum().to(eps.dtype)] if tolerance is not None else [])
        largest, mean, *above = torch.stack(stats).tolist()
        exceeding, kept = (int(above[0]) if above else None), None
    if log:
        tail = "" if exceeding is None else f"  above {tolerance:g}: {exceeding} of {propagator.ntraj}"
        if kept is not None:
            tail += f"  kept {kept} of {propagator.ntraj}"
        logger.info(f" time/fs= {time * units.autime_to_fs}  symplecticity max= {largest:9.3e}  mean= {mean:9.3e}{tail}")
    return step, largest, mean, exceeding, kept


def propagate_batch(propagator, setup, dt, nt, times, norm_every=0, flush=None, across_ranks=False, log=True, errors=False,
                    error_blocks=0, symplecticity_every=0, symplecticity_tolerance=None, discard_nonsymplectic=False, targets=None,
                    operators=None, time_average=None):
    """C_auto(t), k_ic(t) of one batch of trajectories: the device loop leaves the raw per-step sums in a device buffer,
    ``flush`` (None on a single rank) adds the buffers of all ranks -- ONE all-reduce per batch, SURVEY 8e -- and the host
    applies the dynamical phase.  ``norm_every`` > 0 logs the wavefunction norm (the O(n^2) convergence diagnostic of
    cli.py:424-429) at every norm_every-th step by cutting the device loop there; with ``across_ranks`` it is the norm of
    the whole sharded batch (a collective: every rank calls it, ``log`` says who prints).  ``errors``: also the per-sample
    second moments (M_C, M_k) of the batch, (nt, 3) each (see CorrelationStore.add_batch), flushed in the same collective.
    ``error_blocks`` = B > 0: the last element of the result is (C_blocks, k_blocks, counts), the block sums (nt, B) of the batch
    with the phase applied and the trajectories per block (every rank partitions ITS trajectories by their local index; sums and
    counts are added over the ranks in the same collective).
    ``symplecticity_every`` = k > 0 cuts the device loop at every k-th step as well and checks the symplecticity of every
    trajectory's monodromy matrix there (propagator.symplectic_deviation, this rank's trajectories only); the result then ends
    with one more element, a dict with 'steps', 'max' and 'mean' of the deviation per check and, with a
    ``symplecticity_tolerance``, 'exceeding' (trajectories above it) and 'tolerance'.  Nothing else of the result changes.
    ``discard_nonsymplectic`` (needs both): every check discards the trajectories above the tolerance for the rest of the batch
    (propagator.discard_nonsymplectic: samples of value zero, N unchanged); 'max' and 'mean' are then over the trajectories still
    kept before the check, and the record gains 'kept' (the number kept after every check) and 'discard' = True.
    ``targets`` = (Q, P), arrays (K, D): the cross-correlation functions with these target coherent states (propagator.run(targets=...));
    the result then ends with one more element still, the record {'q', 'p', 'correlation' (nt, K)} and, with ``errors``,
    'second_moment' (nt, K, 3), the per-sample second moments as (M_C, M_k).  Single rank only: the flush does not carry them.
    ``operators`` = (bra_c, bra_m, ket_c, ket_m) or (..., bra_k, ket_k) with the Hessians (M, D, D) of quadratic operators: the
    operator correlation functions (propagator.run(operators=...)); the result then ends with yet another element, the record
    {'bra_c', 'bra_m', 'ket_c', 'ket_m', 'correlation' (nt, M)} (and 'bra_k', 'ket_k' when given) and, with ``errors``,
    'second_moment' (nt, M, 3).  Single rank only, for the same reason.  On a thermal ensemble they are the linear operators of
    propagator.run(thermal_operators=...) and fill the same record.
    ``time_average`` = (energies, q, p), arrays (NE,), (K, D), (K, D): the time-averaged spectrum of these reference states over
    the nt steps (propagator.time_average; ONE accumulator across all pieces of the loop, so the cuts change no bit of it); the
    result then ends with a last element, the record {'energies', 'q', 'p', 'window', 'spectrum' (K, NE)} and, with ``errors``,
    'second_moment' (K, NE).  Single rank only."""
    given = [(fam, idents) for fam, idents in zip(ROW_FAMILIES, (targets, operators)) if idents is not None]
    for fam, _ in given:
        if flush is not None:
            raise ValueError(f"{fam.noun} are not available with more than one rank: the flush buffer does not carry the {fam.rows} rows")
    if time_average is not None and flush is not None:
        raise ValueError("a time-averaged spectrum is not available with more than one rank: the flush buffer does not carry its sums")
    if discard_nonsymplectic and not (symplecticity_every > 0 and symplecticity_tolerance is not None):
        raise ValueError("discard_nonsymplectic needs symplecticity_every > 0 and a symplecticity_tolerance")
    slots = torch.zeros((nt, 5), dtype=torch.float64, device=propagator.device)
    moments = torch.zeros((nt, 6), dtype=torch.float64, device=propagator.device) if errors else None
    blocks = counts = None
    rows5 = []                                    # per family given: (family, its identifying arrays, the buffer of raw rows)
    for fam, idents in given:
        idents = tuple(np.asarray(a, dtype=np.float64) for a in idents)
        if idents[0].ndim != fam.ndim or idents[0].shape[0] == 0:
            raise ValueError(f"{fam.noun}: {fam.expected} expected, got {idents[0].shape}")
        rows5.append((fam, idents, torch.zeros((nt, idents[0].shape[0], 5), dtype=torch.float64, device=propagator.device)))
    if error_blocks:
        blocks = torch.zeros((nt, error_blocks, 4), dtype=torch.float64, device=propagator.device)
        counts = torch.from_numpy(propagator.block_counts(propagator.ntraj, error_blocks)).to(torch.float64)
    accumulator = None
    if time_average is not None:
        energies, ref_q, ref_p = time_average
        accumulator = propagator.time_average(energies, dt, None if ref_q is None else (ref_q, ref_p))
        extra_ta = {"time_average": accumulator}
    else:
        extra_ta = {}
    # the device loop is cut at the multiples of either diagnostic's period
    cuts = sorted({0} | {s for every in (norm_every, symplecticity_every) if every > 0 for s in range(0, nt, every)}) if nt > 0 else []
    pieces, checks = [], []
    for first, stop in zip(cuts, cuts[1:] + [nt]):
        if norm_every > 0 and first % norm_every == 0:
            norm = propagator.norm(across_ranks=across_ranks)
            if log:
                logger.info(f" time/fs= {times[first] * units.autime_to_fs}  norm= {norm:9.6f}")
        if symplecticity_every > 0 and first % symplecticity_every == 0:
            checks.append(_check_symplecticity(propagator, first, times[first], symplecticity_tolerance, log,
                                               discard=discard_nonsymplectic))
        count = stop - first
        pieces.append((first, count, propagator.t))
        extra = {}
        for fam, idents, buf in rows5:
            # on a thermal ensemble the operators are run()'s thermal_operators: the same rows
            prefix = "thermal_" if fam.noun == "operators" and getattr(propagator, "thermal_centres", None) is not None else ""
            extra.update({prefix + fam.noun: fam.as_run(idents), prefix + fam.buffer: buf[first:first + count]})
        propagator.run(setup.potential, dt, count, slots=slots[first:first + count],
                       moments=None if moments is None else moments[first:first + count],
                       blocks=None if blocks is None else blocks[first:first + count], **extra, **extra_ta)
    if symplecticity_every > 0 and pieces:
        # The clock of a piece is t0 + (dt + dt + ...), which differs from the uncut loop's 0 + dt + dt + ... in the last bits, and
        # with it the dynamical phase.  The check must leave every bit of the correlation functions as it is: the phase is taken
        # on the grid of the uncut loop (calc_norm_every alone keeps the grid it always had).
        pieces = [(0, nt, pieces[0][2])]
    if flush is not None:
        if blocks is not None:
            flush(slots, moments, blocks, counts)
        elif moments is None:
            flush(slots)
        else:
            flush(slots, moments)
    propagator.synchronize()                      # raises the energy-conservation error of this rank's trajectories
    tail = ()
    if blocks is not None:
        parts = [propagator.finalize_blocks(blocks[first:first + count], t0, dt, setup.zero_point_energy) for first, count, t0 in pieces]
        tail = (tuple(np.concatenate(part) for part in zip(*parts)) + (np.rint(counts.numpy()).astype(np.int64),),)
    if symplecticity_every > 0:
        steps, largest, mean, exceeding, kept = zip(*checks)
        record = {'steps': np.asarray(steps, dtype=np.int64), 'max': np.asarray(largest), 'mean': np.asarray(mean)}
        if symplecticity_tolerance is not None:
            record.update(exceeding=np.asarray(exceeding, dtype=np.int64), tolerance=float(symplecticity_tolerance))
        if discard_nonsymplectic:
            record.update(kept=np.asarray(kept, dtype=np.int64), discard=True)
        tail = tail + (record,)
    for fam, idents, buf in rows5:
        parts = [propagator.phased_cross(buf[first:first + count], t0, dt, setup.zero_point_energy) for first, count, t0 in pieces]
        X, m3 = (np.concatenate(part) for part in zip(*parts))
        record = dict(zip(fam.idents + fam.optional, idents), correlation=X)
        if errors:
            record['second_moment'] = propagator._ntraj_norm * m3
        tail = tail + (record,)
    if accumulator is not None:
        raw = accumulator.raw_sums()
        T, n = accumulator.window, propagator._ntraj_norm
        record = {'energies': accumulator.energies, 'q': accumulator.references[0], 'p': accumulator.references[1], 'window': T,
                  'spectrum': raw[..., 0] / T}
        if errors:
            record['second_moment'] = n * raw[..., 1] / T ** 2
        tail = tail + (record,)
    if moments is None:
        parts = [propagator.finalize_slots(slots[first:first + count], t0, dt, setup.zero_point_energy)
                 for first, count, t0 in pieces]
        return tuple(np.concatenate(part) for part in zip(*parts)) + tail
    parts = [propagator.phased_moments(slots[first:first + count], moments[first:first + count], t0, dt, setup.zero_point_energy)
             for first, count, t0 in pieces]
    C, k, mC, mk = (np.concatenate(part) for part in zip(*parts))
    n = propagator._ntraj_norm
    return (C, k, n * mC, n * mk) + tail


def _load_targets(path, dim):
    """(q, p), float64 (K, D), of a "cross_correlation_targets" file"""
    try:
        with np.load(path, allow_pickle=False) as handle:
            q, p = (np.array(handle[key], dtype=np.float64) for key in ('q', 'p'))
    except (OSError, KeyError, ValueError) as err:
        raise ConfigurationError(f"'cross_correlation_targets': {path} should be an npz file with arrays q and p ({err})")
    if q.ndim != 2 or q.shape != p.shape or q.shape[0] == 0 or q.shape[1] != dim:
        raise ConfigurationError(f"'cross_correlation_targets': q and p of shape (K, {dim}) with K > 0 are expected in {path}, got "
                                 f"{q.shape} and {p.shape}")
    if not (np.isfinite(q).all() and np.isfinite(p).all()):
        raise ConfigurationError(f"'cross_correlation_targets': non-finite entry in {path}")
    return q, p


def _load_time_average(path, setup):
    """(energies, q, p), float64 (NE,), (K, D), (K, D), of a "time_averaged_spectrum" file: the array energies (Hartree) and
    optionally the reference states q and p; without them the one state (q0, p0) of the initial wavepacket"""
    dim = int(setup.q0.shape[0])
    try:
        with np.load(path, allow_pickle=False) as handle:
            energies = np.array(handle['energies'], dtype=np.float64)
            if ('q' in handle) != ('p' in handle):
                raise KeyError("q and p come together")
            q, p = ((np.array(handle[key], dtype=np.float64) for key in ('q', 'p')) if 'q' in handle else
                    (setup.q0.numpy()[None, :].copy(), setup.p0.numpy()[None, :].copy()))
    except (OSError, KeyError, ValueError) as err:
        raise ConfigurationError(f"'time_averaged_spectrum': {path} should be an npz file with an array energies (and q, p) ({err})")
    if energies.ndim != 1 or energies.shape[0] == 0 or not np.isfinite(energies).all():
        raise ConfigurationError(f"'time_averaged_spectrum': finite energies of shape (NE,) with NE > 0 are expected in {path}, got "
                                 f"shape {energies.shape}")
    if q.ndim != 2 or q.shape != p.shape or q.shape[0] == 0 or q.shape[0] > 64 or q.shape[1] != dim:
        raise ConfigurationError(f"'time_averaged_spectrum': q and p of shape (K, {dim}) with 0 < K <= 64 are expected in {path}, got "
                                 f"{q.shape} and {p.shape}")
    if not (np.isfinite(q).all() and np.isfinite(p).all()):
        raise ConfigurationError(f"'time_averaged_spectrum': non-finite entry in {path}")
    return energies, q, p


def _load_operators(path, dim):
    """(bra_c, bra_m, ket_c, ket_m), float64 (M,) and (M, D), of an "operator_correlation" file; without ket_c and ket_m the ket's
    operators are the bra's.  With bra_k or ket_k (M, D, D), the symmetric Hessians of quadratic operators,
    the result is (..., bra_k, ket_k): a ket without ket_c, ket_m and ket_k takes the bra's K as well, every other K left out is
    zero."""
    try:
        with np.load(path, allow_pickle=False) as handle:
            bra_c, bra_m = (np.array(handle[key], dtype=np.float64) for key in ('bra_c', 'bra_m'))
            if ('ket_c' in handle) != ('ket_m' in handle):
                raise KeyError("ket_c and ket_m come together")
            ket_c, ket_m = ((np.array(handle[key], dtype=np.float64) for key in ('ket_c', 'ket_m')) if 'ket_c' in handle else
                            (bra_c.copy(), bra_m.copy()))
            hessians = {key: np.array(handle[key], dtype=np.float64) for key in ('bra_k', 'ket_k') if key in handle}
            whole_ket = 'ket_c' not in handle and 'ket_k' not in handle
    except (OSError, KeyError, ValueError) as err:
        raise ConfigurationError(f"'operator_correlation': {path} should be an npz file with arrays bra_c and bra_m (and ket_c, "
                                 f"ket_m) ({err})")
    for side, c, m in (("bra", bra_c, bra_m), ("ket", ket_c, ket_m)):
        if c.ndim != 1 or c.shape[0] == 0 or m.shape != (c.shape[0], dim) or c.shape != bra_c.shape:
            raise ConfigurationError(f"'operator_correlation': {side}_c of shape (M,) and {side}_m of shape (M, {dim}) with M > 0 are "
                                     f"expected in {path}, got {c.shape} and {m.shape}")
        if not (np.isfinite(c).all() and np.isfinite(m).all()):
            raise ConfigurationError(f"'operator_correlation': non-finite entry in {path}")
    if not hessians:
        return bra_c, bra_m, ket_c, ket_m
    shape = (bra_c.shape[0], dim, dim)
    for key, k in hessians.items():
        if k.shape != shape or not np.isfinite(k).all() or abs(k - np.swapaxes(k, 1, 2)).max() > 1.0e-12 * abs(k).max():
            raise ConfigurationError(f"'operator_correlation': {key} of shape {shape}, finite and symmetric, is expected in {path}")
    bra_k = hessians.get('bra_k', np.zeros(shape))
    return bra_c, bra_m, ket_c, ket_m, bra_k, hessians.get('ket_k', bra_k.copy() if whole_ket else np.zeros(shape))


def run_semiclassical_dynamics(task, device='cuda', comm=None):
    """One 'dynamics' task.  Under ``torch.distributed`` with more than one rank (``python -m semiclassical_amd.driver
    dynamics input.json --gpus N`` or torchrun; north_star: "trajectory batches shard embarrassingly across the 8 GPUs of
    one node with a single RCCL all-reduce ... per flush") every rank integrates ITS share of each batch of the
    reference's repetition loop (cli.py:321-324, 374-476) on its own GPU with the batch size as Monte-Carlo weight, one
    all-reduce per batch adds the raw sums, and rank 0 keeps the result file.  ``comm``: an
    ``distributed.RcclCommunicator`` to flush through the C-ABI's sc_flush_allreduce instead of the process group."""
    from . import distributed as Dm
    torch.set_default_dtype(torch.float64)
    rank, world = Dm.get_rank(), Dm.world_size()
    if comm is not None:
        rank, world = comm.rank, comm.world
    writer = rank == 0
    # per-trajectory symplecticity of the monodromy matrices at every k-th step (keys the reference does not have), 0 = off
    check_every = task.get('check_symplecticity_every', 0) or 0
    tolerance = task.get('symplecticity_tolerance', None)
    if isinstance(check_every, bool) or not isinstance(check_every, int) or check_every < 0:
        raise ConfigurationError(f"'check_symplecticity_every' should be a non-negative integer, got {check_every!r}")
    if tolerance is not None and (isinstance(tolerance, bool) or not isinstance(tolerance, (int, float)) or not tolerance > 0):
        raise ConfigurationError(f"'symplecticity_tolerance' should be a positive number, got {tolerance!r}")
    # discard the trajectories that fail the check for the rest of their batch (a key the reference does not have)
    discard = task.get('discard_nonsymplectic', False)
    if not isinstance(discard, bool):
        raise ConfigurationError(f"'discard_nonsymplectic' should be true or false, got {discard!r}")
    if discard and not check_every:
        raise ConfigurationError("'discard_nonsymplectic' needs 'check_symplecticity_every': k > 0, the steps at which the "
                                 "trajectories are judged")
    if discard and tolerance is None:
        raise ConfigurationError("'discard_nonsymplectic' needs 'symplecticity_tolerance', the deviation above which a trajectory "
                                 "is discarded")
    if discard and world > 1:
        raise ConfigurationError("'discard_nonsymplectic' is not available with more than one rank: the symplecticity check it "
                                 "rests on is not")
    if check_every and world > 1:
        raise ConfigurationError("'check_symplecticity_every' is not available with more than one rank: the maximum over the "
                                 "trajectories does not fit the one sum all-reduce per batch")
    # Two keys the reference does not have, an npz file each, atomic units, in the coordinates of q0.  "cross_correlation_targets":
    # cross-correlation functions with target coherent states, arrays q and p (K, D).  "operator_correlation":
    # correlation functions with linear operators on both sides, arrays bra_c (M,), bra_m (M, D) and optionally
    # ket_c, ket_m; quadratic operators with bra_k (M, D, D) and optionally ket_k.
    targets_file, operators_file = (task.get(fam.task_key, None) for fam in ROW_FAMILIES)
    for fam, file in zip(ROW_FAMILIES, (targets_file, operators_file)):
        if file is not None and task.get('propagator', 'HK') == "WM":
            raise ConfigurationError(f"'{fam.task_key}' is not available with the WM propagator: its Gaussians have "
                                     "per-trajectory widths and another prefactor")
        if file is not None and world > 1:
            raise ConfigurationError(f"'{fam.task_key}' is not available with more than one rank: the flush buffer does not "
                                     f"carry the {fam.rows} rows")
    # "time_averaged_spectrum": the time-averaged HK spectrum I(E) over the whole run, an npz file with the array
    # energies (NE,), Hartree, and optionally the reference states q and p (K, D)
    ta_file = task.get('time_averaged_spectrum', None)
    if ta_file is not None and task.get('propagator', 'HK') == "WM":
        raise ConfigurationError("'time_averaged_spectrum' is not available with the WM propagator: its Gaussians have "
                                 "per-trajectory widths and another prefactor")
    if ta_file is not None and world > 1:
        raise ConfigurationError("'time_averaged_spectrum' is not available with more than one rank: the flush buffer does not "
                                 "carry its sums")
    # "temperature": Kelvin (a key the reference does not have).  The trajectories then sample the canonical
    # ensemble of the harmonic initial surface (widths Gamma_0, masses of the task's potential) instead of its ground state.
    kelvin = task.get('temperature', None)
    if kelvin is not None:
        if isinstance(kelvin, bool) or not isinstance(kelvin, (int, float)) or not (kelvin >= 0 and np.isfinite(kelvin)):
            raise ConfigurationError(f"'temperature' should be a non-negative number (Kelvin), got {kelvin!r}")
        if task.get('propagator', 'HK') == "WM":
            raise ConfigurationError("'temperature' is not available with the WM propagator: the thermal estimator is the "
                                     "Herman-Kluk expression with per-trajectory centres")
        # ("operator_correlation" is: linear operators on a thermal ensemble)
        for key in ('cross_correlation_targets', 'time_averaged_spectrum'):
            if task.get(key, None) is not None:
                raise ConfigurationError(f"'{key}' is not available with 'temperature': its kernel takes the one centre (q0, p0)")
        if task.get('calc_norm_every', 0):
            raise ConfigurationError("'calc_norm_every' is not available with 'temperature': the norm describes one pure state")
    setup = build_problem(task)
    time_average = None if ta_file is None else _load_time_average(ta_file, setup)
    targets = None if targets_file is None else _load_targets(targets_file, int(setup.q0.shape[0]))
    operators = None if operators_file is None else _load_operators(operators_file, int(setup.q0.shape[0]))
    if kelvin is not None and operators is not None and len(operators) > 4:
        raise ConfigurationError("'operator_correlation' with bra_k or ket_k is not available with 'temperature': the task's thermal "
                                 "operator correlation functions take linear operators (from Python: "
                                 "HermanKlukPropagator.thermal_quadratic_correlation / run(thermal_quadratic=...))")

    dt = task['time_step_fs'] / units.autime_to_fs
    nt = task['num_steps']
    # the stored grid has spacing nt dt / (nt - 1) while the propagator advances by dt (cli.py:312-313)
    times = torch.linspace(0.0, nt * dt, nt)

    batch_size = task.get('batch_size', 10000)
    num_trajectories = task.get('num_trajectories', 50000)
    repetitions = max(num_trajectories // batch_size, 1)
    per_batch = min(batch_size, num_trajectories)
    mine = Dm.shard_slice(per_batch, rank, world)            # this rank's trajectories of every batch
    if mine.stop == mine.start:
        raise ConfigurationError(f"batches of {per_batch} trajectories cannot be shared by {world} ranks")

    store = CorrelationStore(task['results'].get('correlations', 'correlations.npz'))
    if writer:
        store.start(task, task.get('propagator', 'HK'), times, setup, cross_targets=targets, operators=operators,
                    time_average=None if time_average is None else time_average + (nt * dt,), temperature=kelvin)

    seed = task.get('manual_seed', None)
    if seed is not None:
        logger.warning("The random number generator should not be seeded manually unless for debugging!")
    # Where the phase-space points are drawn (a key the reference does not have; it samples on its compute device,
    # cli.py:392 -> propagators.py:537-539): "device" = sc_sample_initial (counter-based Philox keyed by the seed, one
    # subsequence per repetition, nothing crosses PCIe; a rank draws ITS slice of the batch), "host" = torch's CPU
    # generator as in the reference's CPU runs (ranks sharing a batch all draw the whole batch from the same seed).
    sampling = task.get('sampling', 'device')
    if sampling not in ('device', 'host'):
        raise ValueError("'sampling' should be one of 'device' or 'host'")
    if seed is None and world > 1:
        seed_all = Dm.broadcast_object(int.from_bytes(os.urandom(7), 'little'))     # fresh entropy, the same on every rank
    else:
        seed_all = seed
    if seed_all is not None and (seed is not None or sampling == 'host'):
        torch.manual_seed(seed_all)
    device_seed = int(seed_all) if seed_all is not None else int.from_bytes(os.urandom(8), 'little')

    if comm is not None:
        flush = lambda slots, moments=None, blocks=None, counts=None: Dm.flush_correlations(slots, moments, blocks, counts, comm=comm)
    elif world > 1:
        flush = Dm.flush_correlations
    else:
        flush = None

    for repetition in range(repetitions):
        logger.info(f"*** Repetition {repetition + 1} ***")
        propagator = make_propagator(task, setup.Gamma_0, device)
        count = mine.stop - mine.start
        if kelvin is not None:
            thermal = (setup.q0, setup.p0, setup.Gamma_0, setup.potential.masses(), units.kelvin_to_hartree * float(kelvin))
            try:
                if sampling == 'device':
                    propagator.thermal_initial_conditions(*thermal, ntraj=count, ntraj_total=per_batch, seed=device_seed,
                                                          subsequence=repetition, first_index=mine.start)
                elif world == 1:
                    propagator.thermal_initial_conditions(*thermal, ntraj=per_batch)
                else:
                    raise ConfigurationError("'temperature' with 'sampling': 'host' is not available with more than one rank")
            except ValueError as err:
                raise ConfigurationError(f"'temperature': {err}")
        elif sampling == 'device':
            propagator.initial_conditions(setup.q0, setup.p0, setup.Gamma_0, ntraj=count, ntraj_total=per_batch,
                                          seed=device_seed, subsequence=repetition, first_index=mine.start)
        elif world == 1:
            propagator.initial_conditions(setup.q0, setup.p0, setup.Gamma_0, ntraj=per_batch)
        else:
            zi, probi = propagator.draw_initial_conditions(setup.q0, setup.p0, setup.Gamma_0, per_batch)
            propagator.set_initial_conditions(setup.q0, setup.p0, setup.Gamma_0, zi[:, mine], probi[mine],
                                              ntraj_total=per_batch)
        errors = bool(task.get('standard_errors', False))
        # error bars of the rate by batch means (a key the reference does not have): B blocks per batch, 0 = off
        error_blocks = int(task.get('error_blocks', 0) or 0)
        if error_blocks and not hostmath.valid_error_blocks(error_blocks):
            raise ConfigurationError(f"'error_blocks' should be a power of two in 2 ... 64 (or 0), got {error_blocks}")
        out = propagate_batch(propagator, setup, dt, nt, times, norm_every=task.get('calc_norm_every', 0), flush=flush,
                              across_ranks=world > 1 and comm is None, log=writer, errors=errors, error_blocks=error_blocks,
                              symplecticity_every=check_every, symplecticity_tolerance=tolerance, discard_nonsymplectic=discard,
                              targets=targets, operators=operators, time_average=time_average)
        records = {}
        if time_average is not None:
            out, records['time_average'] = out[:-1], out[-1]
        for fam, idents in reversed(list(zip(ROW_FAMILIES, (targets, operators)))):
            if idents is not None:
                out, records[fam.noun] = out[:-1], out[-1]
        checks = None
        if check_every:
            out, checks = out[:-1], out[-1]
        autocorrelation, ic_correlation = out[:2]
        assert not np.isnan(autocorrelation).any(), f"encountered NaN's in autocorrelation : {autocorrelation}"
        assert not np.isnan(ic_correlation).any(), f"encountered NaN's in IC correlation : {ic_correlation}"
        if writer:
            store.add_batch(autocorrelation, ic_correlation, per_batch, second_moments=out[2:4] if errors else None,
                            blocks=out[-1] if error_blocks else None, symplecticity=checks, cross=records.get('targets'),
                            operators=records.get('operators'), time_average=records.get('time_average'), temperature=kelvin)


# ---------------------------------------------------------------------------------------------------------------------
# rates
# ---------------------------------------------------------------------------------------------------------------------

def lineshape_from_task(task):
    """damping function of the 'broadening' keys; widths are half widths at half maximum in eV (cli.py:524-545)"""
    kind = task.get('broadening', 'gaussian')
    hwhm_gauss, hwhm_lorentz = task.get('hwhmG_ev', 0.01), task.get('hwhmL_ev', 1.0e-6)
    sigma = hwhm_gauss / np.sqrt(2.0 * np.log(2.0)) / units.hartree_to_ev
    gamma = hwhm_lorentz / units.hartree_to_ev
    shapes = {"gaussian": lambda: broadening.gaussian(sigma),
              "lorentzian": lambda: broadening.lorentzian(gamma),
              "voigtian": lambda: broadening.voigtian(sigma, gamma)}
    if kind not in shapes:
        raise ValueError("'broadening' should be one of 'gaussian', 'lorentzian' or 'voigtian'")
    return shapes[kind](), {'broadening': kind, 'hwhmG': hwhm_gauss, 'hwhmL': hwhm_lorentz}


def calculate_rates(task):
    """k_ic(E) from the stored k_ic(t): damped Fourier transform, factor 2 pi, non-negative energies (cli.py:547-570)"""
    lineshape, record = lineshape_from_task(task)
    stored = dict(np.load(task.get('correlations', 'correlations.npz')))
    stored.update(record)
    energies, spectrum = rates.rate_from_correlation(stored['times'], stored['ic_correlation'], lineshape)
    keep = energies >= 0.0
    stored['energies'] = energies[keep]
    stored['ic_rate'] = (2.0 * np.pi * spectrum)[keep].real
    stored.pop('ic_rate_error', None)
    if all(key in stored for key in CorrelationStore.BLOCK_KEYS):
        # Monte-Carlo standard error of the rate at every energy from the spread of the blocks' own rates (batch means)
        _, sigma = rates.rate_standard_error(stored['times'], stored['ic_correlation_blocks'], stored['block_trajectories'], lineshape)
        stored['ic_rate_error'] = (2.0 * np.pi * sigma)[keep]
    for key in ('operator_lineshape', 'radiative_rate'):
        stored.pop(key, None)
    if 'operator_correlation' in stored:
        # emission lineshapes G_a(E) of the operator correlation functions on the same energies; their sum is the lineshape of the
        # dipole correlation function when the operators are the components of a transition dipole
        X = stored['operator_correlation']
        shapes = np.stack([rates.lineshape_from_correlation(stored['times'], X[:, a], lineshape)[1] for a in range(X.shape[1])], axis=1)
        stored['operator_lineshape'] = shapes[keep].real
        gap_ev = task.get('adiabatic_gap_ev', None)
        if gap_ev is not None:
            stored['radiative_rate'] = rates.radiative_rate(stored['energies'], stored['operator_lineshape'].sum(axis=1),
                                                            gap_ev / units.hartree_to_ev)
    np.savez(task.get('rates', 'correlations.npz'), **stored)


def main(argv=None):
    logging.basicConfig(format="[%(module)-12s] %(message)s", level=logging.INFO)
    parser = argparse.ArgumentParser(prog="semi (semiclassical_amd)")
    sub = parser.add_subparsers(dest='command')
    dyn = sub.add_parser('dynamics', help="run semiclassical dynamics")
    dyn.add_argument('json_input', type=str, metavar='input.json')
    dyn.add_argument('--cuda', type=int, default=None, metavar='id',
                     help="GPU of this process (default: 0, or LOCAL_RANK in a multi-rank job)")
    dyn.add_argument('--gpus', type=int, default=1, metavar='N',
                     help="share every batch of trajectories among N GPUs of this node: starts N rank processes (one per "
                          "GPU, RCCL process group) unless a launcher (torchrun) has already done so")
    rat = sub.add_parser('rates', help="Fourier transform correlation functions into rates")
    rat.add_argument('json_input', type=str, metavar='input.json')
    args = parser.parse_args(argv)
    if args.command == 'dynamics' and args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # self-launch: this parent never touches the GPU, it starts one rank process per GPU and waits for them
        import sys
        from . import distributed as Dm
        forwarded = list(sys.argv[1:] if argv is None else argv)
        raise SystemExit(Dm.launch_local_ranks(["-m", "semiclassical_amd.driver"] + forwarded, args.gpus))
    with open(args.json_input) as f:
        config = json.load(f)
    if args.command == 'dynamics':
        from . import distributed as Dm
        rank, world, local = Dm.init_from_env()
        cuda = args.cuda if args.cuda is not None else (local if world > 1 else 0)
        if world > 1 and rank != 0:
            logging.getLogger().setLevel(logging.WARNING)          # one voice per job
        handler = lambda task: run_semiclassical_dynamics(task, device=f"cuda:{cuda}")
    else:
        world, handler = 1, calculate_rates
    for task in config['semi']:
        if task['task'] == args.command:
            handler(task)
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
