"""Rate constants k(E) by Fourier transform of a damped correlation function.

Host-side NumPy, one inverse FFT of 2 nt - 1 points per run; follows
reference semiclassical/rates.py:20-82 including the cos^2 switching function and the unit conversion to s^-1.
"""
import numpy as np
from numpy import fft

from . import hostmath, units

__all__ = ['rate_from_correlation', 'rate_standard_error', 'lineshape_from_correlation', 'radiative_rate']


def _damped_transform(times, correlation, lineshape):
    """int dt exp(i E t/hbar) f(t) c(t) over -t_max ... t_max with c(-t) = c(t)^* and the cos^2 switching function, on the grid
    conjugate to ``times``, in atomic units: (energies, transform), both of length 2 nt - 1, sorted by energy"""
    assert times.min() == 0.0, "time grid `times` should start at 0.0"
    assert times.shape == correlation.shape, "arrays `times` and `correlation` should have the same length"
    nt = times.shape[0]
    t_max = times.max()
    m = 2 * nt - 1
    full_times = np.linspace(-t_max, t_max, m)
    energies = fft.fftfreq(m) * m / (2 * t_max) * 2.0 * np.pi
    full = np.zeros(m, dtype=complex)
    full[m // 2:] = correlation                       # t >= 0
    full[:m // 2] = correlation[1:].conj()[::-1]      # k(-t) = k(t)^*
    damp = np.cos(0.5 * np.pi * full_times / t_max) ** 2
    rate = 2 * t_max * fft.ifft(fft.ifftshift(damp * lineshape(full_times) * full))
    return fft.fftshift(energies), fft.fftshift(rate)


def rate_from_correlation(times, correlation, lineshape):
    """k(E) = 1/(2 pi hbar) int dt exp(i E t/hbar) f(t) k(t) on the grid conjugate to ``times``.

    times: equidistant grid starting at 0; correlation: complex (nt,); lineshape: callable f(t).
    Returns (energies [Hartree], rate [s^-1]), both of length 2 nt - 1, sorted by energy.
    """
    energies, rate = _damped_transform(times, correlation, lineshape)
    rate *= 1.0e15 / units.autime_to_fs
    return energies, rate


def lineshape_from_correlation(times, correlation, lineshape):
    """G(E) = 1/(2 pi hbar) int dt exp(i E t/hbar) f(t) C(t): the transform of ``rate_from_correlation`` on the same energy grid,
    normalised as a density in atomic units (1 / Hartree) -- its sum times the grid spacing is f(0) C(0) -- and not converted to
    s^-1.  Returns (energies [Hartree], G), both of length 2 nt - 1, sorted by energy."""
    energies, transform = _damped_transform(times, correlation, lineshape)
    return energies, transform / (2.0 * np.pi * units.hbar)


def radiative_rate(energies, G, gap):
    """k_r = 4 / (3 hbar^4 c^3) int_{eps > 0} eps^3 G(gap - eps) d eps in s^-1: the spontaneous-emission rate from the emission
    lineshape G(E) of a dipole correlation function (``lineshape_from_correlation``; E is the vibrational energy left in the final
    state, eps = gap - E the photon's).  energies, G: real (nE,), atomic units, any order; gap: the adiabatic gap in Hartree.
    Trapezoid rule on the grid given, the integrand taken as zero where eps <= 0."""
    energies, G = np.asarray(energies, dtype=np.float64), np.asarray(G, dtype=np.float64)
    assert energies.ndim == 1 and energies.shape == G.shape, "arrays `energies` and `G` should have the same length"
    order = np.argsort(energies)
    E = energies[order]
    eps = gap - E
    y = np.where(eps > 0.0, eps ** 3 * G[order], 0.0)
    integral = 0.5 * np.sum((y[1:] + y[:-1]) * np.diff(E))
    return 4.0 / (3.0 * units.hbar ** 4 * units.speed_of_light ** 3) * integral * 1.0e15 / units.autime_to_fs


def rate_standard_error(times, correlation_blocks, counts, lineshape):
    """Monte-Carlo standard error of the rate of ``rate_from_correlation`` by batch means.

    correlation_blocks: complex (nt, B), the block sums of k(t) (phase applied; their sum over the blocks is the k(t) the rate is
    computed from); counts: (B,) trajectories per block.  The transform is linear in k(t): it is applied to every block's own
    estimate ``blocks[:, b] N / n_b`` and the error follows from the spread of the B rates (hostmath.block_standard_error), which
    carries the correlation between the time steps that per-step errors cannot.  Returns (energies, sigma) on the grid and in the
    unit of ``rate_from_correlation``; sigma is the error of the real part of the rate.  Empty blocks are left out."""
    blocks = np.asarray(correlation_blocks)
    counts = np.asarray(counts, dtype=np.float64)
    assert blocks.ndim == 2 and blocks.shape == (times.shape[0], counts.shape[0]), "`correlation_blocks` should have the shape (nt, B)"
    total = counts.sum()
    filled = np.flatnonzero(counts > 0)
    energies, values = None, []
    for b in filled:
        energies, rate = rate_from_correlation(times, blocks[:, b] * (total / counts[b]), lineshape)
        values.append(rate.real)
    if energies is None:
        energies, _ = rate_from_correlation(times, np.zeros(times.shape[0], dtype=complex), lineshape)
        return energies, np.full(energies.shape, np.nan)
    return energies, hostmath.block_standard_error(np.array(values), counts[filled])
