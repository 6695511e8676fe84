"""Atomic units and conversion factors.

Values are bit-identical to the reference (semiclassical/units.py:8-18): they
enter dt, the mode frequencies and the masses, so parity depends on them.
"""
hbar = 1.0

hartree_to_wavenumbers = 219474.63
hartree_to_ev = 27.211396132
bohr_to_angs = 0.529177249
autime_to_fs = 0.02418884326505
amu_to_aumass = 1822.888486192

# not in the reference: the speed of light in atomic units, 1 / alpha (CODATA 2018), for the radiative rate (rates.radiative_rate)
speed_of_light = 137.035999084

# not in the reference: k_B in Hartree per Kelvin (CODATA 2018), for thermal ensembles (k_B T = kelvin_to_hartree * T / K)
kelvin_to_hartree = 3.166811563e-6
