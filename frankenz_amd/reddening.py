"""
The IGM attenuation of ``frankenz.reddening`` (reference reddening.py:23-95): the Madau (1995) effective transmission as NumPy on
the host, with the reference's signatures and values.  ``frankenz_amd.simulate`` evaluates the same arithmetic on the GPU from the
tables of ``line_table`` / ``continuum_table`` (docs/simulate.md).
"""
import numpy as np

__all__ = ["_madau_t1", "_madau_tau1", "_madau_tau2", "madau_teff"]

# n -> 1 transitions (n = 2, 3, ..., 12) and their coefficients (reddening.py:47-50)
_LINES = (1216.0, 1026.0, 973.0, 950.0, 938.1, 931.0, 926.5, 923.4, 921.2, 919.6, 918.4)
_COEFFS = (0.0037, 0.00177, 0.00106, 0.000584, 0.00044, 0.00040, 0.00037, 0.00035, 0.00033, 0.00032, 0.00031)
# exponents of wave / 912 in the continuum term (reddening.py:72-75), in the order of the device table
_CONT_POWERS = (3, 0.46, 1.5, 0.18, -1.32, 1.68)


def _madau_t1(wave, z, l, coeff):
    """Optical depth at the wavelengths ``wave`` at redshift ``z`` from the line at ``l`` with coefficient ``coeff``."""
    zlambda = l * (1 + z)
    tau = np.zeros_like(wave)
    sel = wave < zlambda                                    # strict
    tau[sel] = coeff * (wave[sel] / l) ** 3.46
    return tau


def _madau_tau1(wave, z):
    """Optical depth of the 11 Lyman lines (912-1216 A) at the wavelengths ``wave`` at redshift ``z``."""
    tau1 = np.zeros_like(wave)
    for l, c in zip(_LINES, _COEFFS):
        tau1 += _madau_t1(wave, z, l, c)
    return tau1


def _madau_tau2(wave, z):
    """Optical depth of the continuum (< 912 A) at the wavelengths ``wave`` at redshift ``z``, floored at 0."""
    zlambda = 912.0 * (1 + z)
    tau2 = np.zeros_like(wave)
    sel = wave < zlambda
    xc = wave[sel] / 912.0
    xem = 1. + z
    tau2[sel] = ((0.25 * (xc**3) * (xem**0.46 - xc**0.46)) +
                 (9.4 * (xc**1.5) * (xem**0.18 - xc**0.18)) -
                 (0.7 * (xc**3) * (xc**-1.32 - xem**-1.32)) -
                 (0.023 * (xem**1.68 - xc**1.68)))
    tau2[tau2 < 0.] = 0.
    return tau2


def madau_teff(wave, z):
    """Effective transmission ``exp(-(tau1 + tau2))`` of the IGM at the wavelengths ``wave`` at redshift ``z``."""
    tau = _madau_tau1(wave, z) + _madau_tau2(wave, z)
    return np.exp(-tau)


def line_table(wave):
    """(len(wave), 12): column j holds the first j line terms ``coeff_i * (wave / l_i)**3.46`` added in the order of
    ``_madau_tau1`` (column 0 is 0).  The lines descend, so at redshift z the lines that reach a wavelength are the first
    ``n = sum(wave < l_i * (1 + z))`` of them and ``_madau_tau1(wave, z) == table[:, n]`` bit for bit (the others add 0)."""
    wave = np.asarray(wave, dtype=np.float64)
    tab = np.zeros((len(wave), len(_LINES) + 1))
    for j, (l, c) in enumerate(zip(_LINES, _COEFFS)):
        tab[:, j + 1] = tab[:, j] + c * (wave / l) ** 3.46
    return tab


def continuum_table(wave):
    """(len(wave), 6): ``(wave / 912)**p`` for the exponents of ``_madau_tau2``: its z-independent powers"""
    xc = np.asarray(wave, dtype=np.float64) / 912.0
    return np.stack([xc**p for p in _CONT_POWERS], axis=1)
