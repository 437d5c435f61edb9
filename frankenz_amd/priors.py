"""
The magnitude-dependent priors of ``frankenz.priors`` (reference priors.py:27-235): ``pmag``, ``_bpz_prior``, ``bpz_pt_m`` and
``bpz_pz_tm`` as vectorised NumPy on the host, and ``logprob_bpz``, the ``lprob_func`` that evaluates ln P(z_j, t_j | m_i) for
every (object, model) pair on the GPU (demos/2 cells 43 and 69-71, ``lprob_bpz``).

The BPZ prior (Benitez 2000, table 1) is tabulated once on the reference's own 1000 x 1000 x 3 grid over (m, z, t) and read by
linear interpolation, as the reference's ``RegularGridInterpolator`` reads it.  It is linear in m, so for a fixed model set the
prior of object i is a blend of two rows of a (1000, Nmodel) table (``pdf.logprob_prior_lerp``; docs/bpz_prior.md).
"""
import numpy as np

from . import pdf as _pdf
from .engine import DeviceArray, get_engine

__all__ = ["pmag", "_bpz_prior", "bpz_pt_m", "bpz_pz_tm", "logprob_bpz"]

# the grid of the tabulated prior (priors.py:171-172, 225-226)
_MGRID = np.linspace(20., 32., 1000)
_ZGRID = np.linspace(0., 15., 1000)
_TGRID = np.array([0., 1., 2.])

# Benitez (2000), table 1: p(z | t, m) ~ z^a exp(-(z / zm)^a) with zm = zo + km (m - 20); type fractions f_t = fo_t exp(-k_t (m - 20))
# for t = E/S0, Spiral, and the remainder for Irr
_A = np.array([2.465, 1.806, 0.906])
_ZO = np.array([0.431, 0.390, 0.0626])
_KM = np.array([0.0913, 0.0636, 0.123])
_KT = np.array([0.450, 0.147])
_FO = np.array([0.35, 0.5])

_base = {}          # 'ptm': (1000, 3), 'pztm': (1000, 1000, 3) -- built on first use, like the reference's module globals


def pmag(mag, maglim, mbounds=(10., 28.), alpha=15., beta=2., gamma=1., Npoints=1000, *args, **kwargs):
    """P(mag) for a 5-sigma limiting magnitude ``maglim`` (priors.py:27-73): ``mag**alpha * exp(-(mag / (maglim - gamma))**beta)``
    tabulated on ``Npoints`` magnitudes over ``mbounds``, normalised to unit (trapezoid) integral, read by ``np.interp``."""
    m = np.linspace(mbounds[0], mbounds[1], Npoints)
    p = m**alpha * np.exp(-(m / (maglim - gamma))**beta)
    p /= (np.diff(m) * (p[1:] + p[:-1]) / 2.0).sum()
    return np.interp(mag, m, p)


def _bpz_prior(m, zgrid, mbounds=(20, 32), zbounds=(0, 15), *args, **kwargs):
    """The BPZ prior at magnitude ``m`` on ``zgrid`` (priors.py:76-133): ``(p_i (Nz, 3), f_t (3,))``, p_i[:, t] being the redshift
    distribution of type t normalised to unit sum over the grid and scaled by the type fraction f_t.  ``m`` may be an array
    (K,): the results then gain a leading axis of length K."""
    m = np.asarray(m, dtype=np.float64)
    scalar = m.ndim == 0
    dm = (np.clip(m, mbounds[0], mbounds[1]) - mbounds[0]).reshape(-1, 1)               # (K, 1)
    zm_a = np.clip(_ZO + _KM * dm, zbounds[0], zbounds[1])**_A                          # (K, 3)
    z_a = np.asarray(zgrid, dtype=np.float64).reshape(-1, 1)**_A                        # (Nz, 3)
    f = np.zeros((len(dm), 3))
    f[:, :2] = _FO * np.exp(-_KT * dm)
    f[:, 2] = 1 - (f[:, 0] + f[:, 1] + 0.)
    p = z_a * np.exp(-np.clip(z_a / zm_a[:, None, :], 0., 700.))                        # (K, Nz, 3)
    p /= p.sum(axis=1, keepdims=True)
    p *= f[:, None, :]
    return (p[0], f[0]) if scalar else (p, f)


def _base_table(name):
    if name not in _base:
        p, f = _bpz_prior(_MGRID, _ZGRID)
        _base['pztm'], _base['ptm'] = np.ascontiguousarray(p), np.ascontiguousarray(f)
    return _base[name]


def _cells(grid, x, what):
    """cell and fraction of ``x`` on ``grid``; values outside it (a caller's bounds wider than the table) and nan are refused,
    as the reference's interpolator refuses them"""
    x = np.asarray(x, dtype=np.float64)
    if np.isnan(x).any() or (x < grid[0]).any() or (x > grid[-1]).any():
        raise ValueError("%s: a value is nan or out of bounds of the tabulated prior [%g, %g]" % (what, grid[0], grid[-1]))
    r, f = _pdf.lerp_cells(grid, x.ravel())
    return r.reshape(x.shape), f.reshape(x.shape)


def _check_t(t):
    t = np.asarray(t, dtype=np.float64)
    if ((t < 0) | (t > 2)).any():
        raise ValueError("t must be between 0 and 2 (inclusive).")
    return t


def _interp(values, coords, grids, names):
    """multilinear interpolation of ``values`` at the broadcast ``coords``: the sum over the cell's corners of the corner value
    times the product of its weights"""
    coords = np.broadcast_arrays(*coords)
    cells = [_cells(g, c, n) for g, c, n in zip(grids, coords, names)]
    out = 0.
    for corner in np.ndindex(*(2,) * len(grids)):
        w, idx = 1., []
        for up, (r, f) in zip(corner, cells):
            w = w * (f if up else 1 - f)
            idx.append(r + up)
        out = out + values[tuple(idx)] * w
    return out


def bpz_pt_m(t, m, mbounds=(20, 32), bpz_ptm_func=None, *args, **kwargs):
    """BPZ P(t | m) (priors.py:136-180); ``t`` and ``m`` broadcast.  ``m`` is clipped to ``mbounds``."""
    t = _check_t(t)
    m = np.clip(np.asarray(m, dtype=np.float64), mbounds[0], mbounds[1])
    if bpz_ptm_func is not None:
        return bpz_ptm_func((m, t))
    return _interp(_base_table('ptm'), (m, t), (_MGRID, _TGRID), ("m", "t"))


def bpz_pz_tm(z, t, m, mbounds=(20, 32), zbounds=(0, 15), bpz_pztm_func=None, *args, **kwargs):
    """BPZ P(z, t | m) on the tabulated grid (priors.py:183-235); ``z``, ``t`` and ``m`` broadcast.  ``m`` and ``z`` are clipped
    to ``mbounds`` / ``zbounds``; nan raises ``ValueError``."""
    t = _check_t(t)
    m = np.clip(np.asarray(m, dtype=np.float64), mbounds[0], mbounds[1])
    z = np.clip(np.asarray(z, dtype=np.float64), zbounds[0], zbounds[1])
    if bpz_pztm_func is not None:
        return bpz_pztm_func((m, z, t))
    return _interp(_base_table('pztm'), (m, z, t), (_MGRID, _ZGRID, _TGRID), ("m", "z", "t"))


def model_cells(model_z, model_type, zbounds=(0, 15)):
    """``(iz int32, g float64, t int32)`` of a model set on the tabulated redshift grid: what ``fz_prior_rows_from_grid`` reads"""
    t = np.asarray(model_type)
    if t.ndim != 1 or not np.all(np.isin(t, (0, 1, 2))):
        raise ValueError("`model_type` must be a 1-D array of the types 0, 1, 2")
    z = np.asarray(model_z, dtype=np.float64)
    if z.shape != t.shape:
        raise ValueError("`model_z` and `model_type` must have the same length")
    iz, g = _cells(_ZGRID, np.clip(z, zbounds[0], zbounds[1]), "model_z")
    return iz.astype(np.int32), g, t.astype(np.int32)


def logprob_bpz(model_z, model_type, mag, mbounds=(20, 32), zbounds=(0, 15), device=None):
    """The ``lprob_func`` of the BPZ posterior, lnprob = lnlike + ln P(z_j, t_j | m_i), for ``BruteForce`` /
    ``NearestNeighbors`` (the demo's ``lprob_bpz`` on the GPU).  ``model_z`` (M,) float and ``model_type`` (M,) int in {0, 1, 2}
    describe the model set, ``mag`` (Ndata,) is every object's reference-band magnitude (clipped to ``mbounds``; nan raises
    ``ValueError`` here, before any device work).  The likelihood options stay in ``lprob_kwargs`` (the demo uses
    ``free_scale=True, ignore_model_err=True``).

    The (1000, M) table of the prior at every tabulated magnitude is built on the device once and stays there: 8 kB per model."""
    iz, g, t = model_cells(model_z, model_type, zbounds)
    mag = np.asarray(mag, dtype=np.float64)
    if np.isnan(mag).any():
        raise ValueError("`mag` holds nan: the prior is undefined there")
    m = np.clip(mag, mbounds[0], mbounds[1])
    if (m < _MGRID[0]).any() or (m > _MGRID[-1]).any():
        raise ValueError("`mag`: a value is out of bounds of the tabulated prior [20, 32]")
    eng = get_engine(device)
    base = getattr(eng, "_bpz_base", None)
    if base is None:
        base = DeviceArray(eng, (len(_MGRID), len(_ZGRID), 3))
        base.set_rows(0, _base_table('pztm'))
        eng._bpz_base = base
    table = DeviceArray(eng, (len(_MGRID), len(iz)))
    eng.prior_rows_from_grid(base, iz, g, t, table)
    return _pdf.logprob_prior_lerp(table, _MGRID, m)
