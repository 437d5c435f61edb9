"""
Mock photometry: the reference's ``frankenz/simulate.py`` (simulate.py:54-1021) with the per-(template, redshift) loop of
``MockSurvey.sample_phot`` / ``make_model_grid`` run on the GPU (``fz_synphot``; docs/simulate.md) and the per-object loops of
``sample_params`` vectorised on the host.

Names, positional order and defaults are the reference's.  Extensions:

* ``sample_phot``, ``make_mock`` and ``make_model_grid`` take the keyword ``device=None`` as the rest of the package does;
  ``device='cpu'`` asks for the vectorised NumPy path, which does the same arithmetic on the host.  A callable ``red_fn`` other
  than the preset is evaluated on the host as well (it is Python).
* ``MockSurvey.set_filters`` / ``set_templates`` take arrays where ``load_survey`` / ``load_templates`` read files.
* The reference's filter and SED files are not shipped: the presets (``'sdss'``, ``'cww+'``, ...) are looked up in the directory
  named by the environment variable ``FRANKENZ_DATA``, which must hold ``filters/`` and ``seds/``.
"""
import os
import sys
import warnings

import numpy as np

from . import priors
from . import reddening

__all__ = ["mag_err", "draw_mag", "draw_type_given_mag",
           "draw_redshift_given_type_mag", "draw_ztm", "MockSurvey"]

# filter lists, reference magnitudes and template lists of the presets (simulate.py:26-42)
_FILTERS = {'cosmos': 'COSMOS.list', 'euclid': 'Euclid.list', 'hsc': 'HSC.list', 'lsst': 'LSST.list', 'sdss': 'SDSS.list'}
_REFMAGS = {'cosmos': 'i+', 'euclid': 'VIS', 'hsc': 'i', 'lsst': 'r', 'sdss': 'r'}
_TEMPLATES = {'brown': 'BROWN.list', 'cww+': 'CWWSB4.list', 'polletta+': 'POLLETTASB.list'}
_PRIORS = {'bpz': (priors.pmag, priors.bpz_pt_m, priors.bpz_pz_tm)}
_IGM = {'madau+99': reddening.madau_teff}

c = 299792458.0  # speed of light in m/s

_trapz = getattr(np, 'trapezoid', None) or np.trapz
_HOST_CELLS = 1 << 21            # (pairs x filter points) evaluated at once on the host path


def mag_err(mag, maglim, sigdet=5., params=(4.56, 1., 1.)):
    """Magnitude error for the ``sigdet``-sigma limiting magnitude ``maglim`` after Rykoff et al. (2015), ``params`` being its
    ``(a, b, k)``.  (The reference's body reads names that are not defined, simulate.py:86-91; this is what it evidently means:
    docs/deviations.md.)"""
    a, b, k = params
    teff = np.exp(a + b * (maglim - 21.))
    F = 10**(-0.4 * (mag - 22.5))
    Flim = 10**(-0.4 * (maglim - 22.5))
    Fnoise = (Flim / sigdet)**2 * k * teff - Flim
    return 2.5 / np.log(10.) * np.sqrt((1. + Fnoise / F) / (F * k * teff))


def _mag_cdf(pmag, pmag_kwargs, mbounds, Npoints):
    if mbounds[0] >= mbounds[1]:
        raise ValueError("The values {0} in `mbounds` are incorrectly ordered.".format(mbounds))
    mgrid = np.linspace(mbounds[0], mbounds[1], Npoints)
    cdf_m = pmag(mgrid, **pmag_kwargs).cumsum()
    cdf_m = np.append(0, cdf_m) / cdf_m[-1]
    lpad = 1e-5 * (mbounds[1] - mbounds[0])
    return cdf_m, np.append(mgrid[0] - lpad, mgrid)


def draw_mag(Nobj, pmag, rstate=None, pmag_kwargs=None, mbounds=(10, 28), Npoints=1000):
    """``Nobj`` magnitudes from ``pmag`` truncated to ``mbounds``, by its inverse CDF on ``Npoints`` points (simulate.py:96-150);
    consumes ``rstate.rand(Nobj)``."""
    if rstate is None:
        rstate = np.random
    cdf_m, mgrid = _mag_cdf(pmag, pmag_kwargs or dict(), mbounds, Npoints)
    return np.interp(rstate.rand(Nobj), cdf_m, mgrid)


def draw_type_given_mag(p_type_given_mag, mags, Ntypes, rstate=None, ptm_kwargs=None):
    """Generator of one type per magnitude from ``p_type_given_mag(t, m)`` (simulate.py:153-200); one ``rstate.rand()`` each."""
    if ptm_kwargs is None:
        ptm_kwargs = dict()
    if rstate is None:
        rstate = np.random
    types = np.arange(-1, Ntypes)
    for m in mags:
        prob = np.array([p_type_given_mag(t, m, **ptm_kwargs) for t in range(Ntypes)])
        cdf = np.append(0., prob).cumsum()
        cdf /= cdf[-1]
        yield int(np.interp(rstate.rand(), cdf, types) + 1)


def _z_grids(zbounds, Npoints):
    if zbounds[0] >= zbounds[1]:
        raise ValueError("The values {0} in `zbounds` are incorrectly ordered.".format(zbounds))
    zgrid = np.linspace(zbounds[0], zbounds[1], Npoints)
    lpad = 1e-5 * (zbounds[1] - zbounds[0])
    return zgrid, np.append(zgrid[0] - lpad, zgrid)


def draw_redshift_given_type_mag(p_z_tm, types, mags, rstate=None, pztm_kwargs=None, zbounds=(0, 15), Npoints=1000):
    """Generator of one redshift per (type, magnitude) from ``p_z_tm(z=, t=, m=)`` by its inverse CDF on ``Npoints`` points
    (simulate.py:203-273); one ``rstate.rand()`` each."""
    if pztm_kwargs is None:
        pztm_kwargs = dict()
    if rstate is None:
        rstate = np.random
    zgrid, zgrid2 = _z_grids(zbounds, Npoints)
    for t, m in zip(types, mags):
        try:
            pdf_z = p_z_tm(z=zgrid, t=t, m=m, **pztm_kwargs)
        except Exception:
            pdf_z = np.array([p_z_tm(z=z, t=t, m=m, **pztm_kwargs) for z in zgrid])
        cdf_z = pdf_z.cumsum()
        cdf_z = np.append(0, cdf_z) / cdf_z[-1]
        yield max(0., np.interp(rstate.rand(), cdf_z, zgrid2))


def draw_ztm(pmag, p_tm, p_ztm, Nobj, pm_kwargs=None, ptm_kwargs=None, pztm_kwargs=None, mbounds=(10, 28), zbound=(0, 15),
             Npoints=1000):
    """``(mags, types, redshifts)`` of ``Nobj`` draws from P(z, t, m) (simulate.py:276-351).  ``p_tm(mag)`` returns the vector
    P(type | mag) over the types, as the reference's docstring has it (its body cannot run: docs/deviations.md)."""
    ptm_kwargs = ptm_kwargs or dict()
    mags = draw_mag(Nobj, pmag, pmag_kwargs=pm_kwargs, mbounds=mbounds, Npoints=Npoints)
    types = np.zeros(Nobj, dtype='int')
    for i, m in enumerate(mags):
        cdf = np.append(0., np.asarray(p_tm(m, **ptm_kwargs), dtype='float')).cumsum()
        cdf /= cdf[-1]
        types[i] = int(np.interp(np.random.rand(), cdf, np.arange(-1, len(cdf) - 1)) + 1)
    redshifts = np.zeros(Nobj, dtype='float')
    for i, z in enumerate(draw_redshift_given_type_mag(p_ztm, types, mags, pztm_kwargs=pztm_kwargs, zbounds=zbound,
                                                       Npoints=Npoints)):
        redshifts[i] = z
    return mags, types, redshifts


def _interp_rows(x, xp, fp):
    """``np.interp(x[i], xp[i], fp[i])`` for every row i, with np.interp's choices: the cell is the rightmost j with
    ``xp[i, j] <= x[i]``, a point on a node takes the node's value, the ends are clamped.  ``fp`` is (L,) or (n, L)."""
    n, L = xp.shape
    fp = np.broadcast_to(fp, xp.shape)
    j = (xp <= x[:, None]).sum(axis=1) - 1
    r = np.arange(n)
    jj = np.clip(j, 0, L - 2)
    x0, f0, x1, f1 = xp[r, jj], fp[r, jj], xp[r, jj + 1], fp[r, jj + 1]
    with np.errstate(all='ignore'):
        res = (f1 - f0) / (x1 - x0) * (x - x0) + f0
    res = np.where(x == x0, f0, res)
    res = np.where(j < 0, fp[:, 0], res)
    return np.where(j >= L - 1, fp[:, -1], res)


def _note(verbose, text):
    if verbose:
        sys.stderr.write(text)
        sys.stderr.flush()


def _data_dir(kind, listfile, preset):
    """the directory of the presets' data: $FRANKENZ_DATA/filters/ or $FRANKENZ_DATA/seds/"""
    root = os.environ.get('FRANKENZ_DATA')
    if not root or not os.path.isfile(os.path.join(root, kind, listfile)):
        raise IOError("the preset '{0}' needs the reference's data files, which this package does not ship: set the environment "
                      "variable FRANKENZ_DATA to a directory that holds filters/ and seds/ ({1} was not found under {2})"
                      .format(preset, os.path.join(kind, listfile), root if root else "an unset FRANKENZ_DATA"))
    return os.path.join(root, kind) + os.sep


# ---- the arithmetic of the photometry: tables, the host path, the device call --------------------------------------------------
class _Tables(object):
    """What ``fz_synphot_upload`` takes, formed from the filter and template dicts with the reference's roundings: ragged arrays
    with offsets.  Per filter point the wavelength ``exp(log(wavelength))`` (what the reference hands its reddening function),
    ``log(wavelength)``, the trapezoid weight over frequency divided by the filter's norm, and the z-independent parts of the
    Madau optical depth; per template point ``log(wavelength)`` and ``arcsinh(fnu)``."""

    def __init__(self, filters, templates):
        fw, flw, fwt, ftab, foff = [], [], [], [], [0]
        for f in filters:
            wl = np.asarray(f['wavelength'], dtype=np.float64)
            nu = np.asarray(f['frequency'], dtype=np.float64)
            tr = np.asarray(f['transmission'], dtype=np.float64)
            with np.errstate(all='ignore'):
                lw = np.log(wl)
                wave = np.exp(lw)
                w = np.zeros_like(nu)
                d = np.diff(nu)
                w[:-1] += d / 2
                w[1:] += d / 2
                wn = tr / nu * w                       # sums to np.trapz(tr / nu, nu): the reference's norm
                wn = wn / wn.sum()
                tab = np.concatenate([reddening.line_table(wave), reddening.continuum_table(wave)], axis=1)
            fw.append(wave); flw.append(lw); fwt.append(wn); ftab.append(tab); foff.append(foff[-1] + len(wl))
        tlw, tas, toff = [], [], [0]
        for t in templates:
            with np.errstate(all='ignore'):
                tlw.append(np.log(np.asarray(t['wavelength'], dtype=np.float64)))
            tas.append(np.arcsinh(np.asarray(t['fnu'], dtype=np.float64)))
            toff.append(toff[-1] + len(tlw[-1]))
        cat = lambda a, w=None: np.ascontiguousarray(np.concatenate(a) if a else np.zeros((0,) if w is None else (0, w)))
        self.foff, self.toff = np.array(foff, dtype=np.int64), np.array(toff, dtype=np.int64)
        self.fwave, self.flw, self.fwt, self.ftab = cat(fw), cat(flw), cat(fwt), cat(ftab, 18)
        self.tlw, self.tas = cat(tlw), cat(tas)
        self.Nf, self.Nt = len(filters), len(templates)

    def check(self):
        """the refusals of ``fz_synphot_upload``, for the host path"""
        for name, off, arr in (("filter", self.foff, self.flw), ("template", self.toff, self.tlw)):
            for i in range(len(off) - 1):
                a = arr[off[i]:off[i + 1]]
                if len(a) < 2:
                    raise ValueError("%s %d has %d points (at least 2 are needed)" % (name, i, len(a)))
                if not np.isfinite(a).all():
                    raise ValueError("%s %d: a wavelength is not positive and finite" % (name, i))
                if name == "template" and (np.diff(a) < 0).any():
                    raise ValueError("template %d: wavelengths decrease" % i)


def _check_pairs(tb, tmpl, z):
    bad = np.flatnonzero((tmpl < 0) | (tmpl >= tb.Nt))
    if len(bad):
        raise IndexError("pair %d asks for template %d of %d" % (bad[0], tmpl[bad[0]], tb.Nt))
    x = 1. + z
    bad = np.flatnonzero(~np.isfinite(x) | (x < 0))
    if len(bad):
        raise ValueError("pair %d: 1 + z = %g is negative or not finite" % (bad[0], x[bad[0]]))


def _teff_rows(tb, k0, k1, z):
    """exp(-tau) of the points [k0, k1) for every redshift in ``z``, from the tables (bit for bit ``_madau_tau1``; ``_madau_tau2`` to
    the rounding of the four powers of 1 + z)"""
    xem = 1. + z
    wave, tab = tb.fwave[k0:k1], tb.ftab[k0:k1]
    na = (wave[None, None, :] < (np.array(reddening._LINES)[:, None] * xem[None, :])[:, :, None]).sum(axis=0)
    tau = tab[np.arange(k1 - k0)[None, :], na]
    c3, c046, c15, c018, cm132, c168 = (tab[:, 12 + i][None, :] for i in range(6))
    e = lambda p: (xem**p)[:, None]
    with np.errstate(all='ignore'):
        tau2 = ((0.25 * c3 * (e(0.46) - c046)) + (9.4 * c15 * (e(0.18) - c018)) - (0.7 * c3 * (cm132 - e(-1.32))) -
                (0.023 * (e(1.68) - c168)))
    tau2 = np.where(wave[None, :] < (912.0 * xem)[:, None], tau2, 0.)
    tau2[tau2 < 0.] = 0.
    return np.exp(-(tau + tau2))


def _synphot_host(tb, tmpl, z, ln1pz, igm, red_fn=None):
    """The device's sum on the host: per template and filter, a chunk of pairs at a time.  ``red_fn``: a user's callable,
    called per (pair, filter) as the reference calls it."""
    tb.check()
    _check_pairs(tb, tmpl, z)
    out = np.empty((len(tmpl), tb.Nf))
    for t in np.unique(tmpl):
        idx = np.flatnonzero(tmpl == t)
        xp, fp = tb.tlw[tb.toff[t]:tb.toff[t + 1]], tb.tas[tb.toff[t]:tb.toff[t + 1]]
        for f in range(tb.Nf):
            k0, k1 = tb.foff[f], tb.foff[f + 1]
            lw, wt, wave = tb.flw[k0:k1], tb.fwt[k0:k1], tb.fwave[k0:k1]
            step = max(1, _HOST_CELLS // (k1 - k0))
            for lo in range(0, len(idx), step):
                ids = idx[lo:lo + step]
                x = lw[None, :] - ln1pz[ids, None]
                with np.errstate(all='ignore'):
                    term = wt[None, :] * np.sinh(np.interp(x.ravel(), xp, fp).reshape(x.shape))
                    if red_fn is not None:
                        term = term * np.array([red_fn(wave, zz) for zz in z[ids]])
                    elif igm and (wave.min() < 1216.0 * (1. + z[ids])).any():
                        term = term * _teff_rows(tb, k0, k1, z[ids])
                    out[ids, f] = term.sum(axis=1)
    return out


def _synphot(tb, tmpl, z, red_fn, device, out=None):
    """(Npair, Nf) photometry of the (template, redshift) pairs: one call into the engine, or the host path"""
    tmpl = np.ascontiguousarray(tmpl, dtype=np.int64)
    z = np.ascontiguousarray(z, dtype=np.float64)
    with np.errstate(all='ignore'):
        ln1pz = np.log(1 + z)
    if red_fn is None:
        igm, fn = 0, None
    elif isinstance(red_fn, str):
        if red_fn not in _IGM:
            raise ValueError("{0} does not appear to be a valid IGM preset.".format(red_fn))
        igm, fn = 1, None
    elif red_fn is reddening.madau_teff:
        igm, fn = 1, None
    elif callable(red_fn):
        igm, fn = 0, red_fn
    else:
        raise ValueError("`red_fn` must be None, a preset name or a callable")
    if fn is not None or (isinstance(device, str) and device == 'cpu'):
        res = _synphot_host(tb, tmpl, z, ln1pz, igm, fn)
        if out is not None:
            out[...] = res
            return out
        return res
    from .engine import get_engine
    eng = get_engine(device)
    eng.synphot_upload(tb)
    if out is None:
        out = np.empty((len(tmpl), tb.Nf))
    eng.synphot(tmpl, z, ln1pz, igm, out)
    return out


class MockSurvey(object):
    """A mock survey: filters, templates, a P(z, type, mag) prior, and the mock data and model grids made from them
    (simulate.py:354-1021).  ``survey``, ``templates`` and ``prior`` name presets; ``rstate`` is the default random state."""

    def __init__(self, survey=None, templates=None, prior=None, rstate=None):
        self.filters = None
        self.NFILTER = None
        self.ref_filter = None
        self.templates = None
        self.NTEMPLATE = None
        self.TYPES = None
        self.TYPE_COUNTS = None
        self.NTYPE = None
        self.TTYPE = None
        self.pm = None
        self.ptm = None
        self.pztm = None
        self.data = None
        self.models = None
        if survey is not None:
            if survey in _FILTERS:
                self.load_survey(survey)
                self.set_refmag(_REFMAGS[survey])
            else:
                raise ValueError("{0} does not appear to be valid survey preset.".format(survey))
        if templates is not None:
            if templates in _TEMPLATES:
                self.load_templates(templates)
            else:
                raise ValueError("{0} does not appear to be valid template preset.".format(templates))
        if prior is not None:
            if prior in _PRIORS:
                self.load_prior(prior)
            else:
                raise ValueError("{0} does not appear to be valid prior preset.".format(prior))
        self.rstate = np.random if rstate is None else rstate

    # -- filters -------------------------------------------------------------------------------------------------------------
    def _fill_filters(self, indices, names, wavelengths, transmissions, depths, Npoints):
        self.filters = []
        for index, name, wl, tr, fdepth_mag in zip(indices, names, wavelengths, transmissions, depths):
            fdepth_mag = float(fdepth_mag)
            wl, tr = np.array(wl, dtype=np.float64), np.array(tr, dtype=np.float64)
            if wl.ndim != 1 or wl.shape != tr.shape:
                raise ValueError("filter {0}: wavelength and transmission must be 1-D arrays of one length".format(name))
            fltr = {'index': int(index), 'name': name, 'depth_mag5sig': fdepth_mag,
                    'depth_flux1sig': 10**((fdepth_mag - 23.9) / -2.5) / 5.,          # noise [uJy]
                    'wavelength': wl, 'transmission': tr}
            with np.errstate(all='ignore'):
                fltr['frequency'] = c / (1e-10 * wl)
                # effective wavelength: the transmission-weighted mean of ln(wavelength) over ln(frequency) (simulate.py:498-509)
                nu = np.linspace(1.001 * c / (max(wl) * 1e-10), 0.999 * c / (min(wl) * 1e-10), Npoints)
                lnu, wave = np.log(nu), c / nu
                trans = np.interp(1e10 * wave, wl, tr)
                fltr['lambda_eff'] = np.exp(_trapz(trans * np.log(wave), lnu) / _trapz(trans, lnu)) * 1e10
            self.filters.append(fltr)
        self.NFILTER = len(self.filters)

    def set_filters(self, names, wavelengths, transmissions, depth_mag5sig, indices=None):
        """``load_survey`` from arrays: per filter a name, its wavelengths [A] and transmissions, and its 5-sigma depth [mag];
        ``indices`` default to 1, 2, ....  Fills ``filters`` and ``NFILTER`` as the file loader does."""
        if indices is None:
            indices = range(1, len(names) + 1)
        if not (len(names) == len(wavelengths) == len(transmissions) == len(depth_mag5sig) == len(list(indices))):
            raise ValueError("names, wavelengths, transmissions, depth_mag5sig and indices must have one length")
        self._fill_filters(indices, names, wavelengths, transmissions, depth_mag5sig, 50000)

    def load_survey(self, filter_list, path='', Npoints=5e4):
        """Read a filter list (lines of ``index name file depth_mag5sig``; the files hold two columns, wavelength [A] and
        transmission) from ``path``, or a preset's from ``$FRANKENZ_DATA/filters/``.  ``Npoints``: points of the effective
        wavelength's integral (taken as ``int(Npoints)``)."""
        if filter_list in _FILTERS:
            path = _data_dir('filters', _FILTERS[filter_list], filter_list)
            filter_list = _FILTERS[filter_list]
        rows = []
        with open(path + filter_list) as f:
            for line in f:
                if line.strip():
                    index, name, fpath, fdepth_mag = line.split()
                    rows.append((int(index), name, fpath, float(fdepth_mag)))
        curves = [np.loadtxt(path + r[2]).T for r in rows]
        self._fill_filters([r[0] for r in rows], [r[1] for r in rows], [cv[0] for cv in curves], [cv[1] for cv in curves],
                           [r[3] for r in rows], int(Npoints))

    # -- templates -----------------------------------------------------------------------------------------------------------
    def _fill_templates(self, indices, names, types, wavelengths, flambdas, wnorm):
        self.templates = []
        for index, name, obj_type, wl, fl in zip(indices, names, types, wavelengths, flambdas):
            wl, fl = np.array(wl, dtype=np.float64), np.array(fl, dtype=np.float64)
            if wl.ndim != 1 or wl.shape != fl.shape:
                raise ValueError("template {0}: wavelength and flambda must be 1-D arrays of one length".format(name))
            tmp = {'index': int(index), 'name': name, 'type': obj_type, 'wavelength': wl}
            with np.errstate(all='ignore'):
                tmp['frequency'] = c / (1e-10 * wl)
                tmp['flambda'] = fl
                tmp['fnu'] = (wl * 1e-10)**2 / c * (fl * 1e10)
                # normalised at the pivot wavelength
                tmp['flambda'] /= np.interp(wnorm, wl, tmp['flambda'])
                tmp['fnu'] /= np.interp(wnorm, wl, tmp['fnu'])
            self.templates.append(tmp)
        self.NTEMPLATE = len(self.templates)
        # groups of templates (simulate.py:554-564)
        ttypes = [t['type'] for t in self.templates]
        _, idx, self.TYPE_COUNTS = np.unique(ttypes, return_index=True, return_counts=True)
        self.TYPES = np.array(ttypes)[np.sort(idx)]
        if len(self.TYPES) == 1:                                # no types given: every template is its own
            self.TYPES = np.arange(self.NTEMPLATE).astype('str')
            self.TYPE_COUNTS = np.ones(self.NTEMPLATE)
        self.NTYPE = len(self.TYPES)
        self.TTYPE = np.array([np.arange(self.NTYPE)[t['type'] == self.TYPES] for t in self.templates], dtype='int').flatten()

    def set_templates(self, names, types, wavelengths, flambdas, wnorm=7000.):
        """``load_templates`` from arrays: per template a name, a type label, its wavelengths [A] and F_lambda; both flux
        densities are normalised at the pivot wavelength ``wnorm``.  Fills ``templates``, ``NTEMPLATE``, ``TYPES``,
        ``TYPE_COUNTS``, ``NTYPE`` and ``TTYPE`` as the file loader does."""
        if not (len(names) == len(types) == len(wavelengths) == len(flambdas)):
            raise ValueError("names, types, wavelengths and flambdas must have one length")
        self._fill_templates(range(1, len(names) + 1), names, types, wavelengths, flambdas, wnorm)

    def load_templates(self, template_list, path='', wnorm=7000.):
        """Read a template list (lines of ``index name type file``; the files hold two columns, wavelength [A] and F_lambda) from
        ``path``, or a preset's from ``$FRANKENZ_DATA/seds/``."""
        if template_list in _TEMPLATES:
            path = _data_dir('seds', _TEMPLATES[template_list], template_list)
            template_list = _TEMPLATES[template_list]
        rows = []
        with open(path + template_list) as f:
            for line in f:
                if line.strip():
                    index, name, obj_type, fpath = line.split()
                    rows.append((int(index), name, obj_type, fpath))
        seds = [np.loadtxt(path + r[3]).T for r in rows]
        self._fill_templates([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], [s[0] for s in seds],
                             [s[1] for s in seds], wnorm)

    # -- prior and reference band ----------------------------------------------------------------------------------------------
    def load_prior(self, prior):
        """A preset name, or the functions ``(p_m, p_tm, p_ztm)``; stored as ``pm``, ``ptm``, ``pztm``."""
        if isinstance(prior, str) and prior in _PRIORS:
            self.pm, self.ptm, self.pztm = _PRIORS[prior]
        else:
            self.pm, self.ptm, self.pztm = prior

    def set_refmag(self, ref, mode='name'):
        """The filter of the magnitude prior, by ``'name'``, ``'index'`` (of the list file) or ``'counter'`` (position); stored
        as ``ref_filter``."""
        if mode not in {'name', 'index', 'counter'}:
            raise ValueError("{0} is not an allowed category.".format(mode))
        if mode == 'counter':
            self.ref_filter = ref
        else:
            sel = np.array([fltr[mode] == ref for fltr in self.filters], dtype=bool)
            if not sel.any():
                raise ValueError("{0} does not match any {1} among the filters.".format(ref, mode))
            self.ref_filter = np.arange(self.NFILTER)[sel][0]

    # -- parameters ------------------------------------------------------------------------------------------------------------
    def sample_params(self, Nobj, rstate=None, mbounds=None, zbounds=(0, 15), Nm=1000, Nz=1000, pm_kwargs=None, ptm_kwargs=None,
                      pztm_kwargs=None, verbose=True):
        """``Nobj`` draws of (magnitude, type, template, redshift) from the prior into ``data`` (simulate.py:630-761).  The random
        stream is consumed as the reference consumes it: ``rand(Nobj)`` for the magnitudes, ``Nobj`` uniforms for the types, one
        ``choice`` per type for the templates, ``Nobj`` uniforms for the redshifts.  With the BPZ preset the per-object CDFs are
        formed in chunks from the vectorised ``priors.bpz_pt_m`` / ``priors.bpz_pz_tm``; other callables are looped."""
        pm_kwargs = dict(pm_kwargs or {})
        ptm_kwargs = dict(ptm_kwargs or {})
        pztm_kwargs = dict(pztm_kwargs or {})
        if rstate is None:
            rstate = self.rstate
        pm_kwargs['maglim'] = pm_kwargs.get('maglim', self.filters[self.ref_filter]['depth_mag5sig'])
        if mbounds is None:
            mbounds = (10, pm_kwargs['maglim'] + 2.5 * np.log10(5))

        _note(verbose, 'Sampling mags: ')
        mags = draw_mag(Nobj, self.pm, pmag_kwargs=pm_kwargs, rstate=rstate, mbounds=mbounds, Npoints=Nm)
        _note(verbose, '{0}/{0}\nSampling types: '.format(Nobj))
        types = np.zeros(Nobj, dtype='int')
        if self.ptm is priors.bpz_pt_m:
            u = rstate.rand(Nobj)
            for lo in range(0, Nobj, 1 << 16):
                m = mags[lo:lo + (1 << 16)]
                prob = priors.bpz_pt_m(np.arange(self.NTYPE)[None, :], m[:, None], **ptm_kwargs)
                cdf = np.concatenate([np.zeros((len(m), 1)), prob], axis=1).cumsum(axis=1)
                cdf /= cdf[:, -1:]
                types[lo:lo + len(m)] = (_interp_rows(u[lo:lo + len(m)], cdf, np.arange(-1., self.NTYPE)) + 1).astype('int')
        else:
            for i, t in enumerate(draw_type_given_mag(self.ptm, mags, self.NTYPE, ptm_kwargs=ptm_kwargs, rstate=rstate)):
                types[i] = t
        _note(verbose, '{0}/{0}\nSampling templates within each type: '.format(Nobj))

        # templates of a type are equally likely
        tmp_types = np.array([tmp['type'] for tmp in self.templates])
        templates = np.empty(Nobj, dtype='int')
        for i, t in enumerate(self.TYPES):
            p = np.array(t == tmp_types, dtype='float') / sum(t == tmp_types)
            sel = types == i
            templates[sel] = rstate.choice(self.NTEMPLATE, size=int(sel.sum()), p=p)
        _note(verbose, '{0}/{0}\nSampling redshifts: '.format(self.NTYPE))

        redshifts = np.zeros(Nobj, dtype='float')
        if self.pztm is priors.bpz_pz_tm:
            zgrid, zgrid2 = _z_grids(zbounds, Nz)
            u = rstate.rand(Nobj)
            step = max(1, (1 << 21) // Nz)
            for lo in range(0, Nobj, step):
                sl = slice(lo, min(Nobj, lo + step))
                pdf_z = priors.bpz_pz_tm(zgrid[None, :], types[sl, None], mags[sl, None], **pztm_kwargs)
                cdf_z = pdf_z.cumsum(axis=1)
                cdf_z = np.concatenate([np.zeros((len(cdf_z), 1)), cdf_z], axis=1) / cdf_z[:, -1:]
                redshifts[sl] = np.maximum(0., _interp_rows(u[sl], cdf_z, zgrid2))
        else:
            for i, z in enumerate(draw_redshift_given_type_mag(self.pztm, types, mags, pztm_kwargs=pztm_kwargs, zbounds=zbounds,
                                                               Npoints=Nz, rstate=rstate)):
                redshifts[i] = z
        _note(verbose, '{0}/{0}\n'.format(Nobj))

        self.data = {'refmags': mags, 'types': types, 'templates': templates, 'redshifts': redshifts}
        self.NOBJ = Nobj

    # -- photometry ------------------------------------------------------------------------------------------------------------
    def sample_phot(self, red_fn='madau+99', rnoise_fn=None, rstate=None, verbose=True, *, device=None):
        """Noisy photometry of the sampled ``(t, z, m)`` into ``data`` (simulate.py:763-878; no Poisson noise).  ``red_fn``: the IGM
        preset ``'madau+99'``, None for no attenuation, or a callable ``red_fn(wave, z)`` (evaluated on the host); ``rnoise_fn``
        jitters the per-band noise (on the host)."""
        if rstate is None:
            rstate = self.rstate
        try:
            mags = self.data['refmags']
            templates = self.data['templates']
            redshifts = self.data['redshifts']
        except Exception:
            raise ValueError("No mock data has been generated.")
        nobj = len(mags)
        _note(verbose, 'Generating photometry: ')
        phot = _synphot(_Tables(self.filters, self.templates), templates, redshifts, red_fn, device)
        _note(verbose, '{0}/{0}\n'.format(nobj))

        # normalised to the reference magnitude
        with warnings.catch_warnings(), np.errstate(all='ignore'):
            warnings.simplefilter('ignore')
            fluxes = 10**((mags - 23.9) / -2.5)
            phot /= phot[:, self.ref_filter][:, None]
            phot *= fluxes[:, None]

        # photometry that makes no sense
        sel_badphot = np.unique(np.nonzero(~np.isfinite(phot))[0])
        self.data['refmags'][sel_badphot] = np.inf
        phot[sel_badphot] = -np.inf

        fnoise = np.array([np.ones(nobj) * f['depth_flux1sig'] for f in self.filters]).T
        if rnoise_fn is not None:
            fnoise = rnoise_fn(fnoise, rstate=rstate)
        _note(verbose, 'Sampling photometry: ')
        phot_obs = rstate.normal(phot, fnoise)
        _note(verbose, '{0}/{0}\n'.format(nobj))

        self.data['phot_true'] = phot
        self.data['phot_obs'] = phot_obs
        self.data['phot_err'] = fnoise

    def make_mock(self, Nobj, mbounds=None, zbounds=(0, 15), Nm=1000, Nz=1000, pm_kwargs=None, ptm_kwargs=None,
                  pztm_kwargs=None, red_fn='madau+99', rnoise_fn=None, rstate=None, verbose=True, *, device=None):
        """``sample_params`` followed by ``sample_phot`` (simulate.py:880-952)."""
        self.sample_params(Nobj, mbounds=mbounds, zbounds=zbounds, Nm=Nm, Nz=Nz, pm_kwargs=pm_kwargs, rstate=rstate,
                           ptm_kwargs=ptm_kwargs, pztm_kwargs=pztm_kwargs, verbose=verbose)
        self.sample_phot(red_fn=red_fn, rnoise_fn=rnoise_fn, rstate=rstate, verbose=verbose, device=device)

    def make_model_grid(self, redshifts, red_fn='madau+99', verbose=True, *, device=None):
        """Photometry of every template at every redshift of ``redshifts`` into ``models``: ``data`` of shape (Nz, Nt, Nf) and
        ``zgrid`` (simulate.py:954-1021)."""
        Nz = len(redshifts)
        z = np.repeat(np.asarray(redshifts, dtype=np.float64), self.NTEMPLATE)
        tmpl = np.tile(np.arange(self.NTEMPLATE), Nz)
        _note(verbose, 'Generating model photometry grid: ')
        phot = _synphot(_Tables(self.filters, self.templates), tmpl, z, red_fn, device)
        _note(verbose, '{0}/{0}\n'.format(Nz))
        self.models = {'data': phot.reshape(Nz, self.NTEMPLATE, self.NFILTER), 'zgrid': redshifts}
