"""G20: the reference's mock photometry (simulate.py, reddening.py) recorded for tests/test_simulate_host.py and
tests/test_hip_synphot.py.  Run from the repository root with the reference importable, or with FRANKENZ_REFERENCE naming its
checkout:

    FRANKENZ_REFERENCE=/path/to/frankenz python tests/golden/make_golden_synphot.py

Filters (5 curves picked from four of the reference's surveys): SDSS u (19 points, one wavelength repeated: a zero-width panel),
COSMOS galex_nuv (starts at 1687 A), LSST r (2201 points; the reference band), Euclid Jw (3305 points), SDSS i.
Templates (4): CWW+ ssp_25myr (6900 points, 91 A - 160 um), CWW+ El (1781 points), Polletta Sb_0 (starts at 316 A: the left end
of the interpolation is reached from z = 4.3 on), and CWW+ Sbc cut to 3000-9000 A BY HAND after loading (both ends are reached).
Recorded: make_model_grid on z = {0, 0.5, 2, 3.3, 6, 14.9} with and without the Madau attenuation (z = 14.9 gives results of +-0 and
values down to 5e-70 for these curves), the reddening functions on wavelengths that straddle every line (some exactly l (1 + z)), a seeded
sample_params(300) + sample_phot() under the BPZ prior with the state of the RandomState afterwards, draw_mag for one seed, and
the public signatures."""
import inspect
import json
import os
import sys
import warnings

import numpy as np

warnings.filterwarnings('ignore')
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
if os.environ.get('FRANKENZ_REFERENCE'):
    sys.path.insert(0, os.environ['FRANKENZ_REFERENCE'])
if not hasattr(np, 'trapz'):
    np.trapz = np.trapezoid

from frankenz import priors as rpriors, reddening as rred, simulate  # noqa: E402

ZGRID = np.array([0., 0.5, 2.0, 3.3, 6.0, 14.9])
FILTERS = (('sdss', 'u'), ('cosmos', 'galex_nuv'), ('lsst', 'r'), ('euclid', 'Jw'), ('sdss', 'i'))
TEMPLATES = (('cww+', 'ssp_25myr'), ('cww+', 'El'), ('polletta+', 'Sb_0'), ('cww+', 'Sbc'))
CUT = (3000., 9000.)


def raw_sed(tset, name):
    """the template's file as it is on disk: (wavelength, flambda) before the loader normalises it"""
    base = os.path.join(os.path.dirname(os.path.abspath(simulate.__file__)), 'seds') + '/'
    for line in open(base + simulate._TEMPLATES[tset]):
        index, nm, obj_type, fpath = line.split()
        if nm == name:
            return np.loadtxt(base + fpath).T
    raise KeyError(name)


def state_arrays(rs, tag, out):
    name, keys, pos, has_gauss, cached = rs.get_state()
    assert name == 'MT19937'
    out[tag + '_keys'], out[tag + '_pos'] = keys, np.array([pos, has_gauss], dtype=np.int64)
    out[tag + '_gauss'] = np.array(cached)


def main():
    out = {}
    # ---- the survey, put together by hand from the loaded presets -----------------------------------------------------
    loaded = {}
    for sv, _ in FILTERS:
        if sv not in loaded:
            loaded[sv] = simulate.MockSurvey()
            loaded[sv].load_survey(sv, Npoints=50000)
    ms = simulate.MockSurvey()
    ms.filters = []
    for sv, name in FILTERS:
        f = [f for f in loaded[sv].filters if f['name'] == name][0]
        ms.filters.append(dict(f))
    ms.NFILTER = len(ms.filters)
    ms.set_refmag('r')
    assert (np.diff(ms.filters[0]['wavelength']) == 0).sum() == 1 and ms.filters[1]['wavelength'].min() < 1700
    assert len(ms.filters[2]['wavelength']) > 2000 and len(ms.filters[3]['wavelength']) > 3000
    for i, f in enumerate(ms.filters):
        out['f%d_wave' % i], out['f%d_trans' % i] = f['wavelength'], f['transmission']
    out['f_names'] = np.array([f['name'] for f in ms.filters])
    out['f_depth'] = np.array([f['depth_mag5sig'] for f in ms.filters])
    out['f_depth_flux'] = np.array([f['depth_flux1sig'] for f in ms.filters])
    out['f_lambda_eff'] = np.array([f['lambda_eff'] for f in ms.filters])
    out['ref_filter'] = np.array(ms.ref_filter)

    tl = {}
    for ts, _ in TEMPLATES:
        if ts not in tl:
            tl[ts] = simulate.MockSurvey()
            tl[ts].load_templates(ts)
    ms.templates = []
    for i, (ts, name) in enumerate(TEMPLATES):
        t = dict([t for t in tl[ts].templates if t['name'] == name][0])
        rw, rf = raw_sed(ts, name)
        assert np.array_equal(rw, t['wavelength'])
        out['t%d_wave' % i], out['t%d_flambda_raw' % i] = rw, rf
        out['t%d_fnu' % i], out['t%d_flambda' % i] = t['fnu'].copy(), t['flambda'].copy()       # as loaded: normalised at 7000 A
        ms.templates.append(t)
    t = ms.templates[3]                                     # cut by hand, after the normalisation
    keep = (t['wavelength'] >= CUT[0]) & (t['wavelength'] <= CUT[1])
    for k in ('wavelength', 'frequency', 'flambda', 'fnu'):
        t[k] = t[k][keep]
    out['t3_keep'] = keep
    assert [len(t['wavelength']) for t in ms.templates[:3]] == [6900, 1781, 1761] and ms.templates[2]['wavelength'].min() < 317
    ms.NTEMPLATE = len(ms.templates)
    ttypes = [t['type'] for t in ms.templates]
    out['t_names'], out['t_types'] = np.array([t['name'] for t in ms.templates]), np.array(ttypes)
    _, idx, ms.TYPE_COUNTS = np.unique(ttypes, return_index=True, return_counts=True)
    ms.TYPES = np.array(ttypes)[np.sort(idx)]
    ms.NTYPE = len(ms.TYPES)
    ms.TTYPE = np.array([np.arange(ms.NTYPE)[t['type'] == ms.TYPES] for t in ms.templates], dtype='int').flatten()
    assert ms.NTYPE == 3
    out['TYPES'], out['TYPE_COUNTS'], out['TTYPE'] = ms.TYPES, ms.TYPE_COUNTS, ms.TTYPE

    # ---- model grids ------------------------------------------------------------------------------------------------------
    out['zgrid'] = ZGRID
    ms.make_model_grid(ZGRID, verbose=False)
    out['grid_madau'] = ms.models['data'].copy()
    ms.make_model_grid(ZGRID, red_fn=None, verbose=False)
    out['grid_none'] = ms.models['data'].copy()
    assert np.isfinite(out['grid_madau']).all() and np.array_equal(out['grid_madau'][0], out['grid_none'][0])
    tiny = np.abs(out['grid_madau'][out['grid_madau'] != 0]).min()
    assert (out['grid_madau'][-1] == 0).any() and tiny < 1e-60, tiny

    # ---- reddening -------------------------------------------------------------------------------------------------------
    lines = np.array([1216.0, 1026.0, 973.0, 950.0, 938.1, 931.0, 926.5, 923.4, 921.2, 919.6, 918.4, 912.0])
    out['red_z'] = np.array([0.5, 3.3])
    for i, z in enumerate(out['red_z']):
        edge = lines * (1 + z)
        wave = np.sort(np.concatenate([edge, edge * (1 - 1e-9), edge * (1 + 1e-9), np.nextafter(edge, 0), np.nextafter(edge, 1e9),
                                       np.linspace(400., 1300. * (1 + z), 150)]))
        out['red%d_wave' % i] = wave
        out['red%d_tau1' % i], out['red%d_tau2' % i] = rred._madau_tau1(wave, z), rred._madau_tau2(wave, z)
        out['red%d_teff' % i] = rred.madau_teff(wave, z)
        out['red%d_t1' % i] = rred._madau_t1(wave, z, 1026.0, 0.00177)

    # ---- a seeded mock -----------------------------------------------------------------------------------------------------
    ms.load_prior('bpz')
    rs = np.random.RandomState(20)
    ms.sample_params(300, rstate=rs, verbose=False)
    state_arrays(rs, 'params_state', out)
    for k in ('refmags', 'types', 'templates', 'redshifts'):
        out['mock_' + k] = ms.data[k].copy()                    # (refmags: before sample_phot marks the bad ones)
    ms.sample_phot(rstate=rs, verbose=False)
    state_arrays(rs, 'phot_state', out)
    out['mock_refmags_after'] = ms.data['refmags'].copy()
    for k in ('phot_true', 'phot_obs', 'phot_err'):
        out['mock_' + k] = ms.data[k].copy()
    nbad = int(np.isinf(ms.data['refmags']).sum())
    # the drawn redshifts reach 11.7: for two of the 300 objects the whole reference band lies below the Lyman limit, its flux
    # underflows to 0 and the reference marks the object bad (fluxes -inf, reference magnitude inf)
    assert nbad >= 1
    out['mock_nbad'] = np.array(nbad)
    print('objects the reference marks bad: %d; z max %.2f' % (nbad, ms.data['redshifts'].max()))

    out['draw_mag'] = simulate.draw_mag(500, rpriors.pmag, rstate=np.random.RandomState(7), pmag_kwargs={'maglim': 25.},
                                        mbounds=(10, 27), Npoints=400)

    # ---- the public surface ------------------------------------------------------------------------------------------------
    sig = {}
    fns = {n: getattr(simulate, n) for n in simulate.__all__ if n != 'MockSurvey'}
    fns.update({'MockSurvey.' + n: getattr(simulate.MockSurvey, n) for n in
                ('__init__', 'load_survey', 'load_templates', 'load_prior', 'set_refmag', 'sample_params', 'sample_phot',
                 'make_mock', 'make_model_grid')})
    fns.update({'reddening.' + n: getattr(rred, n) for n in rred.__all__})
    for n, fn in fns.items():
        ps = inspect.signature(fn).parameters
        sig[n] = [[p.name, None if p.default is p.empty else repr(p.default)] for p in ps.values()]
    out['signatures'] = np.array(json.dumps(sig))
    out['all_simulate'], out['all_reddening'] = np.array(simulate.__all__), np.array(rred.__all__)

    path = os.path.join(HERE, 'g20_synphot.npz')
    np.savez_compressed(path, **out)
    print('g20_synphot %8.1f KB' % (os.path.getsize(path) / 1024.))


if __name__ == '__main__':
    main()
