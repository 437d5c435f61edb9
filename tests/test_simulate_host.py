"""frankenz_amd.simulate / frankenz_amd.reddening on the host (no GPU): against the reference's recorded results (golden G20) and
the reference's stream of random numbers.

Tolerances: the reddening functions are the reference's NumPy expressions (rtol 1e-15 should a power differ in its last bit); the
photometry is held to the project's bar, rtol 1e-12 against the reference with atol 1e-250 for the underflowing z = 14.9 entries
(docs/simulate.md derives why that is enough)."""
import inspect
import json
import os

import numpy as np
import pytest

import _synphot_case as case

RTOL, ATOL = 1e-12, 1e-250


@pytest.fixture(scope='module')
def g():
    return case.g20()


@pytest.fixture(scope='module')
def survey():
    return case.cut_last_template(case.golden_survey())


def test_reddening_values(g):
    from frankenz_amd import reddening
    for i, z in enumerate(g['red_z']):
        wave = g['red%d_wave' % i]
        np.testing.assert_allclose(reddening._madau_t1(wave, z, 1026.0, 0.00177), g['red%d_t1' % i], rtol=1e-15, atol=0)
        np.testing.assert_allclose(reddening._madau_tau1(wave, z), g['red%d_tau1' % i], rtol=1e-15, atol=0)
        np.testing.assert_allclose(reddening._madau_tau2(wave, z), g['red%d_tau2' % i], rtol=1e-15, atol=0)
        np.testing.assert_allclose(reddening.madau_teff(wave, z), g['red%d_teff' % i], rtol=1e-15, atol=0)
        # the strict selections: a wavelength exactly l (1 + z) is not attenuated by that line, the one just below is
        assert np.array_equal(reddening._madau_t1(wave, z, 1026.0, 0.00177) == 0, g['red%d_t1' % i] == 0)
        assert np.array_equal(reddening._madau_tau2(wave, z) == 0, g['red%d_tau2' % i] == 0)
        edge = 1026.0 * (1 + z)
        assert reddening._madau_t1(np.array([edge]), z, 1026.0, 0.00177)[0] == 0
        assert reddening._madau_t1(np.array([np.nextafter(edge, 0)]), z, 1026.0, 0.00177)[0] > 0
        assert (reddening._madau_tau2(wave, z) >= 0).all()
        # the device's tables restate tau1 bit for bit
        tab = reddening.line_table(wave)
        na = (wave[None, :] < (np.array(reddening._LINES) * (1 + z))[:, None]).sum(axis=0)
        assert np.array_equal(tab[np.arange(len(wave)), na], reddening._madau_tau1(wave, z))


def test_array_loaders_fill_the_recorded_fields(g):
    ms = case.golden_survey()
    assert ms.NFILTER == 5 and ms.NTEMPLATE == 4 and ms.ref_filter == int(g['ref_filter'])
    for i, f in enumerate(ms.filters):
        assert sorted(f) == sorted(['index', 'name', 'depth_mag5sig', 'depth_flux1sig', 'wavelength', 'transmission', 'frequency',
                                    'lambda_eff'])
        assert f['index'] == i + 1 and f['name'] == str(g['f_names'][i])
        np.testing.assert_allclose(f['lambda_eff'], g['f_lambda_eff'][i], rtol=1e-13)
        np.testing.assert_allclose(f['depth_flux1sig'], g['f_depth_flux'][i], rtol=1e-15)
        assert np.array_equal(f['frequency'], 299792458.0 / (1e-10 * g['f%d_wave' % i]))
    for i, t in enumerate(ms.templates):
        assert sorted(t) == sorted(['index', 'name', 'type', 'wavelength', 'frequency', 'flambda', 'fnu'])
        np.testing.assert_allclose(t['fnu'], g['t%d_fnu' % i], rtol=1e-15, atol=0)
        np.testing.assert_allclose(t['flambda'], g['t%d_flambda' % i], rtol=1e-15, atol=0)
    assert list(ms.TYPES) == list(g['TYPES']) and list(ms.TYPE_COUNTS) == list(g['TYPE_COUNTS']) and list(ms.TTYPE) == list(g['TTYPE'])
    assert ms.NTYPE == 3
    # the caller's arrays are not normalised in place
    raw = g['t1_flambda_raw'].copy()
    ms.set_templates(['a', 'b'], ['x', 'x'], [g['t1_wave'], g['t1_wave']], [raw, raw])
    assert np.array_equal(raw, g['t1_flambda_raw'])
    assert list(ms.TYPES) == ['0', '1'] and ms.NTYPE == 2 and list(ms.TTYPE) == []          # one type: as the reference relabels


@pytest.mark.parametrize('red,key', [('madau+99', 'grid_madau'), (None, 'grid_none')])
def test_host_model_grid_against_the_reference(g, survey, red, key):
    survey.make_model_grid(g['zgrid'], red_fn=red, verbose=False, device='cpu')
    got, want = survey.models['data'], g[key]
    assert got.shape == want.shape == (6, 4, 5) and np.array_equal(survey.models['zgrid'], g['zgrid'])
    dev = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
    print('host %s: worst relative deviation %.3e at (z, t, f) %s' % (key, dev.max(), np.unravel_index(dev.argmax(), dev.shape)))
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)
    assert np.array_equal(got == 0, want == 0)


def test_host_model_grid_with_a_callable_red_fn(g, survey):
    from frankenz_amd import reddening
    calls = []

    def red(wave, z):
        calls.append(z)
        return reddening.madau_teff(wave, z)
    survey.make_model_grid(g['zgrid'][2:4], red_fn=red, verbose=False)         # a callable takes the host path: no device needed
    assert len(calls) == 2 * 4 * 5
    np.testing.assert_allclose(survey.models['data'], g['grid_madau'][2:4], rtol=RTOL, atol=ATOL)
    with pytest.raises(ValueError, match='IGM preset'):
        survey.make_model_grid(g['zgrid'], red_fn='nope', verbose=False, device='cpu')


def test_sample_params_consumes_the_stream_as_the_reference(g, survey):
    survey.load_prior('bpz')
    rs = np.random.RandomState(20)
    survey.sample_params(300, rstate=rs, verbose=False)
    d = survey.data
    assert sorted(d) == ['redshifts', 'refmags', 'templates', 'types'] and survey.NOBJ == 300
    assert np.array_equal(d['refmags'], g['mock_refmags'])
    assert np.array_equal(d['types'], g['mock_types']) and d['types'].dtype == g['mock_types'].dtype
    assert np.array_equal(d['templates'], g['mock_templates'])
    np.testing.assert_allclose(d['redshifts'], g['mock_redshifts'], rtol=1e-10, atol=1e-12)
    assert case.same_state(rs, g, 'params_state')


def test_sample_params_loops_other_priors(g, survey):
    """a prior that is not the preset is called per object, as the reference calls it, and consumes the same stream"""
    from frankenz_amd import priors
    calls = {'t': 0, 'z': 0}

    def ptm(t, m, **kw):
        calls['t'] += 1
        return priors.bpz_pt_m(t, m, **kw)

    def pztm(z=None, t=None, m=None, **kw):
        calls['z'] += 1
        return priors.bpz_pz_tm(z, t, m, **kw)
    survey.load_prior((priors.pmag, ptm, pztm))
    rs = np.random.RandomState(20)
    survey.sample_params(40, rstate=rs, verbose=False)
    assert calls == {'t': 40 * 3, 'z': 40}
    loop = dict(survey.data)
    survey.load_prior('bpz')
    survey.sample_params(40, rstate=np.random.RandomState(20), verbose=False)
    for k in ('refmags', 'types', 'templates'):
        assert np.array_equal(loop[k], survey.data[k]), k
    np.testing.assert_allclose(loop['redshifts'], survey.data['redshifts'], rtol=1e-10, atol=1e-12)


def test_host_sample_phot_against_the_reference(g, survey):
    survey.load_prior('bpz')
    survey.data = {k: g['mock_' + k].copy() for k in ('refmags', 'types', 'templates', 'redshifts')}
    survey.NOBJ = 300
    rs = case.restore_state(g, 'params_state')
    survey.sample_phot(rstate=rs, verbose=False, device='cpu')
    d = survey.data
    assert sorted(d) == ['phot_err', 'phot_obs', 'phot_true', 'redshifts', 'refmags', 'templates', 'types']
    bad = np.isinf(g['mock_refmags_after'])
    assert bad.sum() == int(g['mock_nbad']) >= 1
    assert np.array_equal(np.isinf(d['refmags']), bad) and np.array_equal(d['refmags'][~bad], g['mock_refmags'][~bad])
    assert np.isneginf(d['phot_true'][bad]).all() and np.isfinite(d['phot_true'][~bad]).all()
    np.testing.assert_allclose(d['phot_true'][~bad], g['mock_phot_true'][~bad], rtol=RTOL, atol=ATOL)
    assert np.array_equal(d['phot_err'], g['mock_phot_err'])
    # the noise is drawn on the host in the reference's order: the same normals around fluxes equal to 1e-12
    sig = g['mock_phot_err'][~bad]
    np.testing.assert_allclose(d['phot_obs'][~bad], g['mock_phot_obs'][~bad], rtol=1e-9, atol=1e-12 * sig.max())
    assert np.isneginf(d['phot_obs'][bad]).all()
    assert case.same_state(rs, g, 'phot_state')
    with pytest.raises(ValueError, match='No mock data'):
        s2 = case.golden_survey()
        s2.sample_phot(verbose=False, device='cpu')


def test_bad_photometry_rule(survey):
    """an object whose reference band lies wholly below the Lyman limit has a reference flux of 0: every band becomes -inf and its
    magnitude inf; its neighbours are untouched"""
    survey.data = {'refmags': np.array([24., 25., 26.]), 'types': np.array([0, 1, 2]), 'templates': np.array([0, 1, 2]),
                   'redshifts': np.array([0.7, 14.9, 1.1])}
    survey.NOBJ = 3
    survey.sample_phot(rstate=np.random.RandomState(1), verbose=False, device='cpu')
    d = survey.data
    assert np.array_equal(d['refmags'], [24., np.inf, 26.])
    assert np.isneginf(d['phot_true'][1]).all() and np.isneginf(d['phot_obs'][1]).all()
    assert np.isfinite(d['phot_true'][[0, 2]]).all() and np.isfinite(d['phot_obs'][[0, 2]]).all()
    ref = survey.ref_filter
    np.testing.assert_allclose(d['phot_true'][[0, 2], ref], 10**((np.array([24., 26.]) - 23.9) / -2.5), rtol=1e-14)
    # rnoise_fn is handed the per-band noise and the random state
    seen = {}

    def rnoise(fnoise, rstate=None):
        seen['shape'], seen['rs'] = fnoise.shape, rstate
        return 2 * fnoise
    rs = np.random.RandomState(2)
    survey.data['refmags'], survey.data['redshifts'] = np.array([24., 25., 26.]), np.array([0.7, 2.0, 1.1])
    survey.sample_phot(red_fn=None, rnoise_fn=rnoise, rstate=rs, verbose=False, device='cpu')
    assert seen == {'shape': (3, 5), 'rs': rs} and np.isfinite(survey.data['phot_true']).all()
    np.testing.assert_allclose(survey.data['phot_err'][0], 2 * np.array([f['depth_flux1sig'] for f in survey.filters]))


def test_file_loaders_round_trip(tmp_path, g):
    from frankenz_amd import simulate
    d = str(tmp_path) + os.sep
    os.mkdir(d + 'curves')
    fl, tl = [], []
    for i in (0, 1):
        np.savetxt(d + 'curves/f%d.res' % i, np.c_[g['f%d_wave' % i], g['f%d_trans' % i]], fmt='%.17g')
        fl.append('%d %s curves/f%d.res %r' % (i + 7, g['f_names'][i], i, float(g['f_depth'][i])))
    for i in (1, 2):
        np.savetxt(d + 'curves/t%d.sed' % i, np.c_[g['t%d_wave' % i], g['t%d_flambda_raw' % i]], fmt='%.17g')
        tl.append('%d %s %s curves/t%d.sed' % (i, g['t_names'][i], g['t_types'][i], i))
    open(d + 'my.list', 'w').write('\n'.join(fl) + '\n')
    open(d + 'my_seds.list', 'w').write('\n'.join(tl) + '\n')
    ms = simulate.MockSurvey()
    ms.load_survey('my.list', path=d, Npoints=5e4)                  # the reference's float default is taken as an int
    ms.load_templates('my_seds.list', path=d)
    ms.set_refmag(8, mode='index')
    assert ms.ref_filter == 1 and ms.NFILTER == 2 and ms.NTEMPLATE == 2
    with pytest.raises(ValueError, match='does not match'):
        ms.set_refmag('nope')
    with pytest.raises(ValueError, match='allowed category'):
        ms.set_refmag('u', mode='colour')
    for k, i in enumerate((0, 1)):
        f = ms.filters[k]
        assert f['index'] == i + 7 and f['name'] == str(g['f_names'][i]) and f['depth_mag5sig'] == g['f_depth'][i]
        assert np.array_equal(f['wavelength'], g['f%d_wave' % i]) and np.array_equal(f['transmission'], g['f%d_trans' % i])
        np.testing.assert_allclose(f['lambda_eff'], g['f_lambda_eff'][i], rtol=1e-13)
    for k, i in enumerate((1, 2)):
        np.testing.assert_allclose(ms.templates[k]['fnu'], g['t%d_fnu' % i], rtol=1e-15)
        assert ms.templates[k]['type'] == str(g['t_types'][i])
    assert list(ms.TYPES) == ['PGAL', 'SGAL'] and list(ms.TTYPE) == [0, 1]


def test_presets_without_data_say_what_is_missing(monkeypatch, tmp_path):
    from frankenz_amd import simulate
    monkeypatch.delenv('FRANKENZ_DATA', raising=False)
    with pytest.raises(IOError, match=r"FRANKENZ_DATA.*filters/ and seds/"):
        simulate.MockSurvey(survey='sdss')
    monkeypatch.setenv('FRANKENZ_DATA', str(tmp_path))
    with pytest.raises(IOError, match=r"does not ship.*FRANKENZ_DATA.*filters/ and seds/.*CWWSB4.list"):
        simulate.MockSurvey(templates='cww+')
    for kw in (dict(survey='nope'), dict(templates='nope'), dict(prior='nope')):
        with pytest.raises(ValueError, match='does not appear to be valid'):
            simulate.MockSurvey(**kw)
    ms = simulate.MockSurvey(prior='bpz')
    from frankenz_amd import priors
    assert (ms.pm, ms.ptm, ms.pztm) == (priors.pmag, priors.bpz_pt_m, priors.bpz_pz_tm) and ms.rstate is np.random


def test_modules_are_exported_with_the_reference_signatures(g):
    import frankenz_amd
    from frankenz_amd import reddening, simulate
    assert frankenz_amd.simulate is simulate and frankenz_amd.reddening is reddening
    assert 'simulate' in frankenz_amd.__all__ and 'reddening' in frankenz_amd.__all__
    assert simulate.__all__ == list(g['all_simulate']) and reddening.__all__ == list(g['all_reddening'])
    sig = json.loads(str(g['signatures']))
    assert len(sig) == 5 + 9 + 4
    for name, want in sig.items():
        if name.startswith('MockSurvey.'):
            fn = getattr(simulate.MockSurvey, name.split('.')[1])
        elif name.startswith('reddening.'):
            fn = getattr(reddening, name.split('.')[1])
        else:
            fn = getattr(simulate, name)
        ps = inspect.signature(fn).parameters
        pos = [p for p in ps.values() if p.kind == p.POSITIONAL_OR_KEYWORD]
        assert [p.name for p in pos] == [w[0] for w in want], name
        for p, (_, default) in zip(pos, want):
            assert (None if p.default is p.empty else repr(p.default)) == default, (name, p.name)
        extra = [p.name for p in ps.values() if p.kind == p.KEYWORD_ONLY]
        assert extra == (['device'] if name in ('MockSurvey.sample_phot', 'MockSurvey.make_mock', 'MockSurvey.make_model_grid') else []), name


def test_draw_mag_and_mag_err(g):
    from frankenz_amd import priors, simulate
    got = simulate.draw_mag(500, priors.pmag, rstate=np.random.RandomState(7), pmag_kwargs={'maglim': 25.}, mbounds=(10, 27),
                            Npoints=400)
    np.testing.assert_allclose(got, g['draw_mag'], rtol=1e-13)
    with pytest.raises(ValueError, match='incorrectly ordered'):
        simulate.draw_mag(5, priors.pmag, pmag_kwargs={'maglim': 25.}, mbounds=(28, 10))
    mag = np.linspace(18., 26., 30)
    err = simulate.mag_err(mag, 25.)
    assert np.isfinite(err).all() and (err > 0).all() and (np.diff(err) > 0).all()          # brighter: smaller error
    assert simulate.mag_err(25., 25.) == pytest.approx(2.5 / np.log(10.) / 5., rel=1e-12)    # the 5-sigma limit is 5 sigma
    assert np.isfinite(simulate.mag_err(22., 25., sigdet=10., params=(4.0, 1.2, 0.9)))


def test_draw_generators_and_draw_ztm():
    from frankenz_amd import priors, simulate
    rs = np.random.RandomState(3)
    mags = np.array([21., 23.5, 26.])
    types = list(simulate.draw_type_given_mag(priors.bpz_pt_m, mags, 3, rstate=rs))
    assert len(types) == 3 and all(isinstance(t, int) and 0 <= t < 3 for t in types)
    zs = list(simulate.draw_redshift_given_type_mag(priors.bpz_pz_tm, types, mags, rstate=rs))
    assert len(zs) == 3 and all(0. <= z <= 15. for z in zs)
    with pytest.raises(ValueError, match='incorrectly ordered'):
        list(simulate.draw_redshift_given_type_mag(priors.bpz_pz_tm, types, mags, zbounds=(3, 1)))
    m, t, z = simulate.draw_ztm(priors.pmag, lambda m: priors.bpz_pt_m(np.arange(3), m), priors.bpz_pz_tm, 20,
                                pm_kwargs={'maglim': 25.})
    assert m.shape == t.shape == z.shape == (20,) and ((t >= 0) & (t < 3)).all() and ((z >= 0) & (z <= 15)).all()


def test_host_path_refusals():
    from frankenz_amd import simulate
    ms = case.synthetic_survey([16, 9], [40, 30])
    tb = simulate._Tables(ms.filters, ms.templates)
    z = np.array([0.5, 1.0])
    with pytest.raises(IndexError, match='template 2 of 2'):
        simulate._synphot(tb, [0, 2], z, None, 'cpu')
    with pytest.raises(IndexError):
        simulate._synphot(tb, [-1, 0], z, None, 'cpu')
    for bad in (-1.5, np.nan, np.inf):
        with pytest.raises(ValueError, match='negative or not finite'):
            simulate._synphot(tb, [0, 1], np.array([0.5, bad]), None, 'cpu')
    for what, edit, msg in (('templates', lambda t: t.update(wavelength=t['wavelength'][:1], fnu=t['fnu'][:1]), 'at least 2'),
                            ('templates', lambda t: t['wavelength'].__setitem__(3, 0.), 'not positive'),
                            ('templates', lambda t: t['wavelength'].__setitem__(5, t['wavelength'][3]), 'decrease'),
                            ('filters', lambda f: f.update(wavelength=f['wavelength'][:1], frequency=f['frequency'][:1],
                                                           transmission=f['transmission'][:1]), 'at least 2'),
                            ('filters', lambda f: f['wavelength'].__setitem__(2, -1.), 'not positive')):
        ms = case.synthetic_survey([16, 9], [40, 30])
        edit(getattr(ms, what)[1])
        with pytest.raises(ValueError, match=msg):
            ms.make_model_grid([0.5], verbose=False, device='cpu')
