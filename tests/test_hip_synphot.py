"""GPU parity of frankenz_amd.simulate (fz_synphot_upload, fz_synphot): against the reference's recorded results (golden G20) and, at
shapes the fixture does not hold, against the package's NumPy host path.

Tolerance (docs/simulate.md): rtol 1e-12 against the reference, the project's bar, with atol 1e-250 for the underflowing z = 14.9
entries.  The weighted-sum restatement of the reference's trapezoid costs < 1e-15; the device's pow / exp / sinh are within a few
ulp; the relative error of exp(-tau) is the absolute error of tau, and tau stays below ~750 before the result underflows: about
750 x a few x 1.1e-16 ~ 3e-13 for the most attenuated normal values and ~1e-15 otherwise.  The host path does the same arithmetic
with other roundings (NumPy's pairwise sums, the host's libm), so the same bar holds between the two."""
import ctypes as C

import numpy as np
import pytest

import _synphot_case as case
from conftest import DevArray

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-12, 1e-250


def report(tag, got, want):
    dev = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
    dev = np.where(want == 0, np.abs(got), dev)
    print('%s: worst relative deviation %.3e at %s' % (tag, dev.max(), np.unravel_index(dev.argmax(), dev.shape)))


@pytest.fixture(scope='module')
def g():
    return case.g20()


@pytest.fixture(scope='module')
def survey():
    return case.cut_last_template(case.golden_survey())


@pytest.fixture(scope='module')
def eng():
    from frankenz_amd.engine import get_engine
    return get_engine()


# ---- 1. G20 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('red,key', [('madau+99', 'grid_madau'), (None, 'grid_none')])
def test_model_grid_against_the_reference(g, survey, red, key):
    survey.make_model_grid(g['zgrid'], red_fn=red, verbose=False)
    got, want = survey.models['data'], g[key]
    assert got.shape == want.shape
    report('GPU %s (z, template, filter)' % key, got, want)
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)
    assert np.array_equal(got == 0, want == 0)


@pytest.mark.parametrize('red', ['madau+99', None])
def test_sample_phot_against_the_reference_and_the_host(g, survey, red):
    survey.load_prior('bpz')
    out = {}
    for dev in (None, 'cpu'):
        survey.data = {k: g['mock_' + k].copy() for k in ('refmags', 'types', 'templates', 'redshifts')}
        survey.NOBJ = 300
        rs = case.restore_state(g, 'params_state')
        survey.sample_phot(red_fn=red, rstate=rs, verbose=False, device=dev)
        out[dev] = dict(survey.data)
        if red is not None:
            assert case.same_state(rs, g, 'phot_state')
    d, h = out[None], out['cpu']
    bad = np.isinf(h['refmags'])
    assert np.array_equal(np.isinf(d['refmags']), bad)
    assert np.isneginf(d['phot_true'][bad]).all() and np.isneginf(d['phot_obs'][bad]).all()
    report('GPU sample_phot(red_fn=%r) against the host path' % red, d['phot_true'][~bad], h['phot_true'][~bad])
    np.testing.assert_allclose(d['phot_true'][~bad], h['phot_true'][~bad], rtol=RTOL, atol=ATOL)
    if red is not None:
        assert np.array_equal(bad, np.isinf(g['mock_refmags_after'])) and bad.sum() >= 1
        report('GPU sample_phot against G20', d['phot_true'][~bad], g['mock_phot_true'][~bad])
        np.testing.assert_allclose(d['phot_true'][~bad], g['mock_phot_true'][~bad], rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(d['phot_obs'][~bad], g['mock_phot_obs'][~bad], rtol=1e-9, atol=1e-12 * g['mock_phot_err'].max())
        assert np.array_equal(d['phot_err'], g['mock_phot_err'])


# ---- 2. the smallest shapes at which the kernel can go wrong, against the host path ---------------------------------------------
# filters of 2, 63, 64, 65 and 129 points (the lane stride's edges); templates of 2 points, 300 points, more points than the LDS
# budget (global-memory search), and a narrow one (4000-6000 A) beyond whose ends whole bands lie
@pytest.fixture(scope='module')
def odd():
    from frankenz_amd import simulate
    ms = case.synthetic_survey([2, 63, 64, 65, 129], [2, 300, 9001], seed=3)
    narrow = case.synthetic_survey([2], [50], seed=4, tmpl_range=(4000., 6000.)).templates[0]
    ms.templates.append(narrow)
    ms.NTEMPLATE = 4
    tb = simulate._Tables(ms.filters, ms.templates)
    rs = np.random.RandomState(5)
    tmpl = rs.randint(0, 4, 257)
    tmpl[:8] = [3, 0, 2, 1, 3, 2, 0, 1]
    z = rs.uniform(0., 4., 257)
    z[:4] = 0.                                                   # z = 0 for every template
    z[4] = 0.                                                    # narrow template: bands 0 and 4 lie wholly beyond its ends
    assert tb.flw[tb.foff[1] - 1] < tb.tlw[tb.toff[3]] and tb.flw[tb.foff[4]] > tb.tlw[-1]
    z[5:8] = [3.9, 2.5, 1.7]
    return ms, tb, tmpl.astype(np.int64), z


def run(eng, tb, tmpl, z, igm, out=None):
    eng.synphot_upload(tb)
    out = np.full((len(tmpl), tb.Nf), -7.) if out is None else out
    eng.synphot(tmpl, z, np.log(1 + z), igm, out)
    return out


@pytest.mark.parametrize('igm', [0, 1])
def test_odd_shapes_against_the_host_path(eng, odd, igm):
    from frankenz_amd import simulate
    ms, tb, tmpl, z = odd
    want = simulate._synphot_host(tb, tmpl, z, np.log(1 + z), igm)
    got = run(eng, tb, tmpl, z, igm)
    assert np.isfinite(want).all() and (want > 0).all()
    report('GPU against the host path, igm %d (pair, filter)' % igm, got, want)
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)
    # bands wholly beyond an end of the narrow template see its end value only: sinh(arcsinh(fnu_end)) times the weights' sum, 1
    fnu = ms.templates[3]['fnu']
    np.testing.assert_allclose(got[4, [0, 4]], [fnu[0], fnu[-1]], rtol=1e-13)
    # one pair, and every template alone
    for p in (0, 1, 2, 3):
        one = run(eng, tb, tmpl[p:p + 1], z[p:p + 1], igm)
        assert np.array_equal(one, got[p:p + 1])
    # through the public interface
    ms.make_model_grid([0., 1.3], red_fn='madau+99' if igm else None, verbose=False)
    ms2 = ms.models['data'].copy()
    ms.make_model_grid([0., 1.3], red_fn='madau+99' if igm else None, verbose=False, device='cpu')
    np.testing.assert_allclose(ms2, ms.models['data'], rtol=RTOL, atol=ATOL)


def test_results_are_reproducible_and_independent_of_the_other_pairs(eng, odd):
    ms, tb, tmpl, z = odd
    a = run(eng, tb, tmpl, z, 1)
    b = run(eng, tb, tmpl, z, 1)
    assert np.array_equal(a, b)
    rs = np.random.RandomState(6)
    sub = rs.permutation(257)[:100]                              # a subset, in another order
    c = run(eng, tb, tmpl[sub], z[sub], 1)
    assert np.array_equal(c, a[sub])
    # cut into chunks by the smallest workspace (1 MiB: 13 107 pairs of these 5 filters at a time): the same bits
    eng.set_workspace_limit(1 << 20)
    try:
        d = run(eng, tb, np.tile(tmpl, 60), np.tile(z, 60), 1)
    finally:
        eng.set_workspace_limit(32 << 30)
    assert np.array_equal(d, np.tile(a, (60, 1)))


def test_output_into_a_device_array(eng, odd):
    ms, tb, tmpl, z = odd
    want = run(eng, tb, tmpl, z, 1)
    dev = DevArray(np.full((257, tb.Nf), -7.))
    run(eng, tb, tmpl, z, 1, out=dev)
    got = np.empty((257, tb.Nf))
    assert eng.lib.fz_dev_copy(eng.h, C.c_void_p(got.ctypes.data), C.c_void_p(dev.data_ptr()), got.nbytes) == 0
    assert np.array_equal(got, want)
    own = eng.device_empty((257, tb.Nf))
    run(eng, tb, tmpl, z, 0, out=own)
    assert np.array_equal(own.numpy(), run(eng, tb, tmpl, z, 0))


def test_refusals_leave_the_output_untouched(eng, odd):
    from frankenz_amd import simulate
    ms, tb, tmpl, z = odd
    out = np.full((4, tb.Nf), -7.)
    t4, z4 = tmpl[:4].copy(), z[:4] + 0.5
    with pytest.raises(IndexError, match='template 4 of 4'):
        run(eng, tb, np.array([0, 1, 4, 2]), z4, 1, out=out)
    with pytest.raises(IndexError, match='template -1'):
        run(eng, tb, np.array([0, -1, 1, 2]), z4, 1, out=out)
    for bad in (-1.5, np.nan, np.inf):
        zz = z4.copy()
        zz[2] = bad
        with pytest.raises(ValueError, match='pair 2: 1 \\+ z'), np.errstate(all='ignore'):
            run(eng, tb, t4, zz, 1, out=out)
    assert (out == -7.).all()
    # tables that are refused at upload leave nothing uploaded: the call that follows is refused as well
    for what, edit, msg in (('templates', lambda t: t.update(wavelength=t['wavelength'][:1], fnu=t['fnu'][:1]), 'template 1 has 1 points'),
                            ('templates', lambda t: t['wavelength'].__setitem__(3, 0.), 'template 1: wavelength 3 is not positive'),
                            ('templates', lambda t: t['wavelength'].__setitem__(5, t['wavelength'][3]), 'template 1: wavelengths decrease at point 5'),
                            ('filters', lambda f: f.update(wavelength=f['wavelength'][:1], frequency=f['frequency'][:1],
                                                           transmission=f['transmission'][:1]), 'filter 1 has 1 points'),
                            ('filters', lambda f: f['wavelength'].__setitem__(2, -1.), 'filter 1: wavelength 2 is not positive')):
        bad_ms = case.synthetic_survey([16, 9], [40, 30])
        edit(getattr(bad_ms, what)[1])
        with np.errstate(all='ignore'):
            bad_tb = simulate._Tables(bad_ms.filters, bad_ms.templates)
        with pytest.raises(ValueError, match=msg):
            eng.synphot_upload(bad_tb)
        with pytest.raises(RuntimeError, match='no filters and templates uploaded'):
            eng.synphot(t4 * 0, z4, np.log(1 + z4), 1, out)
        with pytest.raises(ValueError, match=msg):
            bad_ms.make_model_grid([0.5], verbose=False)
    assert (out == -7.).all()
    # ... and a good upload works again
    assert np.array_equal(run(eng, tb, t4, z4, 1), run(eng, tb, tmpl[:6], np.r_[z4, z[4:6]], 1)[:4])
