"""Host side of frankenz_amd.plotting (no GPU): the NumPy restatement tests/_diag_ref.py against the reference's recorded
results (G19), the object-selection helper, the one-call normal stream, the refusals, and the lazy matplotlib import."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _diag_ref as ref
from conftest import ROOT, load_golden

U = 2.0 ** -53


@pytest.fixture(scope='module')
def g19():
    g = load_golden('g19_diagnostics')
    return g, ref.StoredDict(g)


def _same_stack(got, want, rtol):
    assert np.array_equal(got == 0, want == 0)                  # the same zero set
    np.testing.assert_allclose(got, want, rtol=rtol, atol=0)


CASES = {
    'stack_default': lambda g: {},
    'stack_harsh': lambda g: dict(pdf_wt_thresh=g['harsh'][0], wt_thresh=g['harsh'][1]),
    'stack_obj_cdf': lambda g: dict(wt_thresh=None, cdf_thresh=float(g['obj_cdf_thresh'])),
    'stack_pdf_cdf': lambda g: dict(pdf_wt_thresh=None, pdf_cdf_thresh=float(g['pdf_cdf_thresh'])),
}


@pytest.mark.parametrize('name', sorted(CASES))
def test_restatement_stacks_against_g19(g19, name):
    g, d = g19
    got = ref.input_vs_pdf(g['vals'], g['errs'], d, g['pdfs'], g['pgrid'], weights=g['weights'], **CASES[name](g))
    _same_stack(got, g[name], 1e-14)


@pytest.mark.parametrize('name,disp', [('dstack_default', None), ('dstack_scaled', lambda p, c: (p - c) / (1. + c))])
def test_restatement_recentred_stacks_against_g19(g19, name, disp):
    g, d = g19
    got = ref.input_vs_dpdf(g['vals'], g['errs'], d, g['pdfs'], g['pgrid'], g['pdf_cent'], g['dgrid'], weights=g['weights'],
                            disp=disp)
    _same_stack(got, g[name], 1e-14)


def test_restatement_pit_against_g19(g19):
    g, _ = g19
    nmc, nbins, seed = int(g['nmc']), int(g['nbins']), int(g['seed'])
    a = (g['vals'], g['errs'], g['pdfs'], g['pgrid'])
    assert np.array_equal(ref.cdf_draws(*a, nmc, np.random.RandomState(seed)), g['draws'])          # bit for bit
    n = ref.cdf_vs_epdf(*a, Nmc=nmc, weights=g['weights'], Nbins=nbins, rstate=np.random.RandomState(seed))
    assert np.array_equal(n, g['epdf_n'])
    x, y = ref.cdf_vs_ecdf(*a, Nmc=nmc, rstate=np.random.RandomState(seed))
    assert np.array_equal(x, g['ecdf_x']) and np.array_equal(y, g['ecdf_y'])


@pytest.mark.parametrize('name', ['stack_default', 'stack_harsh', 'stack_obj_cdf'])
def test_selection_helper_reproduces_g19_through_the_restatement(g19, name):
    """the (object, weight) pairs of ``plotting.stack_selection``, stacked one object at a time by the restatement, give the
    reference's stack: with the CDF rule that needs the weight of the loop position, not the object's own"""
    from frankenz_amd import plotting
    g, d = g19
    kw = CASES[name](g)
    okw = {k: v for k, v in kw.items() if k in ('wt_thresh', 'cdf_thresh')}
    pkw = {k: v for k, v in kw.items() if k.startswith('pdf_')}
    objids, weff, cent, eidx = plotting.stack_selection(g['vals'], g['errs'], d, g['weights'], **okw)
    ci, ei = d.fit(g['vals'], g['errs'])
    assert np.array_equal(cent, ci[objids]) and np.array_equal(eidx, ei[objids])
    total = np.zeros_like(g[name])
    for o, w in zip(objids, weff):
        one = np.zeros(len(g['vals']))
        one[o] = 1.
        total += w * ref.input_vs_pdf(g['vals'], g['errs'], d, g['pdfs'], g['pgrid'], weights=one, wt_thresh=0.5, **pkw)
    _same_stack(total, g[name], 4 * len(objids) * U)
    if name == 'stack_obj_cdf':
        assert not np.array_equal(weff, g['weights'][objids])   # the quirk is exercised
        assert len(objids) < len(g['vals'])
    else:
        assert np.array_equal(weff, g['weights'][objids])


def test_selection_helper_without_thresholds_keeps_everything(g19):
    from frankenz_amd import plotting
    g, d = g19
    objids, weff, _, _ = plotting.stack_selection(g['vals'], g['errs'], d, g['weights'], wt_thresh=None, cdf_thresh=None)
    assert np.array_equal(objids, np.arange(len(g['vals']))) and np.array_equal(weff, g['weights'])
    objids, weff, _, _ = plotting.stack_selection(g['vals'], g['errs'], d)
    assert len(objids) == len(g['vals']) and (weff == 1.).all()


def test_one_normal_call_is_the_per_object_stream():
    from frankenz_amd import plotting
    rs = np.random.RandomState(3)
    vals, errs = rs.uniform(-1, 4, 57), rs.uniform(0, 0.5, 57)
    errs[5] = 0.
    a, b = np.random.RandomState(77), np.random.RandomState(77)
    got = plotting._mc_truths(vals, errs, 9, a)
    want = np.array([b.normal(v, e, size=9) for v, e in zip(vals, errs)])
    assert np.array_equal(got, want)
    sa, sb = a.get_state(), b.get_state()
    assert sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]


def test_refusals_before_any_device_work(g19):
    """every ValueError of the bookkeeping names the object; none of these calls reaches the device (there is none here)"""
    from frankenz_amd import plotting
    g, d = g19
    vals, errs, w, pdfs, pgrid = g['vals'].copy(), g['errs'].copy(), g['weights'].copy(), g['pdfs'].copy(), g['pgrid']
    for name, arr in (('vals', vals), ('errs', errs), ('weights', w)):
        for bad in (np.nan, np.inf):
            keep = arr[11]
            arr[11] = bad
            with pytest.raises(ValueError, match=r'`%s` of object 11 ' % name):
                plotting.input_vs_pdf(vals, errs, d, pdfs, pgrid, weights=w, plot=False)
            arr[11] = keep
    # a non-finite PDF entry of a selected object is refused, of a dropped object it is not looked at
    dropped = int(np.argmin(w))
    sel = plotting.stack_selection(vals, errs, d, w)
    assert dropped not in sel[0]
    pdfs[dropped, 3] = np.nan
    plotting._check_rows_finite(pdfs, sel[0])
    pdfs[40, 7] = np.inf
    with pytest.raises(ValueError, match='object 40 '):
        plotting.input_vs_pdf(vals, errs, d, pdfs, pgrid, weights=w, plot=False)
    with pytest.raises(ValueError, match='object 40 '):
        plotting.input_vs_dpdf(vals, errs, d, pdfs, pgrid, g['pdf_cent'], g['dgrid'], weights=w, plot=False)
    with pytest.raises(ValueError, match='object 40 '):
        plotting.cdf_vs_epdf(vals, errs, pdfs, pgrid, weights=w, plot=False, rstate=np.random.RandomState(1))
    pdfs = g['pdfs']
    # a window that does not meet the grid: far off either end with the narrowest kernel
    for v in (-2., 5.5):
        vals2, errs2 = vals.copy(), errs.copy()
        vals2[20], errs2[20] = v, 0.01
        with pytest.raises(ValueError, match='object 20: its window .* does not meet the grid'):
            plotting.input_vs_pdf(vals2, errs2, d, pdfs, pgrid, weights=w, plot=False)
    # ... but not for an object the weight rule drops
    vals2 = vals.copy()
    vals2[dropped], errs2 = -2., errs.copy()
    errs2[dropped] = 0.01
    assert dropped not in plotting.stack_selection(vals2, errs2, d, w)[0]
    # a malformed dictionary entry (one tap short, as the reference's slice makes them for kernels wider than half the grid)
    d2 = ref.StoredDict(g)
    e40 = int(d.fit(vals, errs)[1][40])
    d2.sigma_dict = list(d2.sigma_dict)
    d2.sigma_dict[e40] = d2.sigma_dict[e40][:-1]
    with pytest.raises(ValueError, match='dictionary entry %d is malformed' % e40):
        plotting.input_vs_pdf(vals, errs, d2, pdfs, pgrid, weights=w, plot=False)
    with pytest.raises(ValueError, match='shape'):
        plotting.input_vs_pdf(vals, errs, d, pdfs[:, :-1], pgrid, weights=w, plot=False)


def test_module_is_exported_with_the_reference_signatures():
    import inspect
    import frankenz_amd
    from frankenz_amd import plotting
    assert frankenz_amd.plotting is plotting and 'plotting' in frankenz_amd.__all__
    want = {
        'input_vs_pdf': ['vals', 'errs', 'vdict', 'pdfs', 'pgrid', 'weights', 'pdf_wt_thresh', 'pdf_cdf_thresh', 'wt_thresh',
                         'cdf_thresh', 'plot_thresh', 'cmap', 'smooth', 'plot_kwargs', 'verbose'],
        'input_vs_dpdf': ['vals', 'errs', 'vdict', 'pdfs', 'pgrid', 'pdf_cent', 'dgrid', 'weights', 'disp_func', 'disp_args',
                          'disp_kwargs', 'pdf_wt_thresh', 'pdf_cdf_thresh', 'wt_thresh', 'cdf_thresh', 'plot_thresh', 'cmap',
                          'smooth', 'plot_kwargs', 'verbose'],
        'cdf_vs_epdf': ['vals', 'errs', 'pdfs', 'pdf_grid', 'Nmc', 'weights', 'Nbins', 'plot_kwargs', 'rstate'],
        'cdf_vs_ecdf': ['vals', 'errs', 'pdfs', 'pdf_grid', 'Nmc', 'weights', 'plot_kwargs', 'rstate'],
    }
    defaults = dict(weights=None, pdf_wt_thresh=1e-3, pdf_cdf_thresh=2e-4, wt_thresh=1e-3, cdf_thresh=2e-4, plot_thresh=0.,
                    cmap='viridis', smooth=0, plot_kwargs=None, verbose=False, Nmc=100, Nbins=50, rstate=None, disp_func=None,
                    disp_args=None, disp_kwargs=None, device=None, plot=True)
    for name, names in want.items():
        ps = inspect.signature(getattr(plotting, name)).parameters
        pos = [p.name for p in ps.values() if p.kind == p.POSITIONAL_OR_KEYWORD]
        assert pos == names, name
        assert ps['device'].kind == ps['device'].KEYWORD_ONLY and ps['plot'].kind == ps['plot'].KEYWORD_ONLY
        for p in ps.values():
            if p.default is not p.empty:
                assert p.default == defaults[p.name], (name, p.name)


def test_importing_and_refusing_imports_no_matplotlib():
    """``frankenz_amd.plotting`` imports matplotlib (and scipy.ndimage) inside the functions only: a fresh process that imports the
    module and runs the host side of a ``plot=False`` call up to its refusal has neither loaded"""
    code = ("import sys, numpy as np\n"
            "sys.path.insert(0, %r)\n"
            "from frankenz_amd import plotting, PDFDict\n"
            "d = PDFDict(np.linspace(0., 3., 150), np.linspace(0.01, 0.28, 28))\n"
            "p = np.ones((4, 10)) / 10.\n"
            "plotting.stack_selection(np.ones(4), np.full(4, 0.1), d)\n"
            "try:\n"
            "    plotting.input_vs_pdf(np.array([1., 1., np.nan, 1.]), np.full(4, 0.1), d, p, np.arange(10.), plot=False)\n"
            "except ValueError:\n"
            "    pass\n"
            "else:\n"
            "    raise SystemExit('no refusal')\n"
            "assert 'matplotlib' not in sys.modules and 'scipy.ndimage' not in sys.modules, sorted(m for m in sys.modules if 'matplotlib' in m)[:3]\n"
            "print('clean')\n" % ROOT)
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, cwd=ROOT,
                         env=dict(os.environ, PYTHONDONTWRITEBYTECODE='1'))
    assert out.returncode == 0 and out.stdout.strip() == 'clean', out.stderr[-2000:]
