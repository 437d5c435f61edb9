"""k_hist's screen form keeps the scalar state of its per-object prologue and finish out of the model loop and settles with a leaner
instruction stream (docs/k_hist.md, "Scalar state and the settle's instruction stream").  No arithmetic operation and no order of
operations changed, so the expectation is what the kernel gave BEFORE the change, bit for bit: tests/golden/hist_lean_*.npz were
recorded from a build of the commit in front of it through Engine.fit_predict_prior (tools/record_hist_lean.py writes them from
`compute` below).  Every case also names the kernel form it ran, and 12 of its objects are held against the oracle, so that a
fixture recorded from a wrong build could not pass.

All cases: 5 bands, band-constant model errors, wt_thresh 1e-3, seeded.  M = 65 is a single partial tile, 769 two full 384-model
tiles and a one-model tail, 3000 eight tiles; 48 objects hold a training-set self match (two), an object nothing fits within 2^-400
of the mode (handed to the sweep), two objects with negative fluxes at ten times the noise (best weight 0.07 of the mode's: a wide
ambiguous band under the stacked pairs; and 1e-5 of it, below wt_thresh: every pair that matters waits in the ambiguous list) and 16 identical objects.  `rounds` has
more objects than one round of the launch holds (2 R + 37, R = 16 waves x CUs) and keeps the PDFs of 32 seeded rows."""
import os

import numpy as np
import pytest

import frankenz_oracle as fo
from conftest import EVID64, SDSS_SIGMA

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
# name: (M, lprob_kwargs, share of unobserved object bands, seed)
CASES = {'M65': (65, {}, 0.0, 61), 'M769': (769, {}, 0.0, 62), 'M3000': (3000, {}, 0.0, 63),
         'M769_Ai': (769, {'ignore_model_err': True}, 0.0, 64), 'M769_objk': (769, {}, 0.02, 65),
         'rounds': (1000, {}, 0.0, 66)}
SELF, MISFIT, POOR, SAME = (3, 5), 11, (13, 14), np.arange(20, 36)
ORACLE_ROWS = np.array([0, 1, 2, 3, 5, 11, 13, 14, 20, 21, 40, 47])
_cache = {}


def engine():
    from frankenz_amd.engine import get_engine
    return get_engine()


def dicts():
    if 'dicts' not in _cache:
        from frankenz_amd import PDFDict
        grid, sg = np.arange(0, 7 + 1e-5, .02), np.linspace(.005, 2, 500)
        _cache['dicts'] = (PDFDict(grid, sg), fo.KernelDict(grid, sg))
    return _cache['dicts']


def fixture_path(name):
    return os.path.join(GOLDEN, 'hist_lean_%s.npz' % name)


def problem(name, N=None):
    """objects at 0.05 / 1 / 10 x the SDSS noise, interleaved, and the special ones of the module's docstring"""
    M, kw, mask, seed = CASES[name]
    if N is None:
        N = int(np.load(fixture_path(name))['N']) if name == 'rounds' else 48
    rs = np.random.RandomState(seed)
    B = 5
    Y = rs.lognormal(1., 1., size=(M, B))
    Ye = np.tile(SDSS_SIGMA, (M, 1))
    Ym = np.ones((M, B))
    scale = np.array([0.05, 1., 10.])[np.arange(N) % 3][:, None]
    X = Y[rs.randint(0, M, N)] + scale * SDSS_SIGMA * rs.standard_normal((N, B))
    Xe = scale * np.tile(SDSS_SIGMA, (N, 1))
    Xm = np.ones((N, B))
    X[SELF[0]], X[SELF[1]] = Y[0], Y[M - 1]
    X[MISFIT] = 1e6 + Y[0]
    for i, c in zip(POOR, (-1.5, -2.5)):
        Xe[i] = 10. * SDSS_SIGMA
        X[i] = c * Xe[i]
    X[SAME] = X[SAME[0]]; Xe[SAME] = Xe[SAME[0]]
    if mask > 0:
        Xm = (rs.uniform(size=(N, B)) >= mask).astype(float)
        Xm[[0, 1], [2, 4]] = 0.0                                  # (48 objects at 2 %: make sure some band IS unobserved)
        Xm[Xm.sum(axis=1) < 3] = 1.0
        X[Xm == 0] = -7e5                                         # garbage in the unobserved bands must not matter
    z = rs.uniform(0, 6, M); ze = np.full(M, 0.05)
    keep = np.sort(rs.choice(N, 32, replace=False)) if name == 'rounds' else np.arange(N)
    return dict(Y=Y, Ye=Ye, Ym=Ym, X=X, Xe=Xe, Xm=Xm, z=z, ze=ze, kw=kw, keep=keep)


def compute(pr):
    """one fit_predict into NaN-filled device buffers: PDFs of the kept rows, ln-max and ln-evidence of every object, kernel form"""
    from frankenz_amd.engine import DeviceArray, kde_opts, like_opts
    eng = engine()
    pd, _ = dicts()
    eng.upload_models(pr['Y'], pr['Ye'], pr['Ym'])
    G = eng.set_labels(pr['z'], pr['ze'], label_dict=pd)
    N = len(pr['X'])
    out = [DeviceArray(eng, (N, G)), DeviceArray(eng, (N, 1)), DeviceArray(eng, (N, 1))]
    for a in out:
        a.set_rows(0, np.full(a.shape, np.nan))
    eng.fit_predict_prior(pr['X'].copy(), pr['Xe'].copy(), pr['Xm'].copy(), like_opts(pr['kw']), kde_opts({}), None,
                          out[0], out[1], out[2], n=N)
    eng.sync()
    return dict(pdfs=out[0].numpy()[pr['keep']], lmap=out[1].numpy()[:, 0], levid=out[2].numpy()[:, 0], form=eng.last_form())


def same_bits(a, b):
    """equal as bit patterns up to the payload of a nan: the same nans and nowhere else, every other entry array_equal"""
    assert a.shape == b.shape
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb)
    assert np.array_equal(a[~na].view(np.int64), b[~nb].view(np.int64))


@pytest.mark.parametrize('name', list(CASES))
def test_bits_of_the_parent(name):
    want = np.load(fixture_path(name))
    pr = problem(name)
    got = compute(pr)
    N = len(pr['X'])
    if name == 'rounds':
        assert N > 16 * engine().cu_count()                       # more than one round
    assert got['form'] == str(want['form'])
    assert got['form'] == ('k_hist<screen> (per-object band counts)' if name == 'M769_objk' else 'k_hist<screen>')
    for k in ('lmap', 'levid', 'pdfs'):
        assert np.array_equal(got[k], want[k], equal_nan=True), k
        same_bits(got[k], want[k])
    # the identical objects: identical rows (in `rounds` the kept rows are seeded ones, so there ln-max and ln-evidence only)
    for k in ('lmap', 'levid') + (() if name == 'rounds' else ('pdfs',)):
        assert (got[k][SAME] == got[k][SAME[0]]).all()
    assert not np.isnan(got['lmap']).any() and not np.isnan(got['levid']).any()
    # the poorly fitted object sits where the docstring says: best weight below wt_thresh of the mode's, yet far above 2^-400
    if name in ('M769', 'M3000'):
        assert -40. < got['lmap'][POOR[1]] - fo_mode_lnl() < np.log(1e-3) < got['lmap'][POOR[0]] - fo_mode_lnl() < -1.
    # 12 objects against the oracle
    _, od = dicts()
    idx = ORACLE_ROWS
    with np.errstate(all='ignore'):
        rp, rlm, rle = fo.bruteforce_fit_predict(pr['X'][idx].copy(), pr['Xe'][idx].copy(), pr['Xm'][idx].copy(), pr['Y'], pr['Ye'], pr['Ym'],
                                                 pr['z'], pr['ze'], label_dict=od, **pr['kw'])
    if name != 'rounds':
        np.testing.assert_allclose(got['pdfs'][idx], rp, rtol=1e-7, atol=1e-13)
    np.testing.assert_allclose(got['lmap'][idx], rlm, rtol=1e-9)
    np.testing.assert_allclose(got['levid'][idx], rle, **EVID64)


def fo_mode_lnl():
    """ln of the 5-band dimensionality-prior likelihood at its mode chi2 = k = 3: (k / 2) ln k - k / 2 - ln(2^(5/2) Gamma(5/2))"""
    from math import lgamma, log
    return 1.5 * log(3.) - 1.5 - (2.5 * log(2.) + lgamma(2.5))
